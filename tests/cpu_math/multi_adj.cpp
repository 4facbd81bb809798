// CPU run of the column-tiled adjoint pass of parallel-gps_amd/csrc/pgps_math.h (TEST TOOL, not a product path): a whole
// sequential forward and reverse sweep with adj_step_m / adj_filtered_m / adj_element_m / adj_reverse_m at MC = 4, the
// transition matrices F_k and the process noises Q_k handed in by the caller.  Besides the statistics it reports
//   * whether the shared parts (E, L) of every step's adjoint element are bit-identical to the single-column element
//     (restated below from gp_gfwd_body of pgps_gpadj.hip.h, which is device code) of a single-column filter over the same
//     series, with L scaled by the number of columns that exist;
//   * how far the scan form -- the suffix of the elements, folded with smth_combine_m and applied to (0, 0) with smth_apply_m --
//     is from the (a_c, B) the sequential sweep carries.
// Built by tests/test_multi_grad_host.py with g++.
#include <cstring>
#include <vector>

#include "pgps_math.h"

using namespace pgps;

namespace {
constexpr int MC = 4;

// the single-column step and its adjoint element, as adj_step and gp_gfwd_body (pgps_gpadj.hip.h) compute them
template <int D>
void single_element(const double* F, const double* Q, MeanCov<double, D>& s, double y, const double* h, double R, double* E,
                    double* L) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM;
    double FP[MAT], mp[D], Pp[SYM], u[D], K[D];
    mat_vec<double, D>(F, s.m, mp);
    predict_cov<double, D>(F, s.P, Q, FP, Pp);
    sym_vec<double, D>(Pp, h, u);
    double S = R, mu = 0.0;
    for (int i = 0; i < D; ++i) { S += h[i] * u[i]; mu += h[i] * mp[i]; }
    const bool obs = !is_nan(y);
    const double inv = obs ? recip(S) : 0.0;
    const double r = obs ? y - mu : 0.0;
    for (int i = 0; i < D; ++i) K[i] = u[i] * inv;
    for (int i = 0; i < D; ++i) s.m[i] = mp[i] + K[i] * r;
    for (int i = 0; i < D; ++i)
        for (int j = i; j < D; ++j) s.P[symi<D>(i, j)] = Pp[symi<D>(i, j)] - u[i] * u[j] * inv;
    double v[D];
    for (int j = 0; j < D; ++j) {
        double acc = 0.0;
        for (int i = 0; i < D; ++i) acc += h[i] * F[i * D + j];
        v[j] = acc;
    }
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) E[j * D + i] = F[i * D + j] - K[i] * v[j];
    for (int i = 0; i < D; ++i)
        for (int j = i; j < D; ++j) L[symi<D>(i, j)] = -0.5 * v[i] * v[j] * inv;
}

struct MaxRel {
    double diff = 0.0, ref = 0.0;
    void add(double got, double want) {
        const double d = got - want, ad = d < 0 ? -d : d, aw = want < 0 ? -want : want;
        if (!(ad <= diff)) diff = ad;               // (a NaN sticks)
        if (aw > ref) ref = aw;
    }
};

template <int D>
void sweep(long n, int nc, const double* Fs, const double* Qs, const double* dts, const double* Pinf, const double* h, double R,
           const double* Y, double* stats, double* ll, double* chk) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM, NST = MAT + 2 * D + 1;
    double P0[SYM];
    for (int i = 0; i < D; ++i)
        for (int j = i; j < D; ++j) P0[symi<D>(i, j)] = 0.5 * (Pinf[i * D + j] + Pinf[j * D + i]);
    MeanCovM<double, D, MC> s;
    MeanCov<double, D> single[MC];
    for (int i = 0; i < SYM; ++i) s.P[i] = P0[i];
    for (int c = 0; c < MC; ++c) {
        for (int i = 0; i < D; ++i) { s.m[c][i] = 0.0; single[c].m[i] = 0.0; }
        for (int i = 0; i < SYM; ++i) single[c].P[i] = P0[i];
    }
    std::vector<AdjStepM<double, D, MC>> steps((size_t)n);
    std::vector<SmthElemM<double, D, MC>> elems((size_t)n);
    LogLikM<MC> acc;
    long mismatch = 0;
    for (long k = 0; k < n; ++k) {
        double y[MC], Q[SYM];
        for (int c = 0; c < MC; ++c) y[c] = c < nc ? Y[k * nc + c] : 0.0;
        const bool obs = !is_nan(y[0]);
        for (int i = 0; i < D; ++i)
            for (int j = i; j < D; ++j) Q[symi<D>(i, j)] = Qs[k * MAT + i * D + j];
        AdjStepM<double, D, MC>& st = steps[(size_t)k];
        adj_step_m<double, D, MC>(Fs + k * MAT, Q, s, y, obs, h, R, st);
        if (obs) acc.add(st.r, st.S);
        adj_filtered_m(st, s);
        adj_element_m(st, h, nc, elems[(size_t)k]);
        for (int c = 0; c < nc; ++c) {
            double E[MAT], L[SYM];
            single_element<D>(Fs + k * MAT, Q, single[c], y[c], h, R, E, L);
            for (int i = 0; i < SYM; ++i) L[i] = L[i] * (double)nc;
            if (std::memcmp(E, elems[(size_t)k].E, sizeof(E)) != 0) ++mismatch;
            if (std::memcmp(L, elems[(size_t)k].L, sizeof(L)) != 0) ++mismatch;
        }
    }
    for (int c = 0; c < nc; ++c) ll[c] = acc.value(c);

    double av[MC][D], B[SYM], st_[NST];
    for (int c = 0; c < MC; ++c)
        for (int i = 0; i < D; ++i) av[c][i] = 0.0;
    for (int i = 0; i < SYM; ++i) B[i] = 0.0;
    for (int i = 0; i < NST; ++i) st_[i] = 0.0;
    SmthElemM<double, D, MC> suf;
    smth_identity_m(suf);
    MaxRel scan_a, scan_B;
    for (long k = n - 1; k >= 0; --k) {
        // (a_c, B) behind step k, from the scan form
        MeanCovM<double, D, MC> z;
        for (int i = 0; i < SYM; ++i) z.P[i] = 0.0;
        for (int c = 0; c < MC; ++c)
            for (int i = 0; i < D; ++i) z.m[c][i] = 0.0;
        smth_apply_m(suf, z);
        double Bs[SYM];
        adj_cov_from_scan_m(z, Bs);
        for (int c = 0; c < MC; ++c)
            for (int i = 0; i < D; ++i) scan_a.add(z.m[c][i], av[c][i]);
        for (int i = 0; i < SYM; ++i) scan_B.add(Bs[i], B[i]);
        adj_reverse_m<double, D, MC>(steps[(size_t)k], dts[k], h, P0, nc, av, B, st_);
        SmthElemM<double, D, MC> r;
        smth_combine_m(elems[(size_t)k], suf, r);
        suf = r;
    }
    for (int i = 0; i < NST; ++i) stats[i] = st_[i];
    chk[0] = (double)mismatch;
    chk[1] = scan_a.ref > 0.0 ? scan_a.diff / scan_a.ref : scan_a.diff;
    chk[2] = scan_B.ref > 0.0 ? scan_B.diff / scan_B.ref : scan_B.diff;
    // an absent column must have stayed at zero
    double absent = 0.0;
    for (int c = nc; c < MC; ++c)
        for (int i = 0; i < D; ++i) {
            const double a = av[c][i] < 0 ? -av[c][i] : av[c][i], m = s.m[c][i] < 0 ? -s.m[c][i] : s.m[c][i];
            if (!(a <= absent)) absent = a;
            if (!(m <= absent)) absent = m;
        }
    chk[3] = absent;
}
}  // namespace

// Fs, Qs (n, d, d), dts (n), Pinf (d, d), h (d), Y (n, nc) row-major with NaN rows (all columns or none).  stats (d d + 2 d + 1) =
// [Abar | Ubar | Hbar | Rbar] summed over the columns, ll (nc); chk[0] = shared parts (E, L) that differ in some bit from the
// single-column element's, chk[1], chk[2] = distance of the scan form's a_c / B from the sweep's (max-norm, relative),
// chk[3] = largest |a_c|, |m_c| of an absent column.  Returns 0, or -1 for a d / nc it does not know.
extern "C" int multi_adj_sweep(int d, long n, int nc, const double* Fs, const double* Qs, const double* dts, const double* Pinf,
                               const double* h, double R, const double* Y, double* stats, double* ll, double* chk) {
    if (nc < 1 || nc > MC || n < 1) return -1;
    if (d == 1) sweep<1>(n, nc, Fs, Qs, dts, Pinf, h, R, Y, stats, ll, chk);
    else if (d == 2) sweep<2>(n, nc, Fs, Qs, dts, Pinf, h, R, Y, stats, ll, chk);
    else if (d == 3) sweep<3>(n, nc, Fs, Qs, dts, Pinf, h, R, Y, stats, ll, chk);
    else return -1;
    return 0;
}
