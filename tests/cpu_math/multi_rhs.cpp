// CPU check of the column-tiled ("multi right-hand-side") algebra of parallel-gps_amd/csrc/pgps_math.h (TEST TOOL, not a
// product path): filt_extend_m / filt_combine_m / filt_apply_m / smth_combine_m / smth_apply_m at MC = 4 against four runs of
// the single-column functions on the same operands.  The shared parts (A, C, J; E, L; P) must come out bit-identical, the
// column parts (b, eta; g; m) are compared by the caller.  Built by tests/test_multi_output_host.py with g++.
#include <cstring>

#include "pgps_math.h"

using namespace pgps;

namespace {
constexpr int MC = 4;
constexpr int kPerCase = 256;       // doubles of the random stream one case may consume

struct Stream {
    const double* p;
    double next() { return *p++; }
};

// a well-conditioned symmetric positive definite matrix, packed: G G^T / D + 0.5 I
template <int D>
void spd(Stream& r, double* sym) {
    double G[D * D];
    for (int i = 0; i < D * D; ++i) G[i] = r.next();
    for (int i = 0; i < D; ++i)
        for (int j = i; j < D; ++j) {
            double acc = (i == j) ? 0.5 : 0.0;
            for (int k = 0; k < D; ++k) acc += G[i * D + k] * G[j * D + k] / D;
            sym[symi<D>(i, j)] = acc;
        }
}

template <int D>
void random_filt(Stream& r, FiltElemM<double, D, MC>& m, FiltElem<double, D>* s) {
    for (int i = 0; i < D * D; ++i) m.A[i] = 0.6 * r.next();
    spd<D>(r, m.C);
    spd<D>(r, m.J);
    for (int c = 0; c < MC; ++c)
        for (int i = 0; i < D; ++i) { m.b[c][i] = r.next(); m.eta[c][i] = r.next(); }
    for (int c = 0; c < MC; ++c) {
        std::memcpy(s[c].A, m.A, sizeof(m.A));
        std::memcpy(s[c].C, m.C, sizeof(m.C));
        std::memcpy(s[c].J, m.J, sizeof(m.J));
        for (int i = 0; i < D; ++i) { s[c].b[i] = m.b[c][i]; s[c].eta[i] = m.eta[c][i]; }
    }
}

template <int D>
void random_smth(Stream& r, SmthElemM<double, D, MC>& m, SmthElem<double, D>* s) {
    for (int i = 0; i < D * D; ++i) m.E[i] = 0.6 * r.next();
    spd<D>(r, m.L);
    for (int c = 0; c < MC; ++c)
        for (int i = 0; i < D; ++i) m.g[c][i] = r.next();
    for (int c = 0; c < MC; ++c) {
        std::memcpy(s[c].E, m.E, sizeof(m.E));
        std::memcpy(s[c].L, m.L, sizeof(m.L));
        for (int i = 0; i < D; ++i) s[c].g[i] = m.g[c][i];
    }
}

struct Result {
    long shared_mismatch = 0;       // cases x columns whose shared part differs in some bit
    double col_err = 0.0;           // max |multi - single| / max(1, |single|) over the column parts
    void shared(const void* a, const void* b, size_t n) { if (std::memcmp(a, b, n) != 0) ++shared_mismatch; }
    void col(double got, double want) {
        const double aw = want < 0 ? -want : want, d = got - want, ad = d < 0 ? -d : d;
        const double e = ad / (aw > 1.0 ? aw : 1.0);
        if (!(e <= col_err)) col_err = e;           // (a NaN sticks)
    }
};

template <int D>
void compare_filt(const FiltElemM<double, D, MC>& m, const FiltElem<double, D>* s, Result& res) {
    for (int c = 0; c < MC; ++c) {
        res.shared(m.A, s[c].A, sizeof(m.A));
        res.shared(m.C, s[c].C, sizeof(m.C));
        res.shared(m.J, s[c].J, sizeof(m.J));
        for (int i = 0; i < D; ++i) { res.col(m.b[c][i], s[c].b[i]); res.col(m.eta[c][i], s[c].eta[i]); }
    }
}
template <int D>
void compare_smth(const SmthElemM<double, D, MC>& m, const SmthElem<double, D>* s, Result& res) {
    for (int c = 0; c < MC; ++c) {
        res.shared(m.E, s[c].E, sizeof(m.E));
        res.shared(m.L, s[c].L, sizeof(m.L));
        for (int i = 0; i < D; ++i) res.col(m.g[c][i], s[c].g[i]);
    }
}

// op: 0 = extend by an observed step, 1 = extend by a missing step, 2 = filt_combine, 3 = filt_apply, 4 = smth_combine,
// 5 = smth_apply
template <int D>
void run(int op, const double* stream, long n, Result& res) {
    for (long it = 0; it < n; ++it) {
        Stream r{stream + it * kPerCase};
        if (op <= 1) {
            FiltElemM<double, D, MC> m;
            FiltElem<double, D> s[MC];
            random_filt<D>(r, m, s);
            double F[D * D], Q[Dim<D>::SYM], h[D], y[MC];
            for (int i = 0; i < D * D; ++i) F[i] = 0.5 * r.next();
            spd<D>(r, Q);
            for (int i = 0; i < D; ++i) h[i] = (i == 0) ? 1.0 : 0.3 * r.next();
            for (int c = 0; c < MC; ++c) y[c] = r.next();
            const double R = 0.1, nan = __builtin_nan("");
            filt_extend_m(m, F, Q, y, op == 0, h, R);
            for (int c = 0; c < MC; ++c) filt_extend(s[c], F, Q, op == 0 ? y[c] : nan, h, R);
            compare_filt<D>(m, s, res);
        } else if (op == 2) {
            FiltElemM<double, D, MC> m1, m2, mo;
            FiltElem<double, D> s1[MC], s2[MC], so[MC];
            random_filt<D>(r, m1, s1);
            random_filt<D>(r, m2, s2);
            filt_combine_m(m1, m2, mo);
            for (int c = 0; c < MC; ++c) filt_combine(s1[c], s2[c], so[c]);
            compare_filt<D>(mo, so, res);
        } else if (op == 3) {
            FiltElemM<double, D, MC> m2;
            FiltElem<double, D> s2[MC];
            random_filt<D>(r, m2, s2);
            MeanCovM<double, D, MC> ms;
            MeanCov<double, D> ss[MC];
            spd<D>(r, ms.P);
            for (int c = 0; c < MC; ++c)
                for (int i = 0; i < D; ++i) ms.m[c][i] = r.next();
            for (int c = 0; c < MC; ++c) {
                std::memcpy(ss[c].P, ms.P, sizeof(ms.P));
                for (int i = 0; i < D; ++i) ss[c].m[i] = ms.m[c][i];
            }
            filt_apply_m(ms, m2);
            for (int c = 0; c < MC; ++c) {
                filt_apply(ss[c], s2[c]);
                res.shared(ms.P, ss[c].P, sizeof(ms.P));
                for (int i = 0; i < D; ++i) res.col(ms.m[c][i], ss[c].m[i]);
            }
        } else if (op == 4) {
            SmthElemM<double, D, MC> m1, m2, mo;
            SmthElem<double, D> s1[MC], s2[MC], so[MC];
            random_smth<D>(r, m1, s1);
            random_smth<D>(r, m2, s2);
            smth_combine_m(m1, m2, mo);
            for (int c = 0; c < MC; ++c) smth_combine(s1[c], s2[c], so[c]);
            compare_smth<D>(mo, so, res);
        } else {
            SmthElemM<double, D, MC> m1;
            SmthElem<double, D> s1[MC];
            random_smth<D>(r, m1, s1);
            MeanCovM<double, D, MC> ms;
            MeanCov<double, D> ss[MC];
            spd<D>(r, ms.P);
            for (int c = 0; c < MC; ++c)
                for (int i = 0; i < D; ++i) ms.m[c][i] = r.next();
            for (int c = 0; c < MC; ++c) {
                std::memcpy(ss[c].P, ms.P, sizeof(ms.P));
                for (int i = 0; i < D; ++i) ss[c].m[i] = ms.m[c][i];
            }
            smth_apply_m(m1, ms);
            for (int c = 0; c < MC; ++c) {
                smth_apply(s1[c], ss[c]);
                res.shared(ms.P, ss[c].P, sizeof(ms.P));
                for (int i = 0; i < D; ++i) res.col(ms.m[c][i], ss[c].m[i]);
            }
        }
    }
}
}  // namespace

// stream: n * 256 standard normals.  out[0] = comparisons of a shared part that differ in some bit, out[1] = largest relative
// error of a column part.  Returns 0, or -1 for a d / op it does not know.
extern "C" int multi_rhs_check(int d, int op, const double* stream, long n, double* out) {
    if (op < 0 || op > 5) return -1;
    Result res;
    if (d == 1) run<1>(op, stream, n, res);
    else if (d == 2) run<2>(op, stream, n, res);
    else if (d == 3) run<3>(op, stream, n, res);
    else return -1;
    out[0] = (double)res.shared_mismatch;
    out[1] = res.col_err;
    return 0;
}
