// pgps_panel_gram.hip.h -- the whitened Gram matrix of C columns of EVERY series of a panel in ONE launch.
//
// With V_s = [y_s, Phi_s] (n_s rows, C = 1 + p columns) and K_y = K + diag(R + rs) = L L^T on the observed rows of series s,
// G_s = V_s^T K_y^-1 V_s = W^T W, W = L^-1 V_s, holds everything about the trend coefficients of that series: the GLS estimate,
// its covariance, the profile likelihood (pssgp/trend.py).  The single model forms G by the column-tiled Kalman
// pass over many workgroups (pgps_multi.hip.h, pgps_whiten.hip.h: scalar noise only); the panel kernels run one workgroup per
// series on one column (pgps_panel.hip.h, with a HET flag).  k_gpp_gram joins them:
//
//   grid (1, series of the group), blockIdx.y selects the series through its PanelDesc, as k_gpp_one does
//   rounds   the C columns run in rounds of the tile MC = MultiTile<D>::MC (8 / 4 / 2 at d = 1, 2, 3).  A round is the
//            one-workgroup multi-column reduce (FiltElemM through block_scan_exclusive: nblocks = 1, no spine is folded, the
//            lane's exclusive prefix stays in registers) and, behind the scan's closing barrier, the whitening Kalman pass of
//            k_gpm_whiten: w[k, c] = (V[k, c] - mu_c[k]) / sqrt(S_k) into the series' own slice of scratch, 0.0 at a missing row
//            (the slice is not zeroed).  The covariance part is recomputed per round, as the rounds of launch_gp_multi do;
//            the first round also yields sum log S_k and the count of observed steps.
//   Gram     after the last round and a barrier the same workgroup forms G = W^T W from its slice: lane t sums the products
//            of rows t, t + 256, .. in row order, a wave folds its lanes in a fixed shuffle tree, the four waves' totals are
//            added in wave order, and each entry i <= j is written to (i, j) and (j, i) from the one sum.  No floating-point
//            atomics: the summation order is fixed by (n, C) alone.
//   HET      the step's noise variance is R + rs[k], loaded next to t_k and the row of V.  kf_step_m, filt_first_m and
//            filt_extend_m take R by value: no math routine changes.
//   output   one record of C C + 2 doubles per series: [G (C, C) row-major | logdet | n_obs] (n_obs as a double: exact).
//
// A row of V that is NaN in column 0 is a missing step: the other columns are not read there and the row contributes nothing.
//
// The rules of pgps_panel.hip.h, as they hold here:
//   look-ahead   every load of ts / V / rs[k + 1] is guarded by the lane's own k + 1 < k1 <= N: row N is the NEIGHBOUR's first
//                row (past the allocation for the last series).  ts[k0 - 1] is read only where k0 > 0.
//   steps/lane   PanelDesc::Lc = max(1, ceil(n / 256)), or the pinned pgps_set_chunk value where it covers the series
//   slices       W (n, C) of a series starts at PanelDesc::o_fm, padded to kPanelAlign elements
//   groups       consecutive series whose slices fit pgps_set_batch_scratch (pgps_panel_gram_inst.hip)
//   bits         a record depends on that series' rows, its model row, C and the pinned chunk: its steps per lane are its
//                own, its scratch is its own and no arithmetic crosses workgroups -- not on the other series, its place, the
//                grouping, repetition, or nmodels (1 versus S equal rows)
//
// k_panel_residual: ys_out[k] = V[k, 0] - sum_j V[k, 1 + j] betas[s, j], summed left to right (NaN stays NaN), for the rows of
// series s.  fp64, d <= 3.
#pragma once

#include "pgps_multi.hip.h"

namespace pgps {

constexpr int kPanelGramTri = kPanelGramMax * (kPanelGramMax + 1) / 2;      // entries of G on or above the diagonal

// what one launch (one group of series) sees.  PanelDesc as launch_gp_panel fills it, with o_fm = the series' W slice
struct PanelGramArgs {
    const PanelDesc* desc;      // the group's records
    const double* models;       // (nmodels, kGpModelStride)
    const double* ts;           // concatenated times
    const double* V;            // (all rows, C) row-major
    const double* rs;           // per-observation noise variances, or null
    int C;                      // 1 .. kPanelGramMax
    double* w;                  // the group's scratch: ragged slices (n, C)
    double* out;                // (the group's series, C C + 2)
};

// row k of the series' V: column 0 decides whether the step is observed; the round's columns c0 .. c0 + nc - 1 are read at
// an observed row only, 0.0 elsewhere (what is loaded for an absent column never reaches a store)
template <int MC>
__device__ __forceinline__ bool panel_gram_load(const double* V, int C, int c0, int nc, long k, double* y) {
    const double* p = V + k * (long)C;
    const double v0 = p[0];
    const bool obs = !is_nan(v0);
#pragma unroll
    for (int c = 0; c < MC; ++c) y[c] = 0.0;
    if (obs) {
#pragma unroll
        for (int c = 0; c < MC; ++c)
            if (c < nc) y[c] = p[c0 + c];
    }
    return obs;
}

template <int D, bool HET>
__global__ __launch_bounds__(kBlock) void k_gpp_gram(const PanelGramArgs p) {
    constexpr int MC = MultiTile<D>::MC;
    constexpr int MAT = D * D, SYM = Dim<D>::SYM;
    using FE = FiltElemM<double, D, MC>;
    using MS = MeanCovM<double, D, MC>;
    __shared__ double lds[kWaves * FE::N];
    __shared__ double lds_ll[kWaves];
    __shared__ double red[kWaves * kPanelGramTri];
    const PanelDesc r = p.desc[blockIdx.y];
    const double* q = p.models + (long)r.model * kGpModelStride;
    GpModel<double> m;
    m.lam = q[0];
#pragma unroll
    for (int i = 0; i < 9; ++i) { m.N1[i] = 0.0; m.N2[i] = 0.0; m.Pinf[i] = 0.0; }
#pragma unroll
    for (int i = 0; i < MAT; ++i) { m.N1[i] = q[1 + i]; m.N2[i] = q[10 + i]; m.Pinf[i] = q[19 + i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) m.H[i] = i < D ? q[28 + i] : 0.0;
    // (the model in vector registers at d = 3, as k_gpm_reduce keeps it)
    if constexpr (D == 3) { pin_values(m.N1, MAT); pin_values(m.N2, MAT); pin_values(m.Pinf, MAT); }
    const double R = q[31];
    m.ts = p.ts + r.row0;
    m.t_prev = m.ts[0];                     // the series' own first time
    const int C = p.C;
    const long N = r.n;
    const double* V = p.V + r.row0 * (long)C;
    const double* rs = HET ? p.rs + r.row0 : nullptr;
    double* w = p.w + r.o_fm;
    double* out = p.out + (long)blockIdx.y * (C * C + 2);

    double h[D], P0[SYM];
    gp_prior<double, D>(m, h, P0);
    const long k0 = (long)threadIdx.x * r.Lc;
    const long k1 = min(N, k0 + r.Lc);

    // every branch on c0, C, N is uniform over the workgroup: the barriers inside the scans and sums are met by all lanes
    for (int c0 = 0; c0 < C; c0 += MC) {
        const int nc = min(MC, C - c0);
        // ---- reduce: the lane's aggregate over its chunk, then the exclusive prefix over the lanes
        FE agg;
        filt_identity_m(agg);
        if (k0 < k1) {
            double tprev = (k0 > 0) ? m.ts[k0 - 1] : m.t_prev;
            double tn = m.ts[k0], yn[MC], rn = 0.0;
            bool on = panel_gram_load<MC>(V, C, c0, nc, k0, yn);
            if constexpr (HET) rn = rs[k0];
            for (long k = k0; k < k1; ++k) {
                const double t = tn;
                const bool obs = on;
                const double Rk = (HET && obs) ? R + rn : R;
                double y[MC];
#pragma unroll
                for (int c = 0; c < MC; ++c) y[c] = yn[c];
                if (k + 1 < k1) {
                    tn = m.ts[k + 1];
                    on = panel_gram_load<MC>(V, C, c0, nc, k + 1, yn);
                    if constexpr (HET) rn = rs[k + 1];
                }
                if (k == 0) {
                    filt_first_m(agg, P0, y, obs, h, Rk);
                } else {
                    double F[MAT], Qf[MAT], Q[SYM];
                    lti_step<double, D>(m, t - tprev, F, Qf);
                    sym_from_full<double, D>(Qf, Q);
                    filt_extend_m(agg, F, Q, y, obs, h, Rk);
                }
                tprev = t;
            }
        }
        FE excl, total;
        block_scan_exclusive<FE, true>(agg, excl, total, lds);       // (ends on a barrier)

        // ---- the whitening Kalman pass from the lane's prefix
        MS s;
#pragma unroll
        for (int i = 0; i < SYM; ++i) s.P[i] = P0[i];
#pragma unroll
        for (int c = 0; c < MC; ++c)
#pragma unroll
            for (int i = 0; i < D; ++i) s.m[c][i] = 0.0;
        filt_apply_m(s, excl);
        LogLikM<MC> ll;
        if (k0 < k1) {
            double tprev = (k0 > 0) ? m.ts[k0 - 1] : m.t_prev;
            double tn = m.ts[k0], yn[MC], rn = 0.0;
            bool on = panel_gram_load<MC>(V, C, c0, nc, k0, yn);
            if constexpr (HET) rn = rs[k0];
            for (long k = k0; k < k1; ++k) {
                const double t = tn;
                const bool obs = on;
                const double Rk = (HET && obs) ? R + rn : R;
                double y[MC];
#pragma unroll
                for (int c = 0; c < MC; ++c) y[c] = yn[c];
                if (k + 1 < k1) {
                    tn = m.ts[k + 1];
                    on = panel_gram_load<MC>(V, C, c0, nc, k + 1, yn);
                    if constexpr (HET) rn = rs[k + 1];
                }
                double F[MAT], Qf[MAT], Q[SYM];
                lti_step<double, D>(m, t - tprev, F, Qf);
                sym_from_full<double, D>(Qf, Q);
                tprev = t;
                double mp[MC][D], Pp[SYM], FP[MAT], res[MC], S = 1.0;
#pragma unroll
                for (int c = 0; c < MC; ++c) res[c] = 0.0;
                kf_step_m<double, D, MC>(s, F, Q, y, obs, h, Rk, k == 0, ll, mp, Pp, FP, res, &S);
                const double is = recip(sqrt(S));
                double* pw = w + k * (long)C + c0;
#pragma unroll
                for (int c = 0; c < MC; ++c)
                    if (c < nc) pw[c] = obs ? res[c] * is : 0.0;
            }
        }
        if (c0 == 0) {
            const double ld = block_sum_double(std::log(ll.mant) + double(ll.expo) * 0.6931471805599453, lds_ll);
            const double cnt = block_sum_double(double(ll.count), lds_ll);
            if (threadIdx.x == 0) {
                out[C * C] = ld;
                out[C * C + 1] = cnt;           // (a sum of integers below 2^53: exact)
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- G = W^T W.  Lane t takes rows t, t + 256, .. in row order and keeps all kPanelGramTri products on or above the
    // diagonal (0.0 stands in for the columns beyond C); a wave's 64 sums fold in a fixed shuffle tree, the 4 waves' totals
    // in wave order by the lane that owns the entry
    double acc[kPanelGramTri];
#pragma unroll
    for (int e = 0; e < kPanelGramTri; ++e) acc[e] = 0.0;
    for (long k = threadIdx.x; k < N; k += kBlock) {
        double x[kPanelGramMax];
#pragma unroll
        for (int c = 0; c < kPanelGramMax; ++c) x[c] = c < C ? w[k * (long)C + c] : 0.0;
        int e = 0;
#pragma unroll
        for (int i = 0; i < kPanelGramMax; ++i)
#pragma unroll
            for (int j = i; j < kPanelGramMax; ++j) acc[e++] += x[i] * x[j];
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int e = 0; e < kPanelGramTri; ++e) {
        double t = acc[e];
#pragma unroll
        for (int sft = kWave / 2; sft > 0; sft >>= 1) t += __shfl_down(t, sft, kWave);
        if (lane == 0) red[wave * kPanelGramTri + e] = t;
    }
    __syncthreads();
    if (threadIdx.x < kPanelGramTri) {
        // entry e of the upper triangle, rows first: (i, j), i <= j
        int i = 0, e = (int)threadIdx.x;
        while (e >= kPanelGramMax - i) { e -= kPanelGramMax - i; ++i; }
        const int j = i + e;
        if (j < C) {
            double t = 0.0;
#pragma unroll
            for (int wv = 0; wv < kWaves; ++wv) t += red[wv * kPanelGramTri + (int)threadIdx.x];
            out[i * C + j] = t;
            out[j * C + i] = t;
        }
    }
}

// grid (tiles of the group's longest series, series of the group)
static __global__ __launch_bounds__(kBlock) void k_panel_residual(const long* __restrict__ offs, int C, const double* __restrict__ V,
                                                                  const double* __restrict__ betas, double* __restrict__ ys_out) {
    const long row0 = offs[blockIdx.y], row1 = offs[blockIdx.y + 1];
    const long k = row0 + (long)blockIdx.x * kBlock + threadIdx.x;
    if (k >= row1) return;
    const double* v = V + k * (long)C;
    const double* b = betas + (long)blockIdx.y * (C - 1);
    const double y = v[0];
    if (is_nan(y)) { ys_out[k] = y; return; }           // a missing row: the other columns are not read
    // products and sums rounded one by one, never contracted into fused multiply-adds: the bits are those of the same loop anywhere
    {
#pragma clang fp contract(off)
        double acc = 0.0;
        for (int j = 0; j + 1 < C; ++j) {
            const double prod = v[1 + j] * b[j];
            acc = acc + prod;
        }
        ys_out[k] = y - acc;
    }
}

}  // namespace pgps
