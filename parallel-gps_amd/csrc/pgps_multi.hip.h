// pgps_multi.hip.h -- the fused Matern scan for M observation columns on one clock (pgps_gp_*_multi_f64).
//
// Y (N, M) is M independent GPs that share the kernel, the noise and the inputs (GPflow's num_latent_gps = M).  In the
// state-space form everything that is a covariance -- A, C, J of a filtering element, E, L of a smoothing element, the
// filtered and smoothed covariances, the gains, the innovation variances -- does not depend on y: it is the same for every
// column.  These kernels keep the structure of k_gp_reduce / k_gp_apply / k_gp_smooth<PROJ> (pgps_fused.hip.h: lane chunks
// of Lc steps, block_scan_exclusive over the lanes' aggregates, a spine across workgroups, a second walk over the chunk)
// on COLUMN-TILED elements (pgps_math.h: FiltElemM, SmthElemM, MeanCovM): one shared matrix part plus MC vector parts.  The
// matrix work of every extend / combine / apply, the discretisation (lti_step: one exp per step) and the reads of the times
// are done once per MC columns.
//
//   blockIdx.x   workgroup inside the series, as in the single-column kernels
//   blockIdx.y   column group: columns c0 = c_base + MC * blockIdx.y .. c0 + MC - 1.  A group recomputes the shared part
//                (the price of tiling); the last group loads 0.0 for its absent columns and skips their stores.
//
// ys is the (rows, M) row-major array the caller holds.  A step's row comes from `rows` (the merge of training and query
// times carries the source row of every merged step, NaN at a query step) or is the step itself (rows == nullptr).  A lane
// reads its group's MC adjacent values in 16-byte loads where M and c0 allow it.  A step is missing for all columns or for
// none: a group tests its own first column.  A NaN elsewhere in an observed row poisons that column alone.
//
// Log-likelihood: log S_k is shared, (y - mu)^2 / S_k per column; partials per (column, workgroup) are summed in a fixed order
// by k_gpb_finalize -- no floating-point atomics, results repeat bit for bit.  fp64, d <= 3.
#pragma once

#include "pgps_fused.hip.h"

namespace pgps {

// tile width per state dimension, from the compiler's resource report
template <int D> struct MultiTile { static constexpr int MC = 4; };
template <> struct MultiTile<1> { static constexpr int MC = 8; };
template <> struct MultiTile<3> { static constexpr int MC = 2; };

template <int D, int MC>
__device__ __forceinline__ void pack(const FiltElemM<double, D, MC>& e, double* v) {
    int o = 0;
#pragma unroll
    for (int i = 0; i < D * D; ++i) v[o++] = e.A[i];
#pragma unroll
    for (int i = 0; i < Dim<D>::SYM; ++i) v[o++] = e.C[i];
#pragma unroll
    for (int i = 0; i < Dim<D>::SYM; ++i) v[o++] = e.J[i];
#pragma unroll
    for (int c = 0; c < MC; ++c)
#pragma unroll
        for (int i = 0; i < D; ++i) { v[o++] = e.b[c][i]; v[o++] = e.eta[c][i]; }
}
template <int D, int MC>
__device__ __forceinline__ void unpack(const double* v, FiltElemM<double, D, MC>& e) {
    int o = 0;
#pragma unroll
    for (int i = 0; i < D * D; ++i) e.A[i] = v[o++];
#pragma unroll
    for (int i = 0; i < Dim<D>::SYM; ++i) e.C[i] = v[o++];
#pragma unroll
    for (int i = 0; i < Dim<D>::SYM; ++i) e.J[i] = v[o++];
#pragma unroll
    for (int c = 0; c < MC; ++c)
#pragma unroll
        for (int i = 0; i < D; ++i) { e.b[c][i] = v[o++]; e.eta[c][i] = v[o++]; }
}
template <int D, int MC>
__device__ __forceinline__ void pack(const SmthElemM<double, D, MC>& e, double* v) {
    int o = 0;
#pragma unroll
    for (int i = 0; i < D * D; ++i) v[o++] = e.E[i];
#pragma unroll
    for (int i = 0; i < Dim<D>::SYM; ++i) v[o++] = e.L[i];
#pragma unroll
    for (int c = 0; c < MC; ++c)
#pragma unroll
        for (int i = 0; i < D; ++i) v[o++] = e.g[c][i];
}
template <int D, int MC>
__device__ __forceinline__ void unpack(const double* v, SmthElemM<double, D, MC>& e) {
    int o = 0;
#pragma unroll
    for (int i = 0; i < D * D; ++i) e.E[i] = v[o++];
#pragma unroll
    for (int i = 0; i < Dim<D>::SYM; ++i) e.L[i] = v[o++];
#pragma unroll
    for (int c = 0; c < MC; ++c)
#pragma unroll
        for (int i = 0; i < D; ++i) e.g[c][i] = v[o++];
}

template <int D, int MC>
struct ElemTraits<FiltElemM<double, D, MC>> {
    using E = FiltElemM<double, D, MC>;
    static constexpr int N = E::N;
    using Scalar = double;
    __device__ static __forceinline__ void identity(E& e) { filt_identity_m(e); }
    __device__ static __forceinline__ void combine(const E& a, const E& b, E& o) { filt_combine_m(a, b, o); }
};
template <int D, int MC>
struct ElemTraits<SmthElemM<double, D, MC>> {
    using E = SmthElemM<double, D, MC>;
    static constexpr int N = E::N;
    using Scalar = double;
    __device__ static __forceinline__ void identity(E& e) { smth_identity_m(e); }
    __device__ static __forceinline__ void combine(const E& a, const E& b, E& o) { smth_combine_m(a, b, o); }
};

// this workgroup's column group
struct MultiGroup {
    int g;          // group inside the launch (slices of the scan scratch, of fms)
    int c0;         // its first column in ys / mean / ll
    int nc;         // its columns that exist (1 .. MC)
    bool vec;       // its MC values of a row are whole, 16-byte aligned pieces
};
template <int MC>
__device__ __forceinline__ MultiGroup multi_group(const GpMultiArgs& a) {
    MultiGroup q;
    q.g = (int)blockIdx.y;
    q.c0 = a.c_base + q.g * MC;
    q.nc = min(MC, a.M - q.c0);
    q.vec = (MC % 2 == 0) && q.nc == MC && (a.M % 2 == 0) && a.ys_aligned;
    return q;
}

// the MC observations of step k and whether the step is observed (the group's first column decides); 0.0 where there is no
// column or no row: what is loaded for them never reaches a store
template <int MC>
__device__ __forceinline__ bool multi_load_y(const GpMultiArgs& a, const MultiGroup& q, long k, double* y) {
    long row = k;
    bool have = true;
    if (a.rows != nullptr) {
        const double r = a.rows[k];
        have = !is_nan(r);
        row = have ? (long)r : 0;
    }
#pragma unroll
    for (int c = 0; c < MC; ++c) y[c] = 0.0;
    if (!have) return false;
    const double* p = a.ys + row * (long)a.M + q.c0;
    if (q.vec) {
        load_rec<double, MC>(p, y);
    } else {
#pragma unroll
        for (int c = 0; c < MC; ++c)
            if (c < q.nc) y[c] = p[c];
    }
    return !is_nan(y[0]);
}

// ---------------------------------------------------------------------------------------------
// reduce
// ---------------------------------------------------------------------------------------------
template <int D, int MC>
__global__ __launch_bounds__(kBlock) void k_gpm_reduce(const GpMultiArgs a) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM;
    using FE = FiltElemM<double, D, MC>;
    __shared__ double lds[kWaves * FE::N];
    const MultiGroup q = multi_group<MC>(a);
    // the model in vector registers: as kernel arguments its 28 doubles sit in scalar registers for the whole kernel, and at
    // d = 3 the scan's nested lane masks then no longer fit beside them (the compiler reserved spill slots in scratch)
    GpModel<double> m = a.m;
    if constexpr (D == 3) { pin_values(m.N1, MAT); pin_values(m.N2, MAT); pin_values(m.Pinf, MAT); }
    double h[D], P0[SYM];
    gp_prior<double, D>(m, h, P0);
    const long gt = (long)blockIdx.x * kBlock + threadIdx.x;
    const long k0 = gt * a.Lc;
    const long k1 = min(a.N, k0 + a.Lc);
    FE agg;
    filt_identity_m(agg);
    if (k0 < k1) {
        double tprev = (k0 > 0) ? m.ts[k0 - 1] : m.t_prev;
        double tn = m.ts[k0], yn[MC];
        bool on = multi_load_y<MC>(a, q, k0, yn);
        for (long k = k0; k < k1; ++k) {
            const double t = tn;
            const bool obs = on;
            double y[MC];
#pragma unroll
            for (int c = 0; c < MC; ++c) y[c] = yn[c];
            if (k + 1 < k1) { tn = m.ts[k + 1]; on = multi_load_y<MC>(a, q, k + 1, yn); }
            if (k == 0) {
                filt_first_m(agg, P0, y, obs, h, a.R);
            } else {
                double F[MAT], Qf[MAT], Q[SYM];
                lti_step<double, D>(m, t - tprev, F, Qf);
                sym_from_full<double, D>(Qf, Q);
                filt_extend_m(agg, F, Q, y, obs, h, a.R);
            }
            tprev = t;
        }
    }
    FE excl, total;
    block_scan_exclusive<FE, true>(agg, excl, total, lds);
    ws_store(a.lpre + (long)q.g * a.nlanes * FE::N, a.nlanes, gt, excl);
    if (threadIdx.x == 0) rec_store(a.spine + ((long)q.g * a.nblocks + blockIdx.x) * FE::N, total);
}

// ---------------------------------------------------------------------------------------------
// apply: the Kalman pass with the log-likelihood partials; SMOOTH: + filtered moments to scratch (the covariances once, from
// group 0 of the launch; the means per column) and the smoothing aggregates
// ---------------------------------------------------------------------------------------------
template <int D, int MC, bool SMOOTH>
__global__ __launch_bounds__(kBlock) void k_gpm_apply(const GpMultiArgs a) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM;
    using FE = FiltElemM<double, D, MC>;
    using SE = SmthElemM<double, D, MC>;
    using MS = MeanCovM<double, D, MC>;
    __shared__ double lds[kWaves * FE::N];      // (FE::N >= SE::N)
    __shared__ double lds_ll[kWaves];
    const MultiGroup q = multi_group<MC>(a);
    const double* spine = a.spine + (long)q.g * a.nblocks * FE::N;

    double h[D];
    MS s;
    gp_prior<double, D>(a.m, h, s.P);
#pragma unroll
    for (int c = 0; c < MC; ++c)
#pragma unroll
        for (int i = 0; i < D; ++i) s.m[c][i] = 0.0;

    const long gt = (long)blockIdx.x * kBlock + threadIdx.x;
    const long k0 = gt * a.Lc;
    const long k1 = min(a.N, k0 + a.Lc);

    FE left_part, lp;
    if (blockIdx.x > 0) fold_spine_partial<FE>(spine, 0, (int)blockIdx.x, left_part);
    ws_load(a.lpre + (long)q.g * a.nlanes * FE::N, a.nlanes, gt, lp);
    if (blockIdx.x > 0) {
        FE left;
        block_reduce_ordered(left_part, left, lds);
        filt_apply_m(s, left);
    }
    filt_apply_m(s, lp);

    LogLikM<MC> ll;
    SE sagg;
    smth_identity_m(sagg);
    if (k0 < k1) {
        double tprev = (k0 > 0) ? a.m.ts[k0 - 1] : a.m.t_prev;
        double tn = a.m.ts[k0], yn[MC];
        bool on = multi_load_y<MC>(a, q, k0, yn);
        for (long k = k0; k < k1; ++k) {
            const double t = tn;
            const bool obs = on;
            double y[MC];
#pragma unroll
            for (int c = 0; c < MC; ++c) y[c] = yn[c];
            if (k + 1 < a.N && (k + 1 < k1 || SMOOTH)) tn = a.m.ts[k + 1];
            if (k + 1 < k1) on = multi_load_y<MC>(a, q, k + 1, yn);
            double F[MAT], Qf[MAT], Q[SYM];
            lti_step<double, D>(a.m, t - tprev, F, Qf);
            sym_from_full<double, D>(Qf, Q);
            tprev = t;
            double mp[MC][D], Pp[SYM], FP[MAT];
            if constexpr (SMOOTH) {
                const MS prev = s;
                kf_step_m<double, D, MC>(s, F, Q, y, obs, h, a.R, k == 0, ll, mp, Pp, FP);
                if (k > k0) {                       // element of step k-1 from this step's predict
                    SE e, r;
                    smth_element_m<double, D, MC>(prev, mp, Pp, FP, e);
                    smth_combine_m(sagg, e, r);
                    sagg = r;
                }
                store_rec<double, MC * D>(a.fms + (k * (long)a.ldm + (long)q.g * MC) * D, &s.m[0][0]);
                if (q.g == 0) store_rec<double, SYM>(a.fPs + k * SYM, s.P);
            } else {
                kf_step_m<double, D, MC>(s, F, Q, y, obs, h, a.R, k == 0, ll, mp, Pp, FP);
            }
        }
        if constexpr (SMOOTH) {
            // the chunk's last step: its element comes from the predict of the step after the chunk
            SE e, r;
            if (k1 < a.N) {
                double F[MAT], Qf[MAT], Q[SYM], mp[MC][D], Pp[SYM], FP[MAT];
                lti_step<double, D>(a.m, tn - tprev, F, Qf);
                sym_from_full<double, D>(Qf, Q);
#pragma unroll
                for (int c = 0; c < MC; ++c) mat_vec<double, D>(F, s.m[c], mp[c]);
                predict_cov<double, D>(F, s.P, Q, FP, Pp);
                smth_element_m<double, D, MC>(s, mp, Pp, FP, e);
            } else {
                smth_last_m(s, e);
            }
            smth_combine_m(sagg, e, r);
            sagg = r;
        }
    }
#pragma unroll
    for (int c = 0; c < MC; ++c) {
        const double t = block_sum_double(ll.value(c), lds_ll);
        if (threadIdx.x == 0 && c < q.nc) a.llpart[(long)(q.c0 + c) * a.nblocks + blockIdx.x] = t;
    }
    if constexpr (SMOOTH) {
        SE excl, total;
        block_scan_exclusive<SE, false>(sagg, excl, total, lds);
        ws_store(a.lsuf + (long)q.g * a.nlanes * SE::N, a.nlanes, gt, excl);
        if (threadIdx.x == 0) rec_store(a.sspine + ((long)q.g * a.nblocks + blockIdx.x) * SE::N, total);
    }
}

// ---------------------------------------------------------------------------------------------
// smoother: backwards over the chunk, projected through H at the query steps only.  var[slot] is written once (by the group
// that holds column 0), mean[slot, c0 : c0 + nc] per group.
// ---------------------------------------------------------------------------------------------
template <int D, int MC>
__global__ __launch_bounds__(kBlock) void k_gpm_smooth(const GpMultiArgs a) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM;
    using SE = SmthElemM<double, D, MC>;
    using MS = MeanCovM<double, D, MC>;
    __shared__ double lds[kWaves * SE::N];
    const MultiGroup q = multi_group<MC>(a);
    const double* sspine = a.sspine + (long)q.g * a.nblocks * SE::N;

    const long gt = (long)blockIdx.x * kBlock + threadIdx.x;
    const long k0 = gt * a.Lc;
    const long k1 = min(a.N, k0 + a.Lc);
    const bool has_right = (int)blockIdx.x + 1 < a.nblocks;

    SE right_part, ls;
    if (has_right) fold_spine_partial<SE>(sspine, (int)blockIdx.x + 1, a.nblocks, right_part);
    ws_load(a.lsuf + (long)q.g * a.nlanes * SE::N, a.nlanes, gt, ls);
    MS s;
#pragma unroll
    for (int i = 0; i < SYM; ++i) s.P[i] = 0.0;
#pragma unroll
    for (int c = 0; c < MC; ++c)
#pragma unroll
        for (int i = 0; i < D; ++i) s.m[c][i] = 0.0;
    if (has_right) {
        SE right;
        block_reduce_ordered(right_part, right, lds);
        smth_apply_m(right, s);
    }
    smth_apply_m(ls, s);
    if (k0 >= k1) return;

    double h[D];
#pragma unroll
    for (int i = 0; i < D; ++i) h[i] = a.m.H[i];
    double tnext = (k1 < a.N) ? a.m.ts[k1] : 0.0;
    double tcur = a.m.ts[k1 - 1];
    for (long k = k1 - 1; k >= k0; --k) {
        double fm[MC][D], fP[SYM];
        load_rec<double, MC * D>(a.fms + (k * (long)a.ldm + (long)q.g * MC) * D, &fm[0][0]);
        load_rec<double, SYM>(a.fPs + k * SYM, fP);
        const double t = tcur;
        if (k > 0) tcur = a.m.ts[k - 1];
        if (k == a.N - 1) {
            // last element of the series: (0, m_N, P_N)
#pragma unroll
            for (int i = 0; i < SYM; ++i) s.P[i] = fP[i];
#pragma unroll
            for (int c = 0; c < MC; ++c)
#pragma unroll
                for (int i = 0; i < D; ++i) s.m[c][i] = fm[c][i];
        } else {
            double F[MAT], Qf[MAT], Q[SYM], mp[MC][D], Pp[SYM], FP[MAT];
            lti_step<double, D>(a.m, tnext - t, F, Qf);
            sym_from_full<double, D>(Qf, Q);
#pragma unroll
            for (int c = 0; c < MC; ++c) mat_vec<double, D>(F, fm[c], mp[c]);
            predict_cov<double, D>(F, fP, Q, FP, Pp);
            rts_step_m<double, D, MC>(fm, fP, mp, Pp, FP, s);
        }
        tnext = t;
        const int slot = a.qslot[k];
        if (slot >= 0) {
            double mu[MC];
#pragma unroll
            for (int c = 0; c < MC; ++c) {
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < D; ++r) v += h[r] * s.m[c][r];
                mu[c] = v;
            }
            double* pm = a.pmean + (long)slot * a.M + q.c0;
            if (q.vec && a.mean_aligned) {
                store_rec<double, MC>(pm, mu);
            } else {
#pragma unroll
                for (int c = 0; c < MC; ++c)
                    if (c < q.nc) pm[c] = mu[c];
            }
            if (q.c0 == 0) {
                double var = 0.0;
#pragma unroll
                for (int r = 0; r < D; ++r)
#pragma unroll
                    for (int c = 0; c < D; ++c) var += h[r] * h[c] * s.P[symi<D>(r < c ? r : c, r < c ? c : r)];
                a.pvar[slot] = var;
            }
        }
    }
}

}  // namespace pgps
