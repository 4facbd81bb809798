// pgps_multi_grad.hip.h -- log-likelihoods AND the model's adjoints for M observation columns on one clock
// (pgps_gp_ll_grad_multi_*): the adjoint pass of pgps_gpadj.hip.h on the column tiles of pgps_multi.hip.h.
//
// With a_c = d ll / d m per column and B = d ll / d P summed over the columns -- P is shared -- everything in the reverse
// sweep that is a matrix does not depend on y: F, Pp, u, s, K of a step, E = A^T and L of its scan element, B.  Per column
// there are only the vectors mp_c, r_c, a_c, g_c.  A tile of MC columns therefore costs one set of matrix work (and one
// discretisation, one read of the times) per step, as in the forward pass.  The statistics are the SUMS over the columns:
// what the host contracts with the model's derivatives (pssgp/_backend.py contract_grad_stats) is linear in them.
//
//   k_gpm_reduce  (pgps_multi.hip.h)  chunk totals of the tile's filtering elements, workgroup scan, spine
//   k_gpm_gfwd    every lane filters its chunk from the state entering it (log-likelihood partials per (column, workgroup) as
//                 k_gpm_apply writes them), keeps the state ENTERING every step lane-major -- P once per tile, m per column --
//                 and folds the steps' adjoint elements (pgps_math.h adj_element_m:  E = A^T shared,  g_c = v r_c / s,
//                 L = -nc v v^T / (2 s) shared, nc = the tile's columns that exist) into its chunk's total; workgroup suffix
//                 scan, spine.  With W = B - (1/2) sum_c a_c a_c^T:  a_c <- E a_c + g_c,  W <- E W E^T + L.
//   k_gpm_gback   the suffix applied to (0, 0) is (a_c, W) behind the lane's chunk; the lane walks its steps backwards from the
//                 kept states (pgps_math.h adj_reverse_m) and accumulates [Abar | Ubar | Hbar | Rbar]; workgroup sums in a fixed
//                 order -> gpart[(group of the CALL, workgroup, statistic)].
//   k_gpm_gfinal  one workgroup per statistic sums gpart over groups and workgroups in a fixed order; k_gpb_finalize the M
//                 log-likelihoods.  No floating-point atomics: results repeat bit for bit and do not depend on how the groups
//                 are split into rounds.
// blockIdx.y is the column group, as in pgps_multi.hip.h; the absent columns of the last group are loaded as 0.0 and keep
// r_c = a_c = 0.  rows == nullptr (training steps only: step k reads row k).  fp64, d <= 3.
#pragma once

#include "pgps_multi.hip.h"

namespace pgps {

// tile width per state dimension, from the compiler's resource report
template <int D> struct MultiGradTile { static constexpr int MC = MultiTile<D>::MC; };

template <int D>
constexpr int gpm_nstat() { return D * D + 2 * D + 1; }

struct GpMultiGradArgs {
    GpMultiArgs a;              // N, M, c_base, Lc, nblocks, nlanes, m, R, ys, spine, lpre, sspine, lsuf, llpart
    double* xs;                 // (groups, (sym + MC d) Lc, nlanes): the filtered state entering every step, lane-major
    long gs_xs;                 // doubles of one group's slice of xs
    double* gpart;              // (groups of the call, nblocks, d^2 + 2 d + 1)
};

// the step's F and Q (packed) from the time step
template <int D>
__device__ __forceinline__ void gpm_discretise(const GpModel<double>& m, double dt, double* F, double* Q /*sym*/) {
    double Qf[D * D];
    lti_step<double, D>(m, dt, F, Qf);
    sym_from_full<double, D>(Qf, Q);
}

// ---------------------------------------------------------------------------------------------
// forward: filter, log-likelihoods, kept states, adjoint elements
// ---------------------------------------------------------------------------------------------
template <int D, int MC>
__global__ __launch_bounds__(kBlock) void k_gpm_gfwd(const GpMultiGradArgs ga) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM, NX = SYM + MC * D;
    using FE = FiltElemM<double, D, MC>;
    using SE = SmthElemM<double, D, MC>;
    using MS = MeanCovM<double, D, MC>;
    __shared__ double lds[kWaves * FE::N];      // (FE::N >= SE::N)
    __shared__ double lds_ll[kWaves];
    const GpMultiArgs& a = ga.a;
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

    {
        FE left_part, lp;
        if (blockIdx.x > 0) fold_spine_partial<FE>(spine, 0, (int)blockIdx.x, left_part);
        ws_load(a.lpre + (long)q.g * a.nlanes * FE::N, a.nlanes, gt, lp);
        if (blockIdx.x > 0) {
            FE left;
            block_reduce_ordered(left_part, left, lds);
            filt_apply_m(s, left);
        }
        filt_apply_m(s, lp);
    }

    LogLikM<MC> ll;
    SE agg;
    smth_identity_m(agg);
    if (k0 < k1) {
        double* xs = ga.xs + (long)q.g * ga.gs_xs + gt;
        double tprev = (k0 > 0) ? a.m.ts[k0 - 1] : a.m.t_prev;
        double tn = a.m.ts[k0], yn[MC];
        bool on = multi_load_y<MC>(a, q, k0, yn);
        for (long k = k0; k < k1; ++k) {
            const double t = tn;
            const bool obs = on;
            double y[MC];
#pragma unroll
            for (int c = 0; c < MC; ++c) y[c] = yn[c];
            if (k + 1 < k1) { tn = a.m.ts[k + 1]; on = multi_load_y<MC>(a, q, k + 1, yn); }
            // the state entering the step: what the reverse pass starts the step from
            {
                double* x = xs + (long)(k - k0) * NX * a.nlanes;
#pragma unroll
                for (int i = 0; i < SYM; ++i) x[(long)i * a.nlanes] = s.P[i];
#pragma unroll
                for (int c = 0; c < MC; ++c)
#pragma unroll
                    for (int i = 0; i < D; ++i) x[(long)(SYM + c * D + i) * a.nlanes] = s.m[c][i];
            }
            double F[MAT], Q[SYM];
            gpm_discretise<D>(a.m, t - tprev, F, Q);
            tprev = t;
            AdjStepM<double, D, MC> st;
            adj_step_m<double, D, MC>(F, Q, s, y, obs, h, a.R, st);
            if (obs) ll.add(st.r, st.S);
            adj_filtered_m(st, s);
            // adjoint element of the step, folded into the chunk's total on its right (time order)
            SE e, r;
            adj_element_m(st, h, q.nc, e);
            smth_combine_m(agg, e, r);
            agg = r;
        }
    }
#pragma unroll
    for (int c = 0; c < MC; ++c) {
        const double t = block_sum_double(ll.value(c), lds_ll);
        if (threadIdx.x == 0 && c < q.nc) a.llpart[(long)(q.c0 + c) * a.nblocks + blockIdx.x] = t;
    }
    SE excl, total;
    block_scan_exclusive<SE, false>(agg, excl, total, lds);
    ws_store(a.lsuf + (long)q.g * a.nlanes * SE::N, a.nlanes, gt, excl);
    if (threadIdx.x == 0) rec_store(a.sspine + ((long)q.g * a.nblocks + blockIdx.x) * SE::N, total);
}

// ---------------------------------------------------------------------------------------------
// backward: the reverse sweep
// ---------------------------------------------------------------------------------------------
template <int D, int MC>
__global__ __launch_bounds__(kBlock) void k_gpm_gback(const GpMultiGradArgs ga) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM, NX = SYM + MC * D, NST = gpm_nstat<D>();
    using SE = SmthElemM<double, D, MC>;
    using MS = MeanCovM<double, D, MC>;
    __shared__ double lds[kWaves * SE::N];
    __shared__ double lds_ll[kWaves];
    const GpMultiArgs& a = ga.a;
    const MultiGroup q = multi_group<MC>(a);
    const double* sspine = a.sspine + (long)q.g * a.nblocks * SE::N;

    double h[D], Pinf[SYM];
    gp_prior<double, D>(a.m, h, Pinf);
    const long gt = (long)blockIdx.x * kBlock + threadIdx.x;
    const long k0 = gt * a.Lc;
    const long k1 = min(a.N, k0 + a.Lc);
    const bool has_right = (int)blockIdx.x + 1 < a.nblocks;

    double av[MC][D], B[SYM];
    {
        SE right_part, ls;
        if (has_right) fold_spine_partial<SE>(sspine, (int)blockIdx.x + 1, a.nblocks, right_part);
        ws_load(a.lsuf + (long)q.g * a.nlanes * SE::N, a.nlanes, gt, ls);
        MS z;                   // (a_c, W) behind the chunk
#pragma unroll
        for (int i = 0; i < SYM; ++i) z.P[i] = 0.0;
#pragma unroll
        for (int c = 0; c < MC; ++c)
#pragma unroll
            for (int i = 0; i < D; ++i) z.m[c][i] = 0.0;
        if (has_right) {
            SE right;
            block_reduce_ordered(right_part, right, lds);
            smth_apply_m(right, z);
        }
        smth_apply_m(ls, z);
#pragma unroll
        for (int c = 0; c < MC; ++c)
#pragma unroll
            for (int i = 0; i < D; ++i) av[c][i] = z.m[c][i];
        adj_cov_from_scan_m(z, B);
    }

    double st_[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) st_[i] = 0.0;

    if (k0 < k1) {
        const double* xs = ga.xs + (long)q.g * ga.gs_xs + gt;
        double tcur = a.m.ts[k1 - 1];
        for (long k = k1 - 1; k >= k0; --k) {
            const double t = tcur;
            const double tp = (k > 0) ? a.m.ts[k - 1] : a.m.t_prev;
            tcur = tp;
            double y[MC];
            const bool obs = multi_load_y<MC>(a, q, k, y);
            MS s;
            {
                const double* x = xs + (long)(k - k0) * NX * a.nlanes;
#pragma unroll
                for (int i = 0; i < SYM; ++i) s.P[i] = x[(long)i * a.nlanes];
#pragma unroll
                for (int c = 0; c < MC; ++c)
#pragma unroll
                    for (int i = 0; i < D; ++i) s.m[c][i] = x[(long)(SYM + c * D + i) * a.nlanes];
            }
            const double dt = t - tp;
            double F[MAT], Q[SYM];
            gpm_discretise<D>(a.m, dt, F, Q);
            AdjStepM<double, D, MC> st;
            adj_step_m<double, D, MC>(F, Q, s, y, obs, h, a.R, st);
            adj_reverse_m<double, D, MC>(st, dt, h, Pinf, q.nc, av, B, st_);
        }
    }
    const long gg = (long)(a.c_base / MC) + q.g;        // the group's place in the call
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        const double t = block_sum_double(st_[i], lds_ll);
        if (threadIdx.x == 0) ga.gpart[(gg * a.nblocks + blockIdx.x) * NST + i] = t;
    }
}

// one workgroup per statistic: out[blockIdx.x] = sum over the `count` (group, workgroup) partials, in a fixed order
static __global__ __launch_bounds__(kBlock) void k_gpm_gfinal(const double* gpart, long count, int nst, double* out) {
    __shared__ double lds_ll[kWaves];
    double v = 0.0;
    for (long i = threadIdx.x; i < count; i += kBlock) v += gpart[i * nst + blockIdx.x];
    const double t = block_sum_double(v, lds_ll);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

}  // namespace pgps
