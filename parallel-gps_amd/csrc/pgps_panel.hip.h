// pgps_panel.hip.h -- S independent series, each on its own clock and of its own length, in ONE launch.
//
// The third batching axis: B models over one series is gp_batch_select, M columns on one clock is pgps_multi.hip.h, and here
// blockIdx.y selects a SERIES.  Series of 10^2 .. 10^3 steps are bound by launch latency: one workgroup does all the work of a
// call and the other CUs idle.  A panel gives every series one workgroup of one launch -- the one-workgroup forms k_gp_one /
// k_gp_gone / k_gpb_one behind a view built per series from a descriptor table:
//
//   PanelDesc          one record per series, in device memory: where its rows lie in the concatenated ts / ys / rs, where its
//                      queries lie in tq / mean / var, where its merged slot lies, its steps per lane, its ragged scratch slices
//   gp_panel_select    the GpArgs<double> view of series blockIdx.y: N = its own length, nblocks = 1, nlanes = kBlock, every
//                      pointer pre-offset so the bodies index from 0.  What the bodies may touch behind a view is what they may
//                      touch in a single call: rows [0, N) of the series.  Row N is the NEIGHBOUR's first row (past the allocation
//                      for the last series), so every look-ahead of the bodies must be guarded by N or by the lane's own k1:
//                        gp_reduce_body   ts / ys / rs[k + 1]  only where k + 1 < k1 <= N
//                        gp_apply_body    ts[k + 1]            only where k + 1 < N;  ys / rs[k + 1] where k + 1 < k1
//                        gp_smooth_body   ts[k1]               only where k1 < N;     ts[k - 1] where k > 0
//                        gp_gfwd_body     ts / ys / rs[k + 1]  only where k + 1 < k1
//                        gp_gback_body    ts[k - 1]            only where k > 0;      ys / rs[k], xs of its own steps
//                        gp_apply_body    (OSA) the same reads; stores osa_mean / osa_var[k] of its own steps k0 <= k < k1
//                        gp_smooth_body   (LOO, LHET) ys / rs[k1 - 1] where k0 < k1;  ys / rs[k - 1] only where k > k0;
//                                         stores loo_mean / loo_var[k] of its own steps
//                      (read off the bodies as they stand; tests/test_gpu_panel.py gives every series its own seed, so a read of
//                      a neighbour's row moves a result)
//   k_gpp_one          reduce, Kalman pass and (predict) projecting smoother back to back, one workgroup per series
//   k_gpp_gone         reduce, adjoint forward, adjoint backward: out[s] = [ll | Abar | Ubar | Hbar | Rbar]
//   k_gpp_loo          reduce, Kalman pass (OSA), smoother (LOO): the predictive checks, sums[s] = {ll, loo_lpd}
//   k_panel_merge      (pgps_panel_inst.hip) merge_sorted_body per series
//
// These are also the first one-workgroup forms of the HET bodies (per-observation noise variances): HET is a
// template flag of both kernels, rs travels next to the view.
//
// A row's bits depend on that series alone: its steps per lane come from its own (merged) length and the pinned chunk, its
// scratch is its own, and no arithmetic crosses workgroups.
#pragma once

#include "pgps_gpadj.hip.h"

namespace pgps {

// (PanelDesc, PanelArgs, kPanelAlign and its two rules: pgps_internal.h)

// The view of one series.  `merged`: the series has queries and this is the predict call -- the view reads its merged slot;
// otherwise it reads the training rows where they lie (a series without queries needs no merge).
// What k_gp_one relies on, set the same way here: nblocks = 1 (no spine is folded, carry_shortcut_* is never reached:
// shortcut = 0), ll_in_apply = 0 (the ticket of ll_finish is ONE word of the context: workgroups of different series must not
// meet there; the kernel stores llpart[0] itself, or the smoother's prologue sums it), status = the context's word.
template <int D, bool HET>
__device__ __forceinline__ GpArgs<double> gp_panel_select(const PanelArgs& p, const PanelDesc& r, bool merged, const double** rs) {
    const double* q = p.models + (long)r.model * kGpModelStride;
    const long s = r.slot;
    GpArgs<double> g{};
    g.s.N = merged ? r.m : r.n;
    g.s.Lc = r.Lc; g.s.nblocks = 1; g.s.nlanes = kBlock;
    g.s.seg_first = 1; g.s.seg_last = 1;
    g.s.shortcut = 0; g.s.ll_in_apply = 0;
    g.s.status = p.status;
    g.s.ys = merged ? p.ys_m + r.m0 : p.ys + r.row0;
    g.s.R = q[31];
    g.s.spine = p.spine + s * Dim<D>::NFILT;
    g.s.lpre = p.lpre + s * kBlock * Dim<D>::NFILT;
    g.s.sspine = p.sspine + s * Dim<D>::NSMTH;
    g.s.lsuf = p.lsuf + s * kBlock * Dim<D>::NSMTH;
    g.s.llpart = p.llpart + s;
    g.s.ll = p.ll ? p.ll + blockIdx.y : nullptr;        // (the gradient call has none: its rows carry ll)
    g.m.lam = q[0];
#pragma unroll
    for (int i = 0; i < D * D; ++i) { g.m.N1[i] = q[1 + i]; g.m.N2[i] = q[10 + i]; g.m.Pinf[i] = q[19 + i]; }
#pragma unroll
    for (int i = 0; i < D; ++i) g.m.H[i] = q[28 + i];
    g.m.ts = merged ? p.ts_m + r.m0 : p.ts + r.row0;
    g.m.t_prev = g.m.ts[0];                 // the series' own first time
    if constexpr (HET) *rs = merged ? p.rs_m + r.m0 : p.rs + r.row0;
    else *rs = nullptr;
    if (merged) {
        g.s.fms = p.fms + r.o_fm;
        g.s.fPs = p.fPs + r.o_fP;
        g.qslot = p.qslot + r.m0;
        g.pmean = p.pmean;                  // (qslot holds global positions)
        g.pvar = p.pvar;
    }
    return g;
}

// What the kernels that run a whole search inside one workgroup (k_gpp_newton, pgps_panel_site.hip.h; k_gpp_fit,
// pgps_panel_fit.hip.h) put between the bodies and read the bodies' totals with.
// Stores that other lanes of the workgroup read later are drained before the barrier
__device__ __forceinline__ void wg_sync() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// A sum every lane already holds with the same bits, moved to scalar registers (the first active lane's copy): the compiler
// then KNOWS that the search's branches are uniform -- the loops around the barriers become scalar branches, and the swapped
// pointers stay in scalar registers instead of a vector register pair each
__device__ __forceinline__ double uniform_word(double x) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(x)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(x));
    return __hiloint2double(hi, lo);
}

// a word another lane of this workgroup stored before the last wg_sync: always a vector load
__device__ __forceinline__ double site_word(const double* p) {
    return uniform_word(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}

// One workgroup per series, grid (1, series of the launch): blockIdx.x stays the workgroup's place inside its series, 0.
// SMOOTH: 0 = the log-likelihoods, 2 = predict (a series without queries takes the log-likelihood's road: it still returns ll).
// Every branch below is uniform over the workgroup; there is no early return (every series of a launch has n >= 1).
template <int D, bool HET, int SMOOTH>
__global__ __launch_bounds__(kBlock) void k_gpp_one(const PanelArgs p) {
    static_assert(SMOOTH == 0 || SMOOTH == 2, "log-likelihood or predict");
    __shared__ GpLds<double, D> sh;
    const PanelDesc r = p.desc[blockIdx.y];
    const bool merged = SMOOTH == 2 && r.k > 0;
    const double* rs;
    const GpArgs<double> g = gp_panel_select<D, HET>(p, r, merged, &rs);
    gp_reduce_body<double, D, HET>(g, sh.lds, rs);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (SMOOTH == 2) {
        if (merged) {
            gp_apply_body<double, D, true, false, HET>(g, sh, rs);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            gp_smooth_body<double, D, false, true>(g, sh);
            return;
        }
    }
    gp_apply_body<double, D, false, false, HET>(g, sh, rs);
    if (threadIdx.x == 0) *g.s.ll = g.s.llpart[0];      // (this lane wrote the partial)
}

template <int D, bool HET>
__global__ __launch_bounds__(kBlock) void k_gpp_gone(const PanelArgs p) {
    constexpr int NST = gp_adj_nstat<D>();
    __shared__ GpLds<double, D> sh;
    const PanelDesc r = p.desc[blockIdx.y];
    const double* rs;
    GpAdjArgs ga{};
    ga.g = gp_panel_select<D, HET>(p, r, false, &rs);
    ga.xs = p.xs + r.o_xs;
    ga.gpart = p.gpart + (long)r.slot * NST;
    ga.out = p.out + (long)blockIdx.y * (1 + NST);
    gp_reduce_body<double, D, HET>(ga.g, sh.lds, rs);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    gp_gfwd_body<D, HET>(ga, sh, rs);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    gp_gback_body<D, HET>(ga, sh, rs);
    if (threadIdx.x == 0) {                     // (this lane wrote the partials)
        ga.out[0] = ga.g.s.llpart[0];
#pragma unroll
        for (int i = 0; i < NST; ++i) ga.out[1 + i] = ga.gpart[i];
    }
}

// The predictive checks of every series: reduce, the Kalman pass in its OSA flavour (it keeps the
// filtered moments: EVERY series has fms / fPs slices of its own n rows in this call) and the smoother in its LOO flavour, one
// workgroup per series.  The view is that of the training rows (never merged); the four per-row outputs are indexed from the
// series' row0 in arrays over the concatenated rows, any of them may be null.  nblocks = 1: the workgroup's llpart[0] and
// lpd_part[0] are the series' totals.
struct PanelLooArgs {
    PanelArgs p;                // desc, models, ts, ys, rs, the scan records, fms / fPs, llpart, status; ll is null
    GpLooOut<double> o;         // the call's arrays (all rows of the call); lpd_part: the group's scratch, one word per slot
    double* sums;               // (the group's series, 2): {ll, loo_lpd}
};

template <int D, bool HET>
__global__ __launch_bounds__(kBlock) void k_gpp_loo(const PanelLooArgs l) {
    __shared__ GpLds<double, D> sh;
    const PanelDesc r = l.p.desc[blockIdx.y];
    const double* rs;
    GpArgs<double> g = gp_panel_select<D, HET>(l.p, r, false, &rs);
    g.s.fms = l.p.fms + r.o_fm;
    g.s.fPs = l.p.fPs + r.o_fP;
    GpLooOut<double> o;
    o.osa_mean = l.o.osa_mean ? l.o.osa_mean + r.row0 : nullptr;
    o.osa_var = l.o.osa_var ? l.o.osa_var + r.row0 : nullptr;
    o.loo_mean = l.o.loo_mean ? l.o.loo_mean + r.row0 : nullptr;
    o.loo_var = l.o.loo_var ? l.o.loo_var + r.row0 : nullptr;
    o.lpd_part = l.o.lpd_part + r.slot;
    gp_reduce_body<double, D, HET>(g, sh.lds, rs);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    gp_apply_body<double, D, true, false, HET, true>(g, sh, rs, o);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    gp_smooth_body<double, D, false, false, true, false, HET>(g, sh, o, GpSiteOut<double>{}, rs);
    if (threadIdx.x == 0) {                     // (this lane wrote both partials)
        double* out = l.sums + 2 * (long)blockIdx.y;
        out[0] = g.s.llpart[0];
        out[1] = o.lpd_part[0];
    }
}

}  // namespace pgps
