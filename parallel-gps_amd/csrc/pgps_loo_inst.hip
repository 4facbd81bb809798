// pgps_loo_inst.hip -- one translation unit per state dimension d = 1, 2, 3 (fp64): the fused kernels in their predictive-check
// flavours and the launch function the C ABI dispatches to (pgps_check_api.hip).
//
// Two laws of y_k per step of a fitted model, by-products of the filter and smoother passes over the N training steps (no
// merge, no query rows):  the one-step-ahead law  y_k | y_1..k-1 ~ N(mu_k, S_k)  is what the Kalman pass hands to its
// log-likelihood accumulator (gp_apply_body's OSA flag stores it);  the leave-one-out law  y_k | y_-k  follows from the smoothed
// law of f_k = H x_k by removing the factor N(y_k | f_k, R) (gp_smooth_body's LOO flag: projection at every step, the epilogue
// loo_step, a per-lane accumulator of the log densities).  Four launches: k_gp_reduce as it is, k_gpl_apply, k_gpl_smooth, and
// a one-workgroup finalize that sums the workgroups' partials of both scores in index order (repeatable bit for bit).  No
// one-workgroup form, no resident launch, no streaming stores, no per-observation variances.
#include "pgps_fused.hip.h"
#include "pgps_scratch.h"

#ifndef PGPS_LOO_D
#error "compile with -DPGPS_LOO_D=<1|2|3>"
#endif

namespace pgps {

struct GpLooArgs {
    GpArgs<double> g;
    GpLooOut<double> o;
};

template <int D>
__global__ __launch_bounds__(kBlock) void k_gpl_apply(const GpLooArgs l) {
    __shared__ GpLds<double, D> sh;
    gp_apply_body<double, D, true, false, false, true>(l.g, sh, nullptr, l.o);
}

template <int D>
__global__ __launch_bounds__(kBlock) void k_gpl_smooth(const GpLooArgs l) {
    __shared__ GpLds<double, D> sh;
    gp_smooth_body<double, D, false, false, true>(l.g, sh, l.o);
}

// sums[0] = sum of llpart, sums[1] = sum of lpd_part: one workgroup, lane-strided partial sums and a fixed tree
static __global__ __launch_bounds__(kBlock) void k_gpl_finalize(const double* llpart, const double* lpd_part, int nblocks,
                                                                double* sums) {
    __shared__ double lds_ll[kWaves];
    double v = 0.0, w = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kBlock) { v += llpart[b]; w += lpd_part[b]; }
    const double tv = block_sum_double(v, lds_ll);
    const double tw = block_sum_double(w, lds_ll);
    if (threadIdx.x == 0) { sums[0] = tv; sums[1] = tw; }
}

template <int D>
int launch_gp_loo(pgps_ctx* ctx, GpArgs<double> g, GpLooOut<double> o, double* sums) {
    ScanArgs<double>& a = g.s;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    geometry(ctx, a.N, &a.Lc, &a.nblocks);
    a.nlanes = (long)a.nblocks * kBlock;
    a.seg_first = 1;
    a.seg_last = 1;
    a.shortcut = (ctx->shortcut != 0 && (long)kBlock * a.Lc >= 2048) ? 1 : 0;      // (as launch_gp sets it)
    a.ll = nullptr;                             // (the finalize launch sums the partials, not the smoother's first workgroup)
    a.ll_in_apply = 0;
    const size_t nl = (size_t)a.nlanes, nb = (size_t)a.nblocks;
    Carver c(256);
    const auto spine = c.part<double>(nb * Dim<D>::NFILT), lpre = c.part<double>(nl * Dim<D>::NFILT);
    const auto sspine = c.part<double>(nb * Dim<D>::NSMTH), lsuf = c.part<double>(nl * Dim<D>::NSMTH);
    const auto ll = c.part<double>(nb), lpd = c.part<double>(nb);
    Scratch s;
    if (int rc = commit(ctx, ctx->ws, c, &s)) return rc;
    a.spine = s(spine); a.lpre = s(lpre); a.sspine = s(sspine); a.lsuf = s(lsuf);
    a.llpart = s(ll);
    a.status = ctx->status_word;
    o.lpd_part = s(lpd);
    const GpLooArgs l{g, o};
    const dim3 grid(a.nblocks), block(kBlock);
    timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_gp_reduce<double, D>, grid, block, 0, g);
    timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpl_apply<D>, grid, block, 0, l);
    timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gpl_smooth<D>, grid, block, 0, l);
    timed_launch(ctx, PGPS_K_LL_FINALIZE, k_gpl_finalize, dim3(1), block, 0, (const double*)a.llpart, (const double*)o.lpd_part,
                 a.nblocks, sums);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

template int launch_gp_loo<PGPS_LOO_D>(pgps_ctx*, GpArgs<double>, GpLooOut<double>, double*);

}  // namespace pgps
