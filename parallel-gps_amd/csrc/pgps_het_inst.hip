// pgps_het_inst.hip -- one translation unit per state dimension d = 1, 2, 3 (fp64): the fused kernels in their
// per-observation-noise flavour and the launch functions the C ABI dispatches to (pgps_het_api.hip).
//
// The model is  y_k = H x_k + e_k,  e_k ~ N(0, R + s_k):  s_k given per step (`rs`, N doubles), R the shared jitter.  The bodies
// are those of pgps_fused.hip.h / pgps_gpadj.hip.h with their HET flag set: a lane loads rs[k + 1] next to its prefetch of
// ts[k + 1], ys[k + 1] and hands R + s_k to filt_first / filt_extend / kf_step / adj_step in place of R (het_noise: at a missing
// step the loaded value is replaced by 0 before the add, so it may be anything, NaN included).  The smoother never sees R: it is
// k_gp_smooth itself.  Three-launch forms only: reduce / Kalman pass / smoother with projection, and reduce / adjoint forward /
// adjoint backward (+ the finalize of the partials); no one-workgroup form here (the panel has them: pgps_panel.hip.h), no resident
// launch, no streaming stores.
#include "pgps_gpadj.hip.h"
#include "pgps_het.hip.h"
#include "pgps_scratch.h"

#ifndef PGPS_HET_D
#error "compile with -DPGPS_HET_D=<1|2|3>"
#endif

namespace pgps {

// (GpHetArgs, k_gph_reduce, k_gph_apply: pgps_het.hip.h)
struct GpHetAdjArgs {
    GpAdjArgs ga;
    const double* rs;
};

template <int D>
__global__ __launch_bounds__(kBlock) void k_gph_gfwd(const GpHetAdjArgs h) {
    __shared__ GpLds<double, D> sh;
    gp_gfwd_body<D, true>(h.ga, sh, h.rs);
}

template <int D>
__global__ __launch_bounds__(kBlock) void k_gph_gback(const GpHetAdjArgs h) {
    __shared__ GpLds<double, D> sh;
    gp_gback_body<D, true>(h.ga, sh, h.rs);
}

// geometry and the scan scratch of one call (what carve_workspace of pgps_inst.hip gives the scalar launches, less the parts
// only the array path uses)
template <int D>
static int het_setup(pgps_ctx* ctx, ScanArgs<double>& a, bool shortcut) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    geometry(ctx, a.N, &a.Lc, &a.nblocks);
    a.nlanes = (long)a.nblocks * kBlock;
    a.seg_first = 1;
    a.seg_last = 1;
    a.shortcut = (shortcut && ctx->shortcut != 0 && (long)kBlock * a.Lc >= 2048) ? 1 : 0;      // (as launch_gp sets it)
    const size_t nl = (size_t)a.nlanes, nb = (size_t)a.nblocks;
    Carver c(256);
    const auto spine = c.part<double>(nb * Dim<D>::NFILT), lpre = c.part<double>(nl * Dim<D>::NFILT);
    const auto sspine = c.part<double>(nb * Dim<D>::NSMTH), lsuf = c.part<double>(nl * Dim<D>::NSMTH);
    const auto ll = c.part<double>(nb);
    Scratch s;
    if (int rc = commit(ctx, ctx->ws, c, &s)) return rc;
    a.spine = s(spine); a.lpre = s(lpre); a.sspine = s(sspine); a.lsuf = s(lsuf);
    a.llpart = s(ll);
    a.status = ctx->status_word;
    return PGPS_OK;
}

// log-likelihood (g.qslot == nullptr: g.s.ll set) or predict_f over a merged series (g.qslot, g.pmean, g.pvar, g.s.fms, g.s.fPs
// set; rs merged as ys is)
template <int D>
int launch_gp_het(pgps_ctx* ctx, GpArgs<double> g, const double* rs) {
    ScanArgs<double>& a = g.s;
    if (int rc = het_setup<D>(ctx, a, true)) return rc;
    const bool predict = g.qslot != nullptr;
    a.ll_in_apply = (!predict && a.ll != nullptr && a.status != nullptr) ? 1 : 0;
    const GpHetArgs h{g, rs};
    const dim3 grid(a.nblocks), block(kBlock);
    timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_gph_reduce<D>, grid, block, 0, h);
    if (predict) {
        timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gph_apply<D, true>, grid, block, 0, h);
        timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gp_smooth<double, D, false, true>, grid, block, 0, g);
    } else {
        timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gph_apply<D, false>, grid, block, 0, h);
        if (a.ll && !a.ll_in_apply)
            timed_launch(ctx, PGPS_K_LL_FINALIZE, k_ll_finalize, dim3(1), block, 0, (const double*)a.llpart, a.nblocks, a.ll);
    }
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

// log-likelihood and the model's adjoints: out = [ll | Abar | Ubar | Hbar | Rbar] [device], Rbar = sum_k d ll / d (R + s_k)
template <int D>
int launch_gp_adj_het(pgps_ctx* ctx, GpArgs<double> g, const double* rs, double* out) {
    ScanArgs<double>& a = g.s;
    if (int rc = het_setup<D>(ctx, a, false)) return rc;
    constexpr int NX = D + Dim<D>::SYM, NST = gp_adj_nstat<D>();
    Carver cg(sizeof(double));
    const auto xs = cg.part<double>((size_t)a.Lc * NX * (size_t)a.nlanes), gpart = cg.part<double>((size_t)a.nblocks * NST);
    Scratch sg;
    if (int rc = commit(ctx, ctx->gadj, cg, &sg)) return rc;
    GpHetAdjArgs h{};
    h.ga.g = g;
    h.ga.xs = sg(xs);
    h.ga.gpart = sg(gpart);
    h.ga.out = out;
    h.rs = rs;
    const GpHetArgs hr{g, rs};
    const dim3 grid(a.nblocks), block(kBlock);
    timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_gph_reduce<D>, grid, block, 0, hr);
    timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gph_gfwd<D>, grid, block, 0, h);
    timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gph_gback<D>, grid, block, 0, h);
    timed_launch(ctx, PGPS_K_LL_FINALIZE, k_grad_lti_finalize, dim3(1 + NST), dim3(256), 0, (long)a.nblocks, (int)NST,
                 (const double*)a.llpart, (const double*)h.ga.gpart, out);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

template int launch_gp_het<PGPS_HET_D>(pgps_ctx*, GpArgs<double>, const double*);
template int launch_gp_adj_het<PGPS_HET_D>(pgps_ctx*, GpArgs<double>, const double*, double*);

}  // namespace pgps
