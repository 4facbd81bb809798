// pgps_multi_inst.hip -- one translation unit per state dimension d = 1, 2, 3 (fp64): the multi-column kernels of
// pgps_multi.hip.h instantiated for PGPS_MULTI_D at its tile width, and the launch function the C ABI dispatches to.
#include "pgps_multi.hip.h"
#include "pgps_scratch.h"

#ifndef PGPS_MULTI_D
#error "compile with -DPGPS_MULTI_D=<1|2|3>"
#endif

namespace pgps {

template <int D>
int launch_gp_multi(pgps_ctx* ctx, GpMultiArgs a, int predict, double* ll) {
    constexpr int MC = MultiTile<D>::MC;
    using FE = FiltElemM<double, D, MC>;
    using SE = SmthElemM<double, D, MC>;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int groups_all = (a.M + MC - 1) / MC;
    multi_geometry(ctx, a.N, groups_all, &a.Lc, &a.nblocks);
    a.nlanes = (long)a.nblocks * kBlock;
    if (a.nblocks > 0x7fffff) return PGPS_E_INVALID;
    const size_t nb = (size_t)a.nblocks, nl = (size_t)a.nlanes, n = (size_t)a.N;
    // doubles of ONE group (the smoother's and the kept means in a predict call only); what the groups share comes first
    const size_t g_spine = nb * FE::N, g_lpre = nl * FE::N, g_sspine = predict ? nb * SE::N : 0, g_lsuf = predict ? nl * SE::N : 0;
    const size_t g_fm = predict ? n * MC * D : 0;
    Carver c(256);
    const auto llpart = c.part<double>((size_t)groups_all * MC * nb), fPs = c.part<double>(predict ? n * Dim<D>::SYM : 0);
    const size_t group = batch_group(batch_budget_fused(ctx), c.bytes(), (g_spine + g_lpre + g_sspine + g_lsuf + g_fm) * sizeof(double),
                                     (size_t)groups_all);
    const auto spine = c.part<double>(group * g_spine), lpre = c.part<double>(group * g_lpre);
    const auto sspine = c.part<double>(group * g_sspine), lsuf = c.part<double>(group * g_lsuf);
    const auto fms = c.part<double>(group * g_fm);
    Scratch s;
    if (int rc = commit(ctx, ctx->ws, c, &s)) return rc;
    a.llpart = s(llpart); a.fPs = s(fPs); a.fms = s(fms);
    a.spine = s(spine); a.lpre = s(lpre); a.sspine = s(sspine); a.lsuf = s(lsuf);
    const dim3 block(kBlock);
    for (size_t g0 = 0; g0 < (size_t)groups_all; g0 += group) {
        const unsigned G = (unsigned)((size_t)groups_all - g0 < group ? (size_t)groups_all - g0 : group);
        a.c_base = (int)(g0 * MC);
        a.ldm = (int)(G * MC);
        const dim3 grid(a.nblocks, G);
        timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_gpm_reduce<D, MC>, grid, block, 0, a);
        if (predict) {
            timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpm_apply<D, MC, true>, grid, block, 0, a);
            timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gpm_smooth<D, MC>, grid, block, 0, a);
        } else {
            timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpm_apply<D, MC, false>, grid, block, 0, a);
        }
        HIPCHK(ctx, hipGetLastError());
    }
    if (ll) {
        timed_launch(ctx, PGPS_K_LL_FINALIZE, k_gpb_finalize, dim3(a.M), block, 0, (const double*)a.llpart, a.nblocks, ll);
        HIPCHK(ctx, hipGetLastError());
    }
    return PGPS_OK;
}

template int launch_gp_multi<PGPS_MULTI_D>(pgps_ctx*, GpMultiArgs, int, double*);

}  // namespace pgps
