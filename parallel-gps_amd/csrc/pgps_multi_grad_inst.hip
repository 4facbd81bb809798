// pgps_multi_grad_inst.hip -- one translation unit per state dimension d = 1, 2, 3 (fp64): the multi-column adjoint kernels of
// pgps_multi_grad.hip.h (and k_gpm_reduce at their tile width) instantiated for PGPS_MULTI_D, and the launch function the
// C ABI dispatches to.
#include "pgps_multi_grad.hip.h"
#include "pgps_scratch.h"

#ifndef PGPS_MULTI_D
#error "compile with -DPGPS_MULTI_D=<1|2|3>"
#endif

namespace pgps {

template <int D>
int launch_gp_multi_grad(pgps_ctx* ctx, GpMultiArgs a, double* out) {
    constexpr int MC = MultiGradTile<D>::MC, NST = gpm_nstat<D>(), NX = Dim<D>::SYM + MC * D;
    using FE = FiltElemM<double, D, MC>;
    using SE = SmthElemM<double, D, MC>;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int groups_all = (a.M + MC - 1) / MC;
    multi_geometry(ctx, a.N, groups_all, &a.Lc, &a.nblocks);
    a.nlanes = (long)a.nblocks * kBlock;
    if (a.nblocks > 0x7fffff) return PGPS_E_INVALID;
    a.rows = nullptr;
    const size_t nb = (size_t)a.nblocks, nl = (size_t)a.nlanes;
    // doubles of ONE group; what the groups of the whole call share comes first
    const size_t g_spine = nb * FE::N, g_lpre = nl * FE::N, g_sspine = nb * SE::N, g_lsuf = nl * SE::N;
    const size_t g_xs = nl * (size_t)a.Lc * NX;
    Carver c(256);
    const auto llpart = c.part<double>((size_t)groups_all * MC * nb), gpart = c.part<double>((size_t)groups_all * nb * NST);
    const size_t group = batch_group(batch_budget_fused(ctx), c.bytes(), (g_spine + g_lpre + g_sspine + g_lsuf + g_xs) * sizeof(double),
                                     (size_t)groups_all);
    const auto spine = c.part<double>(group * g_spine), lpre = c.part<double>(group * g_lpre);
    const auto sspine = c.part<double>(group * g_sspine), lsuf = c.part<double>(group * g_lsuf);
    const auto xs = c.part<double>(group * g_xs);
    Scratch s;
    if (int rc = commit(ctx, ctx->ws, c, &s)) return rc;
    GpMultiGradArgs ga{};
    a.llpart = s(llpart); ga.gpart = s(gpart);
    a.spine = s(spine); a.lpre = s(lpre); a.sspine = s(sspine); a.lsuf = s(lsuf);
    ga.xs = s(xs);
    ga.gs_xs = (long)g_xs;
    const dim3 block(kBlock);
    for (size_t g0 = 0; g0 < (size_t)groups_all; g0 += group) {
        const unsigned G = (unsigned)((size_t)groups_all - g0 < group ? (size_t)groups_all - g0 : group);
        a.c_base = (int)(g0 * MC);
        a.ldm = (int)(G * MC);
        ga.a = a;
        const dim3 grid(a.nblocks, G);
        timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_gpm_reduce<D, MC>, grid, block, 0, a);
        timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpm_gfwd<D, MC>, grid, block, 0, ga);
        timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gpm_gback<D, MC>, grid, block, 0, ga);
        HIPCHK(ctx, hipGetLastError());
    }
    timed_launch(ctx, PGPS_K_LL_FINALIZE, k_gpb_finalize, dim3(a.M), block, 0, (const double*)a.llpart, a.nblocks, out);
    timed_launch(ctx, PGPS_K_LL_FINALIZE, k_gpm_gfinal, dim3(NST), block, 0, (const double*)ga.gpart,
                 (long)groups_all * a.nblocks, NST, out + a.M);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

template int launch_gp_multi_grad<PGPS_MULTI_D>(pgps_ctx*, GpMultiArgs, double*);

}  // namespace pgps
