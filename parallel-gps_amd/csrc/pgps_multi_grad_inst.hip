// pgps_multi_grad_inst.hip -- one translation unit per state dimension d = 1, 2, 3 (fp64): the multi-column adjoint kernels of
// pgps_multi_grad.hip.h (and k_gpm_reduce at their tile width) instantiated for PGPS_MULTI_D, and the launch function the
// C ABI dispatches to.
#include "pgps_multi_grad.hip.h"

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
    // geometry ONCE per call from (M, N), by the rule of launch_gp_multi: neither a column's log-likelihood nor the sums
    // depend on the round a group runs in
    int lc = ctx->chunk;
    if (lc <= 0) {
        lc = 16;
        while (lc > 4 && (long)groups_all * ((a.N + (long)kBlock * lc - 1) / ((long)kBlock * lc)) < 1024) lc /= 2;
        if (a.N < (long)kBlock * 4) lc = (int)((a.N + kBlock - 1) / kBlock);
        if (lc < 1) lc = 1;
    }
    a.Lc = lc;
    a.nblocks = (int)((a.N + (long)kBlock * lc - 1) / ((long)kBlock * lc));
    a.nlanes = (long)a.nblocks * kBlock;
    if (a.nblocks > 0x7fffff) return PGPS_E_INVALID;
    a.rows = nullptr;
    const size_t nb = (size_t)a.nblocks, nl = (size_t)a.nlanes;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    // scratch of ONE group, and what the groups of the whole call share
    const size_t g_spine = nb * FE::N * 8, g_lpre = nl * FE::N * 8, g_sspine = nb * SE::N * 8, g_lsuf = nl * SE::N * 8;
    const size_t g_xs = nl * (size_t)lc * NX * 8;
    const size_t per_group = g_spine + g_lpre + g_sspine + g_lsuf + g_xs;
    const size_t s_ll = up((size_t)groups_all * MC * nb * 8), s_gp = up((size_t)groups_all * nb * NST * 8);
    const size_t budget = ctx->batch_scratch ? ctx->batch_scratch : kBatchScratchDefault;
    size_t group = budget > s_ll + s_gp ? (budget - s_ll - s_gp) / per_group : 0;
    if (group < 1) group = 1;                           // (one group is the least a launch can hold)
    if (group > (size_t)groups_all) group = (size_t)groups_all;
    if (group > 65535) group = 65535;                   // grid.y
    int rc = ensure(ctx, ctx->ws, s_ll + s_gp + up(group * g_spine) + up(group * g_lpre) + up(group * g_sspine) +
                                      up(group * g_lsuf) + up(group * g_xs));
    if (rc) return rc;
    char* base = (char*)ctx->ws.p;
    size_t off = 0;
    GpMultiGradArgs ga{};
    a.llpart = (double*)(base + off); off += s_ll;
    ga.gpart = (double*)(base + off); off += s_gp;
    a.spine = (double*)(base + off);  off += up(group * g_spine);
    a.lpre = (double*)(base + off);   off += up(group * g_lpre);
    a.sspine = (double*)(base + off); off += up(group * g_sspine);
    a.lsuf = (double*)(base + off);   off += up(group * g_lsuf);
    ga.xs = (double*)(base + off);
    ga.gs_xs = (long)(g_xs / 8);
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
