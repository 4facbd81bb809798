// pgps_multi_inst.hip -- one translation unit per state dimension d = 1, 2, 3 (fp64): the multi-column kernels of
// pgps_multi.hip.h instantiated for PGPS_MULTI_D at its tile width, and the launch function the C ABI dispatches to.
#include "pgps_multi.hip.h"

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
    // geometry, ONCE per call from (M, N) -- a column's result does not depend on the round it runs in: pgps_set_chunk's
    // value, else 16 steps per lane while the groups keep the chip covered (>= 1024 workgroups), halved towards 4 when
    // groups x N is small; a series shorter than four steps per lane of one workgroup takes one workgroup
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
    const size_t nb = (size_t)a.nblocks, nl = (size_t)a.nlanes, n = (size_t)a.N;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    // scratch of ONE group, and what the groups share
    const size_t g_spine = nb * FE::N * 8, g_lpre = nl * FE::N * 8;
    const size_t g_sspine = predict ? nb * SE::N * 8 : 0, g_lsuf = predict ? nl * SE::N * 8 : 0;
    const size_t g_fm = predict ? n * MC * D * 8 : 0;
    const size_t per_group = g_spine + g_lpre + g_sspine + g_lsuf + g_fm;
    const size_t s_ll = up((size_t)groups_all * MC * nb * 8), s_fP = predict ? up(n * Dim<D>::SYM * 8) : 0;
    const size_t budget = ctx->batch_scratch ? ctx->batch_scratch : kBatchScratchDefault;
    size_t group = budget > s_ll + s_fP ? (budget - s_ll - s_fP) / per_group : 0;
    if (group < 1) group = 1;                           // (one group is the least a launch can hold)
    if (group > (size_t)groups_all) group = (size_t)groups_all;
    if (group > 65535) group = 65535;                   // grid.y
    int rc = ensure(ctx, ctx->ws, s_ll + s_fP + up(group * g_spine) + up(group * g_lpre) + up(group * g_sspine) +
                                      up(group * g_lsuf) + up(group * g_fm));
    if (rc) return rc;
    char* base = (char*)ctx->ws.p;
    size_t off = 0;
    a.llpart = (double*)(base + off); off += s_ll;
    a.fPs = (double*)(base + off);    off += s_fP;
    a.spine = (double*)(base + off);  off += up(group * g_spine);
    a.lpre = (double*)(base + off);   off += up(group * g_lpre);
    a.sspine = (double*)(base + off); off += up(group * g_sspine);
    a.lsuf = (double*)(base + off);   off += up(group * g_lsuf);
    a.fms = (double*)(base + off);
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
