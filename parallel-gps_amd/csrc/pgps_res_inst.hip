// pgps_res_inst.hip -- the resident filter + smoother launch (pgps_resident.hip.h) instantiated for one (dtype, d):
// array form (Fs, Qs given: pgps_pkfs_dev_*) and fused form (Matern model + time stamps: pgps_gp_dev_*).
#include "pgps_resident.hip.h"
#include "pgps_scratch.h"

#ifndef PGPS_RES_T
#error "compile with -DPGPS_RES_T=<float|double> -DPGPS_RES_D=<d>"
#endif

namespace pgps {

template <typename T, int D>
int launch_resident(pgps_ctx* ctx, ResArgs<T> ra, bool fused, bool smooth) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ScanArgs<T>& a = ra.s;
    // steps per lane: 16 (4096 per workgroup) -- or 8 where the whole series then still fits the chip: twice the workgroups
    // for series of up to 2048 steps per CU, which at 16 would leave half of the CUs idle (2^19 steps: 39 -> 30 us)
    const int max_blocks = ctx->n_cu < kResMaxBlocks ? ctx->n_cu : kResMaxBlocks;
    int lc = kResLc;
    if (ctx->resident > 0 && (ctx->chunk == 8 || ctx->chunk == 16)) lc = ctx->chunk;
    else if (a.N <= (long)kBlock * 8 * max_blocks) lc = 8;
    a.Lc = lc;
    a.nblocks = (int)((a.N + (long)kBlock * lc - 1) / ((long)kBlock * lc));
    // every workgroup must be resident, and the hand-off records and the general fold hold kResMaxBlocks workgroups
    if (a.nblocks < 1 || a.nblocks > max_blocks) return PGPS_E_INVALID;
    a.nlanes = (long)a.nblocks * kBlock;
    a.seg_first = 1;
    a.seg_last = 1;
    a.shortcut = ctx->shortcut != 0 ? 1 : 0;        // (a workgroup spans 2048 or 4096 steps; the test is on the data either way)
    // the workspace holds the log-likelihood partials alone: the totals travel as tagged granules in the context's own arrays
    // (which never move or grow: a granule of an earlier launch keeps its tag, wherever the workspace has gone since)
    const size_t nb = (size_t)a.nblocks;
    Carver c(256);
    const auto llpart = c.part<double>(nb);
    Scratch s;
    if (int rc = commit(ctx, ctx->ws, c, &s)) return rc;
    a.spine = nullptr;
    a.sspine = nullptr;
    a.llpart = s(llpart);
    a.status = ctx->status_word;
    const unsigned e = ctx->res_epoch++;
    ra.bar = ctx->status_word + kResBarWord + (e & 1u) * kResBarSet;
    ra.bar2 = ra.bar + kResBarSet / 2;
    ra.bar_next = ctx->status_word + kResBarWord + ((e + 1u) & 1u) * kResBarSet;
    ra.gran1 = ctx->res_gran;
    ra.gran2 = ctx->res_gran + (size_t)kResMaxBlocks * kResGranStride / sizeof(unsigned long long);
    ra.epoch = (int)(e % 0x7ffffffeu) + 1;           // compared for equality: a stale granule of any earlier launch never matches
    ra.stamps = nullptr;
    ra.wstamps = nullptr;
    ra.delay_tile = -1;
    ra.delay_phase = 0;
    ra.delay_ticks = 0;
    const bool skew = ctx->res_delay_tile >= 0;        // the start-skew hook (pgps_debug_resident_delay): diagnostics only
    if (ctx->resident == 2 || skew) {
        // (nblocks, 16) workgroup stamps, then (nblocks, 8) per-wave stamps (pgps_resident_wave_stamps)
        if (int rc = ensure(ctx, ctx->res_stamps, nb * (16 + 8) * sizeof(long long))) return rc;
        if (ctx->resident == 2) ra.stamps = (long long*)ctx->res_stamps.p;
        ctx->res_stamp_blocks = a.nblocks;
    }
    if (skew) {
        // every record a workgroup could read before it is published is NaN: a stale read cannot match by luck (the granules'
        // data words all ones, which is a NaN in either half of a double, under a tag of all ones, which is no epoch)
        HIPCHK(ctx, hipMemsetAsync(ctx->res_stamps.p, 0, nb * 16 * sizeof(long long), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(a.llpart, 0xFF, c.bytes(), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(ctx->res_gran, 0xFF, kResGranBytes, ctx->stream));
        ra.wstamps = (long long*)ctx->res_stamps.p;
        ra.delay_tile = ctx->res_delay_tile;
        ra.delay_phase = ctx->res_delay_phase;
        ra.delay_ticks = ctx->res_delay_ticks;
    }
    const dim3 grid(a.nblocks), block(kBlock);
    auto go = [&](auto lcv, auto fusedv, auto smoothv) {
        constexpr int L = decltype(lcv)::value;
        constexpr bool FU = decltype(fusedv)::value, SM = decltype(smoothv)::value;
        if (skew) timed_launch(ctx, PGPS_K_RESIDENT, k_pkfs_resident<T, D, L, FU, SM, true>, grid, block, 0, ra);
        else timed_launch(ctx, PGPS_K_RESIDENT, k_pkfs_resident<T, D, L, FU, SM, false>, grid, block, 0, ra);
    };
    auto pick = [&](auto lcv) {
        if (fused) { if (smooth) go(lcv, std::true_type{}, std::true_type{}); else go(lcv, std::true_type{}, std::false_type{}); }
        else { if (smooth) go(lcv, std::false_type{}, std::true_type{}); else go(lcv, std::false_type{}, std::false_type{}); }
    };
    if (lc == 8) pick(std::integral_constant<int, 8>{}); else pick(std::integral_constant<int, kResLc>{});
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

template int launch_resident<PGPS_RES_T, PGPS_RES_D>(pgps_ctx*, ResArgs<PGPS_RES_T>, bool, bool);

}  // namespace pgps
