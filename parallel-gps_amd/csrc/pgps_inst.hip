// pgps_inst.hip -- one translation unit per compiled (dtype, state dimension): the kernels of
// pgps_kernels.hip.h / pgps_discretise.hip.h instantiated for PGPS_INST_T, PGPS_INST_D, and the
// launch functions the C ABI dispatches to.  Split this way because the fully unrolled algebra
// for d >= 5 takes minutes to compile; the Makefile builds the units in parallel.
//
// With -DPGPS_NARROW -DPGPS_BLOCK=128 the unit holds a second build of the array-path scan only, with 128-lane
// workgroups (half the lanes per workgroup = half the scan tree per step at the same number of workgroups: c2 86.7 ->
// 82.6 us, RBF order 6 fp32 0.66 -> 0.59 ms, 2^14 .. 2^16 steps 32 -> 26 us; the fused kernels prefer 256 lanes).  Its
// kernels and its launch function carry their own names so that both builds link into one library.
#ifdef PGPS_NARROW
#define k_filter_reduce k_filter_reduce_n
#define k_filter_apply k_filter_apply_n
#define k_filter_single k_filter_single_n
#define k_smoother_reduce k_smoother_reduce_n
#define k_smoother_apply k_smoother_apply_n
#define k_seg_filter_total k_seg_filter_total_n
#define k_seg_smoother_total k_seg_smoother_total_n
#define launch_scan launch_scan_narrow
#include "pgps_kernels.hip.h"
#else
#include "pgps_discretise.hip.h"
#include "pgps_fused.hip.h"
#include "pgps_gpadj.hip.h"
#include "pgps_gradlti.h"
#include "pgps_kernels.hip.h"
#endif

#include <type_traits>

#include "pgps_scratch.h"

#ifndef PGPS_INST_T
#error "compile with -DPGPS_INST_T=<float|double> -DPGPS_INST_D=<d>"
#endif

// single-pass filter where the grid fits the chip: automatic choice (A/B: profiles/r03_experiments.txt)
#ifndef PGPS_SINGLE_PASS_AUTO
#define PGPS_SINGLE_PASS_AUTO false
#endif

namespace pgps {

template <typename T, int D>
static int carve_workspace(pgps_ctx* ctx, ScanArgs<T>& a) {
    const size_t nl = (size_t)a.nlanes, nb = (size_t)a.nblocks;
    Carver c(256);
    const auto spine = c.part<T>(nb * Dim<D>::NFILT), lpre = c.part<T>(nl * Dim<D>::NFILT);
    const auto sspine = c.part<T>(nb * Dim<D>::NSMTH), lsuf = c.part<T>(nl * Dim<D>::NSMTH);
    const auto ll = c.part<double>(nb);
    c.part<char>(16);                                                   // reserved (the status word lives in the context)
    const auto seg = c.part<T>(2 * (size_t)(D + D * D) + 2 * D * D);
    const auto flags = c.part<int>(nb + 4 + 8 * 32);                    // (ticket +) the single-pass barrier's counter shards
    const auto incl = c.part<T>(nb * Dim<D>::NMP);
    Scratch s;
    if (int rc = commit(ctx, ctx->ws, c, &s)) return rc;
    a.spine = s(spine); a.lpre = s(lpre); a.sspine = s(sspine); a.lsuf = s(lsuf);
    a.llpart = s(ll);
    a.status = ctx->status_word;
    a.seg_ws = s(seg);
    a.ticket = s(flags);
    a.flags = a.ticket + 4;
    a.incl = s(incl);
#ifdef PGPS_STAMPS
    if (int rc = ensure(ctx, ctx->stamps, (size_t)3 * nb * 8 * sizeof(long long))) return rc;
    a.stamps = (long long*)ctx->stamps.p;
#endif
    return PGPS_OK;
}

#ifdef PGPS_NARROW
static_assert(kBlock == kBlockNarrow, "the narrow build is compiled with -DPGPS_BLOCK=128");
#endif

template <typename T, int D, int G, bool NT>
static int launch_scan_g(pgps_ctx* ctx, ScanArgs<T> a, Mode mode) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
#ifdef PGPS_NARROW
    geometry_narrow(ctx, a.N, &a.Lc, &a.nblocks, D);
#else
    geometry(ctx, a.N, &a.Lc, &a.nblocks, D);
#endif
    a.nlanes = (long)a.nblocks * kBlock;
    a.nt = NT ? 1 : 0;
    a.shortcut = (ctx->shortcut != 0 && (long)kBlock * a.Lc >= 2048) ? 1 : 0;
    int rc = carve_workspace<T, D>(ctx, a);
    if (rc) return rc;
    const dim3 grid(a.nblocks), block(kBlock);
    hipStream_t s = ctx->stream;
    // Whole series: nothing reads the stitching operands, but they must point at memory -- the compiler turns the small
    // `k + 1 < N ? Fs[k + 1] : halo_FQ` choices of d <= 2 into loads of both sides and a select (k_smoother_reduce<T, 2>
    // faulted on a null halo_FQ in the stand-alone smoother).
    a.carry_in = a.seg_ws;
    a.halo_FQ = a.seg_ws + (D + D * D);
    a.carry_back = a.seg_ws + (D + D * D) + 2 * D * D;
    // the Kalman pass with its inputs through an LDS-DMA ring (FilterApplyDma): 128-lane build, d = 2, fp64, 4-step
    // sub-tiles, 16 or 32 steps per lane.  A measured experiment, off unless asked for (pgps_set_dma(ctx, 1)): the ring
    // fills while the spine is folded, but issuing its 64 pieces costs the prologue what the loop then saves -- the
    // streaming loops are bound by the CU's memory path (10 - 14 B/clk), not by latency (profiles/r03_experiments.txt)
    bool dma = false;
#ifdef PGPS_NARROW
    if constexpr (sizeof(T) == 8 && D == 2 && G == 4)
        dma = ctx->dma > 0 && (a.Lc == 16 || a.Lc == 32);
#endif
    // whole-series filter + smoother: the smoothing totals in innovation form (pgps_math.h smth_extend_u) -- the fold of a step into
    // the lane's total is one matrix product and a rank-one update instead of three matrix products, and no L = P - E F P
    // (-DPGPS_DFORM=0: the reference's (E, g, L) elements everywhere, as the segment protocol keeps them)
#ifndef PGPS_DFORM
#define PGPS_DFORM 1
#endif
    const bool dform = PGPS_DFORM != 0 && mode == MODE_PKFS && !dma;
    a.dform = dform ? 1 : 0;
    auto launch_apply = [&](auto smooth_tag) {
        constexpr bool SMOOTH = decltype(smooth_tag)::value;
        if constexpr (SMOOTH) {
            if (dform) {
                timed_launch(ctx, PGPS_K_FILTER_APPLY, k_filter_apply<T, D, true, G, NT, false, true>, grid, block, 0, a);
                return;
            }
        }
#ifdef PGPS_NARROW
        if constexpr (sizeof(T) == 8 && D == 2 && G == 4) {
            if (dma) {
                timed_launch(ctx, PGPS_K_FILTER_APPLY, k_filter_apply<T, D, SMOOTH, G, NT, true>, grid, block, 0, a);
                return;
            }
        }
#endif
        timed_launch(ctx, PGPS_K_FILTER_APPLY, k_filter_apply<T, D, SMOOTH, G, NT>, grid, block, 0, a);
    };
    (void)dma;
    if (mode == MODE_SEG_REDUCE || mode == MODE_SEG_FILTER || mode == MODE_SEG_SMOOTHER) {
        // one segment of a series sharded over GPUs: carry_in / halo_FQ / carry_back live in seg_ws
        a.seg_first = (a.rank == 0);
        a.seg_last = (a.rank == a.nranks - 1);
        a.carry_in = a.seg_ws;
        a.halo_FQ = a.seg_ws + (D + D * D);
        a.carry_back = a.seg_ws + (D + D * D) + 2 * D * D;
        const int pad = seg_rec_s_pad(D);
        if (mode == MODE_SEG_REDUCE) {
            timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_filter_reduce<T, D, G>, grid, block, 0, a);
            hipLaunchKernelGGL((k_seg_filter_total<T, D>), dim3(1), block, 0, s, a);
        } else if (mode == MODE_SEG_FILTER) {
            // halo step of this segment = first step of the next rank, straight out of its record
            if (!a.seg_last)
                a.halo_FQ = a.gathered_f + (long)(a.rank + 1) * seg_rec_f_len(D) + Dim<D>::NFILT;
            launch_apply(std::true_type{});
            hipLaunchKernelGGL((k_seg_smoother_total<T, D>), dim3(1), block, 0, s, a, pad);
        } else timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_smoother_apply<T, D, G, NT>, grid, block, 0, a);
        HIPCHK(ctx, hipGetLastError());
        return PGPS_OK;
    }
    if constexpr (G == 4 && D <= 2) {
        // single-pass filter: whole series on this GPU, 16 steps per lane (they live in registers), one grid barrier
        // inside -- so every workgroup must be resident: one wave per SIMD (the chunk's registers allow no more), i.e.
        // workgroups x waves <= 4 x CUs.  Automatic where that holds (pgps_set_single_pass(ctx, 0) turns it off).
        const bool fits = (long)a.nblocks * kWaves <= 4L * ctx->n_cu && a.Lc == 16;
        const bool want = ctx->single_pass < 0 ? PGPS_SINGLE_PASS_AUTO : ctx->single_pass != 0;
        if (want && fits && (mode == MODE_PKF || mode == MODE_PKFS)) {
            a.win = 0;
            a.dform = 0;                    // (k_filter_single builds the reference's elements)
            HIPCHK(ctx, hipMemsetAsync(a.flags, 0, 8 * 32 * sizeof(int), s));        // the barrier's 8 counter shards
            if (mode == MODE_PKFS) {
                timed_launch(ctx, PGPS_K_FILTER_APPLY, k_filter_single<T, D, true, 16, NT>, grid, block, 0, a);
            } else {
                timed_launch(ctx, PGPS_K_FILTER_APPLY, k_filter_single<T, D, false, 16, NT>, grid, block, 0, a);
                if (a.ll)
                    timed_launch(ctx, PGPS_K_LL_FINALIZE, k_ll_finalize, dim3(1), block, 0, (const double*)a.llpart,
                                 a.nblocks, a.ll);
            }
            if (mode == MODE_PKFS) {
                ScanArgs<T> b = a;
                timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_smoother_apply<T, D, G, NT>, grid, block, 0, b);
            }
            HIPCHK(ctx, hipGetLastError());
            return PGPS_OK;
        }
    }
    if (mode == MODE_PKF || mode == MODE_PKFS) {
        timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_filter_reduce<T, D, G>, grid, block, 0, a);
        if (mode == MODE_PKFS) launch_apply(std::true_type{}); else {
            a.ll_in_apply = (a.ll != nullptr && a.status != nullptr) ? 1 : 0;
            launch_apply(std::false_type{});
            if (a.ll && !a.ll_in_apply) {
                timed_launch(ctx, PGPS_K_LL_FINALIZE, k_ll_finalize, dim3(1), block, 0, (const double*)a.llpart, a.nblocks,
                             a.ll);
            }
        }
    }
    if (mode == MODE_PKS) {
        ScanArgs<T> b = a;
        b.ll = nullptr;
        timed_launch(ctx, PGPS_K_SMOOTHER_REDUCE, k_smoother_reduce<T, D>, grid, block, 0, b);
    }
    if (mode == MODE_PKS || mode == MODE_PKFS) {
        ScanArgs<T> b = a;
        if (mode == MODE_PKS) b.ll = nullptr;
        timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_smoother_apply<T, D, G, NT>, grid, block, 0, b);
    }
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

// G = steps per lane per LDS-staged sub-tile (0 = direct global accesses); staging exists for
// d <= 3 only (StageCfg), G = 2 only in fp64 (a lane segment must be >= 16 bytes).
template <typename T, int D, int G>
static int launch_scan_nt(pgps_ctx* ctx, const ScanArgs<T>& a, Mode mode) {
    // streaming (non-temporal) output stores once one pass -- (7d^2+3d+1) scalars per step -- is well
    // beyond the 256 MiB Infinity Cache: -12 % on the smoother pass at N = 2^24, +5 % at 2^20
    const bool nt = (double)a.N * (7 * D * D + 3 * D + 1) * sizeof(T) > 512.0 * 1024 * 1024;
    if constexpr (G > 0) {
        if (nt) return launch_scan_g<T, D, G, true>(ctx, a, mode);
    }
    return launch_scan_g<T, D, G, false>(ctx, a, mode);
}

template <typename T, int D>
int launch_scan(pgps_ctx* ctx, ScanArgs<T> a, Mode mode) {
    if constexpr (D <= 2) {
        int g = ctx->stage_g < 0 ? 4 : ctx->stage_g;
        if (g == 4) return launch_scan_nt<T, D, 4>(ctx, a, mode);
        if constexpr (sizeof(T) == 8) {
            if (g == 2) return launch_scan_nt<T, D, 2>(ctx, a, mode);
        }
    } else if constexpr (D == 3) {
        // 144-byte lane segments: 2 steps of 72-byte fp64 records or 4 steps of 36-byte fp32 ones
        constexpr int g3 = (sizeof(T) == 8) ? 2 : 4;
        if (ctx->stage_g != 0) return launch_scan_nt<T, D, g3>(ctx, a, mode);
    } else if constexpr (D == 4 || (D == 6 && sizeof(T) == 4)) {
        // one step per sub-tile: 64- / 128-byte (d = 4) and 144-byte (d = 6 fp32) records
        if (ctx->stage_g != 0) return launch_scan_nt<T, D, 1>(ctx, a, mode);
    }
    return launch_scan_nt<T, D, 0>(ctx, a, mode);
}

#ifdef PGPS_NARROW
template int launch_scan<PGPS_INST_T, PGPS_INST_D>(pgps_ctx*, ScanArgs<PGPS_INST_T>, Mode);
#else
template <typename T, int D>
int launch_disc(pgps_ctx* ctx, long N, const T* F, const T* Pinf, const T* ts, T t0, T* Fs, T* Qs) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int block = 256;
    const long grid = (N + block - 1) / block;
    timed_launch(ctx, PGPS_K_DISCRETISE, k_discretise<T, D>, dim3((unsigned)grid), dim3(block), 0, N, F, Pinf, ts, t0, Fs,
                 Qs);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

// ---- fused-discretisation ("gp") launches: d <= 3 ------------------------------------------------------
// One workgroup walks the whole series: steps per lane, rounded up to whole 4-step sub-tiles (the other geometry rule the fused
// launchers share, batch_steps_per_lane, is the context's: pgps_ctx.hip)
static inline long one_workgroup_steps(long N) {
    const long v = (N + kBlock - 1) / kBlock;
    return (v + 3) / 4 * 4;
}

template <typename T, int D, bool NT>
static int launch_gp_nt(pgps_ctx* ctx, GpArgs<T> g, int want_filtered, int want_smoothed) {
    ScanArgs<T>& a = g.s;
    const dim3 grid(a.nblocks), block(kBlock);
    timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_gp_reduce<T, D>, grid, block, 0, g);
    if (want_smoothed) {
        timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gp_apply<T, D, true, NT>, grid, block, 0, g);
        if (g.qslot)
            timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gp_smooth<T, D, false, true>, grid, block, 0, g);
        else
            timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gp_smooth<T, D, NT>, grid, block, 0, g);
    } else {
        (void)want_filtered;
        a.ll_in_apply = (a.ll != nullptr && a.status != nullptr) ? 1 : 0;
        timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gp_apply<T, D, false, NT>, grid, block, 0, g);
        if (a.ll && !a.ll_in_apply)
            timed_launch(ctx, PGPS_K_LL_FINALIZE, k_ll_finalize, dim3(1), block, 0, (const double*)a.llpart, a.nblocks,
                         a.ll);
    }
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

template <typename T, int D>
int launch_gp(pgps_ctx* ctx, GpArgs<T> g, int want_filtered, int want_smoothed) {
    if constexpr (D <= 3) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        ScanArgs<T>& a = g.s;
        geometry(ctx, a.N, &a.Lc, &a.nblocks);
        // a short series: ONE workgroup, ONE launch (k_gp_one) instead of three launches of a few workgroups
        const bool one = ctx->one_launch != 0 && ctx->chunk <= 0 &&
                         a.N <= (ctx->one_launch > 0 ? (long)ctx->one_launch : (long)kOneLaunchAuto);
        if (one) {
            a.Lc = (int)one_workgroup_steps(a.N);
            a.nblocks = 1;
        }
        a.nlanes = (long)a.nblocks * kBlock;
        a.seg_first = 1;
        a.seg_last = 1;
        a.shortcut = (ctx->shortcut != 0 && (long)kBlock * a.Lc >= 2048) ? 1 : 0;
        int rc = carve_workspace<T, D>(ctx, a);
        if (rc) return rc;
        if (one) {
            const dim3 grid1(1), block1(kBlock);
            if (!want_smoothed) timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gp_one<T, D, 0>, grid1, block1, 0, g);
            else if (g.qslot) timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gp_one<T, D, 2>, grid1, block1, 0, g);
            else timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gp_one<T, D, 1>, grid1, block1, 0, g);
            HIPCHK(ctx, hipGetLastError());
            return PGPS_OK;
        }
        // bytes one pass moves: t, y in; (d^2 + d) filtered out and back in, (d^2 + d) smoothed out
        const double pass = (double)a.N * (2 + 3 * (D * D + D)) * sizeof(T);
        if (pass > 512.0 * 1024 * 1024) return launch_gp_nt<T, D, true>(ctx, g, want_filtered, want_smoothed);
        return launch_gp_nt<T, D, false>(ctx, g, want_filtered, want_smoothed);
    } else {
        (void)ctx; (void)g; (void)want_filtered; (void)want_smoothed;
        return PGPS_E_UNSUPPORTED_DIM;
    }
}

// ---- batched log-likelihood (B models over one series) ---------------------------------------------------
template <typename T, int D>
int launch_gp_batch(pgps_ctx* ctx, int B, GpBatchArgs<T> b) {
    if constexpr (D <= 3) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        const int lc = batch_steps_per_lane(ctx, B, b.N);
        b.Lc = lc;
        b.nblocks = (int)((b.N + (long)kBlock * lc - 1) / ((long)kBlock * lc));
        b.nlanes = (long)b.nblocks * kBlock;
        if (b.nblocks > 65535 * 16) return PGPS_E_INVALID;
        const size_t nb = (size_t)b.nblocks, nl = (size_t)b.nlanes, nB = (size_t)B;
        Carver c(256);
        const auto spine = c.part<T>(nB * nb * Dim<D>::NFILT), lpre = c.part<T>(nB * nl * Dim<D>::NFILT);
        const auto llpart = c.part<double>(nB * nb);
        Scratch s;
        if (int rc = commit(ctx, ctx->ws, c, &s)) return rc;
        b.spine = s(spine); b.lpre = s(lpre); b.llpart = s(llpart);
        const dim3 grid(b.nblocks, B), block(kBlock);
        timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_gpb_reduce<T, D>, grid, block, 0, b);
        timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpb_apply<T, D>, grid, block, 0, b);
        timed_launch(ctx, PGPS_K_LL_FINALIZE, k_gpb_finalize, dim3(B), block, 0, (const double*)b.llpart, b.nblocks, b.ll);
        HIPCHK(ctx, hipGetLastError());
        return PGPS_OK;
    } else {
        (void)ctx; (void)B; (void)b;
        return PGPS_E_UNSUPPORTED_DIM;
    }
}

// ---- batched predict_f (B models over one merged series of b.N steps) ------------------------------------
template <typename T, int D>
int launch_gp_predict_batch(pgps_ctx* ctx, int B, GpBatchArgs<T> b) {
    if constexpr (D <= 3) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        // form and geometry are fixed HERE, once per call, from (B, N): a model's result then depends neither on the group
        // it runs in nor on the other models
        // automatic = form 2: measured equal to form 1 within the spread up to B = 512 and faster at B = 1000.
        // Form 1 is honoured up to kBatchOneMax merged steps (one workgroup walks the whole series: 256 steps per lane there)
        const bool one = ctx->batch_form == 1 && b.N <= kBatchOneMax;
        int lc;
        if (one) {
            const long v = one_workgroup_steps(b.N);
            if (v > 0x7fffffffL) return PGPS_E_INVALID;
            lc = (int)v;
        } else {
            lc = batch_steps_per_lane(ctx, B, b.N);
        }
        b.Lc = lc;
        b.nblocks = one ? 1 : (int)((b.N + (long)kBlock * lc - 1) / ((long)kBlock * lc));
        b.nlanes = (long)b.nblocks * kBlock;
        if (b.nblocks > 65535) return PGPS_E_INVALID;    // (6.7e7 merged steps at 4 per lane: one model's scratch would be 10 GB)
        // The slices of a kind lie side by side (gp_batch_select strides them by the UNROUNDED record counts for the scan
        // records, as launch_gp_batch does, and by bs_fm / bs_fP for the moments: a model's slice of those is rounded to 256
        // bytes).  The layout of ONE model is what a model costs the budget
        const size_t nb = (size_t)b.nblocks, nl = (size_t)b.nlanes, n = (size_t)b.N;
        b.bs_fm = (long)(align_up(n * D * sizeof(T), 256) / sizeof(T));
        b.bs_fP = (long)(align_up(n * D * D * sizeof(T), 256) / sizeof(T));
        struct Parts { Part<T> spine, lpre, sspine, lsuf, fms, fPs; Part<double> ll; };
        auto lay = [&](Carver& c, size_t g) {
            Parts p;
            p.spine = c.part<T>(g * nb * Dim<D>::NFILT);  p.lpre = c.part<T>(g * nl * Dim<D>::NFILT);
            p.sspine = c.part<T>(g * nb * Dim<D>::NSMTH); p.lsuf = c.part<T>(g * nl * Dim<D>::NSMTH);
            p.ll = c.part<double>(g * nb);
            p.fms = c.part<T>(g * (size_t)b.bs_fm);       p.fPs = c.part<T>(g * (size_t)b.bs_fP);
            return p;
        };
        Carver c1(256), c(256);
        lay(c1, 1);
        const size_t group = batch_group(batch_budget_fused(ctx), 0, c1.bytes(), (size_t)B);
        const Parts p = lay(c, group);
        Scratch s;
        if (int rc = commit(ctx, ctx->ws, c, &s)) return rc;
        b.spine = s(p.spine); b.lpre = s(p.lpre); b.sspine = s(p.sspine); b.lsuf = s(p.lsuf);
        b.llpart = s(p.ll); b.fms = s(p.fms); b.fPs = s(p.fPs);
        const double* models = b.models;
        T* pmean = b.pmean;
        T* pvar = b.pvar;
        double* ll = b.ll;
        const dim3 block(kBlock);
        for (size_t g0 = 0; g0 < (size_t)B; g0 += group) {
            const unsigned G = (unsigned)((size_t)B - g0 < group ? (size_t)B - g0 : group);
            b.models = models + g0 * kGpModelStride;
            b.pmean = pmean + g0 * (size_t)b.K;
            b.pvar = pvar + g0 * (size_t)b.K;
            b.ll = ll + g0;
            if (one) {
                timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpb_one<T, D>, dim3(1, G), block, 0, b);
            } else {
                const dim3 grid(b.nblocks, G);
                timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_gpb_reduce<T, D>, grid, block, 0, b);
                timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpb_apply<T, D, true>, grid, block, 0, b);
                timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gpb_smooth<T, D>, grid, block, 0, b);
            }
            HIPCHK(ctx, hipGetLastError());
        }
        return PGPS_OK;
    } else {
        (void)ctx; (void)B; (void)b;
        return PGPS_E_UNSUPPORTED_DIM;
    }
}

// ---- fused path: log-likelihood and the model's adjoints (pgps_gpadj.hip.h), fp64 units of d <= 3 ---------------------
template <typename T, int D>
int launch_gp_adj(pgps_ctx* ctx, GpArgs<double> g, double* out) {
    if constexpr (D <= 3 && std::is_same<T, double>::value) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        ScanArgs<double>& a = g.s;
        geometry(ctx, a.N, &a.Lc, &a.nblocks);
        const bool one = ctx->one_launch != 0 && ctx->chunk <= 0 &&
                         a.N <= (ctx->one_launch > 0 ? (long)ctx->one_launch : (long)kOneLaunchAuto);
        if (one) {
            a.Lc = (int)one_workgroup_steps(a.N);
            a.nblocks = 1;
        }
        a.nlanes = (long)a.nblocks * kBlock;
        a.seg_first = 1;
        a.seg_last = 1;
        int rc = carve_workspace<double, D>(ctx, a);
        if (rc) return rc;
        constexpr int NX = D + Dim<D>::SYM, NST = gp_adj_nstat<D>();
        // the kept states and the workgroup partials, packed (the states are a whole number of 256-lane rows)
        Carver cg(sizeof(double));
        const auto xs = cg.part<double>((size_t)a.Lc * NX * (size_t)a.nlanes), gpart = cg.part<double>((size_t)a.nblocks * NST);
        Scratch sg;
        if ((rc = commit(ctx, ctx->gadj, cg, &sg))) return rc;
        GpAdjArgs ga{};
        ga.g = g;
        ga.xs = sg(xs);
        ga.gpart = sg(gpart);
        ga.out = out;
        const dim3 grid(a.nblocks), block(kBlock);
        if (one) {
            timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gp_gone<D>, dim3(1), block, 0, ga);
        } else {
            timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_gp_reduce<double, D>, grid, block, 0, g);
            timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gp_gfwd<D>, grid, block, 0, ga);
            timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gp_gback<D>, grid, block, 0, ga);
            timed_launch(ctx, PGPS_K_LL_FINALIZE, k_grad_lti_finalize, dim3(1 + NST), dim3(256), 0, (long)a.nblocks, (int)NST,
                         (const double*)a.llpart, (const double*)ga.gpart, out);
        }
        HIPCHK(ctx, hipGetLastError());
        return PGPS_OK;
    } else {
        (void)ctx; (void)g; (void)out;
        return PGPS_E_UNSUPPORTED_DIM;
    }
}
template int launch_gp_adj<PGPS_INST_T, PGPS_INST_D>(pgps_ctx*, GpArgs<double>, double*);

// ---- the same for B models over one series (pgps_gp_ll_grad_adj_batch_*): out (B, 1 + d^2 + 2 d + 1) on the device -----
template <typename T, int D>
int launch_gp_adj_batch(pgps_ctx* ctx, int B, GpBatchArgs<double> b, double* out) {
    if constexpr (D <= 3 && std::is_same<T, double>::value) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        // form and geometry are fixed HERE, once per call, from (B, N): a row then depends neither on its place in the table,
        // nor on the other rows, nor on the group it runs in.  One workgroup per model where launch_gp_adj takes ONE launch
        const bool one = ctx->one_launch != 0 && ctx->chunk <= 0 &&
                         b.N <= (ctx->one_launch > 0 ? (long)ctx->one_launch : (long)kOneLaunchAuto);
        int lc;
        if (one) lc = (int)one_workgroup_steps(b.N);
        else lc = batch_steps_per_lane(ctx, B, b.N);
        b.Lc = lc;
        b.nblocks = one ? 1 : (int)((b.N + (long)kBlock * lc - 1) / ((long)kBlock * lc));
        b.nlanes = (long)b.nblocks * kBlock;
        if (b.nblocks > 65535) return PGPS_E_INVALID;
        constexpr int NX = D + Dim<D>::SYM, NST = gp_adj_nstat<D>();
        // The scan records in ctx->ws, the kept states and the workgroup partials in ctx->gadj; the slices of a kind lie side by
        // side, strided by the unrounded record counts (gp_batch_select, gp_adj_batch_select) -- the kept states by a model's
        // count rounded to 256 bytes.  The two layouts of ONE model are what a model costs the budget
        const size_t nb = (size_t)b.nblocks, nl = (size_t)b.nlanes;
        const size_t bs_xs = align_up((size_t)lc * NX * nl * sizeof(double), 256) / sizeof(double);
        struct Parts { Part<double> spine, lpre, sspine, lsuf, ll, xs, gpart; };
        auto lay = [&](Carver& cw, Carver& cg, size_t g) {
            Parts p;
            p.spine = cw.part<double>(g * nb * Dim<D>::NFILT);  p.lpre = cw.part<double>(g * nl * Dim<D>::NFILT);
            p.sspine = cw.part<double>(g * nb * Dim<D>::NSMTH); p.lsuf = cw.part<double>(g * nl * Dim<D>::NSMTH);
            p.ll = cw.part<double>(g * nb);
            p.xs = cg.part<double>(g * bs_xs);                  p.gpart = cg.part<double>(g * nb * NST);
            return p;
        };
        Carver cw1(256), cg1(256), cw(256), cg(256);
        lay(cw1, cg1, 1);
        const size_t group = batch_group(batch_budget_fused(ctx), 0, cw1.bytes() + cg1.bytes(), (size_t)B);
        const Parts p = lay(cw, cg, group);
        Scratch s, sg;
        if (int rc = commit(ctx, ctx->ws, cw, &s)) return rc;
        if (int rc = commit(ctx, ctx->gadj, cg, &sg)) return rc;
        b.spine = s(p.spine); b.lpre = s(p.lpre); b.sspine = s(p.sspine); b.lsuf = s(p.lsuf); b.llpart = s(p.ll);
        GpAdjBatchArgs ab{};
        ab.xs = sg(p.xs);
        ab.bs_xs = (long)bs_xs;
        ab.gpart = sg(p.gpart);
        const double* models = b.models;
        const dim3 block(kBlock);
        for (size_t g0 = 0; g0 < (size_t)B; g0 += group) {
            const unsigned G = (unsigned)((size_t)B - g0 < group ? (size_t)B - g0 : group);
            b.models = models + g0 * kGpModelStride;
            ab.b = b;
            ab.out = out + g0 * (size_t)(1 + NST);
            if (one) {
                timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpb_gone<D>, dim3(1, G), block, 0, ab);
            } else {
                const dim3 grid(b.nblocks, G);
                timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_gpb_reduce<double, D>, grid, block, 0, b);
                timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpb_gfwd<D>, grid, block, 0, ab);
                timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gpb_gback<D>, grid, block, 0, ab);
                timed_launch(ctx, PGPS_K_LL_FINALIZE, k_grad_lti_finalize_batch, dim3(1 + NST, G), dim3(256), 0, (long)b.nblocks, (int)NST,
                             (const double*)b.llpart, (const double*)ab.gpart, ab.out);
            }
            HIPCHK(ctx, hipGetLastError());
        }
        return PGPS_OK;
    } else {
        (void)ctx; (void)B; (void)b; (void)out;
        return PGPS_E_UNSUPPORTED_DIM;
    }
}
template int launch_gp_adj_batch<PGPS_INST_T, PGPS_INST_D>(pgps_ctx*, int, GpBatchArgs<double>, double*);

template int launch_gp_batch<PGPS_INST_T, PGPS_INST_D>(pgps_ctx*, int, GpBatchArgs<PGPS_INST_T>);
template int launch_gp_predict_batch<PGPS_INST_T, PGPS_INST_D>(pgps_ctx*, int, GpBatchArgs<PGPS_INST_T>);
template int launch_gp<PGPS_INST_T, PGPS_INST_D>(pgps_ctx*, GpArgs<PGPS_INST_T>, int, int);
template int launch_scan<PGPS_INST_T, PGPS_INST_D>(pgps_ctx*, ScanArgs<PGPS_INST_T>, Mode);
template int launch_disc<PGPS_INST_T, PGPS_INST_D>(pgps_ctx*, long, const PGPS_INST_T*, const PGPS_INST_T*,
                                                   const PGPS_INST_T*, PGPS_INST_T, PGPS_INST_T*, PGPS_INST_T*);
#endif      // PGPS_NARROW

}  // namespace pgps
