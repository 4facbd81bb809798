// pgps_ctx.hip -- the context of libpgps.so (include/pgps.h): creation, settings, status, device memory, per-kernel
// profiling, launch geometry, and the copy of results back to pageable host arrays.  HIP runtime only.
#include <cstdio>
#include <new>

#include "pgps_host.h"
#include "pgps_scratch.h"

using namespace pgps;

namespace pgps {
int ensure(pgps_ctx* ctx, DevBuf& b, size_t bytes) {
    if (&b == &ctx->ws) ++ctx->ws_epoch;            // somebody is about to lay the scratch out (again)
    if (bytes <= b.cap) return PGPS_OK;
    if (b.p) HIPCHK(ctx, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        ctx->hip_err = std::string("hipMalloc: ") + hipGetErrorString(e);
        (void)hipGetLastError();                    // reported here: the next call's launch check must not find it
        b.p = nullptr;
        return PGPS_E_NOMEM;
    }
    b.cap = want;
    return PGPS_OK;
}
}  // namespace pgps

extern "C" int pgps_version(void) { return 100; }

extern "C" const char* pgps_strerror(int code) {
    switch (code) {
        case PGPS_OK: return "ok";
        case PGPS_E_INVALID: return "invalid argument";
        case PGPS_E_UNSUPPORTED_DIM: return "state dimension not supported by the compiled kernels";
        case PGPS_E_HIP: return "HIP runtime error";
        case PGPS_E_NOMEM: return "out of memory";
        case PGPS_E_NUMERIC: return "non-finite result";
        case PGPS_E_NO_DEVICE: return "no HIP device";
        case PGPS_E_COMM: return "RCCL communicator error (pgps_last_hip_error)";
        default: return "unknown error";
    }
}

extern "C" int pgps_device_count(int* n) {
    if (!n) return PGPS_E_INVALID;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *n = c;
    return PGPS_OK;
}

extern "C" int pgps_create(int device, pgps_ctx** out) {
    if (!out) return PGPS_E_INVALID;
    *out = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c <= 0) return PGPS_E_NO_DEVICE;
    if (device < 0 || device >= c) return PGPS_E_INVALID;
    pgps_ctx* ctx = new (std::nothrow) pgps_ctx();
    if (!ctx) return PGPS_E_NOMEM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return PGPS_E_HIP;
    }
    ctx->stream = ctx->own_stream;
    if (hipDeviceGetAttribute(&ctx->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) ctx->n_cu = 0;
    if (const char* e = std::getenv("PGPS_WC_ROWS2")) ctx->wc_rows2 = std::atoi(e) & 15;            // diagnostic, see pgps_wc.hip
    if (const char* e = std::getenv("PGPS_WC_SERIAL3")) ctx->wc_serial3 = (e[0] == '1');      // diagnostic, see pgps_wc.hip
    // (the resident launch's hand-off records are zeroed HERE and never again: a granule's tag is the epoch of the launch that
    // wrote it, epochs only grow, so a zero or an old tag never matches)
    if (hipMalloc((void**)&ctx->status_word, pgps::kStatusBytes) != hipSuccess ||
        hipMemset(ctx->status_word, 0, pgps::kStatusBytes) != hipSuccess ||
        hipMalloc((void**)&ctx->res_gran, pgps::kResGranBytes) != hipSuccess ||
        hipMemset(ctx->res_gran, 0, pgps::kResGranBytes) != hipSuccess) {
        if (ctx->res_gran) (void)hipFree(ctx->res_gran);
        if (ctx->status_word) (void)hipFree(ctx->status_word);
        (void)hipStreamDestroy(ctx->own_stream);
        delete ctx;
        return PGPS_E_NOMEM;
    }
    *out = ctx;
    return PGPS_OK;
}

extern "C" int pgps_destroy(pgps_ctx* ctx) {
    if (!ctx) return PGPS_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm) (void)pgps_comm_destroy(ctx);
    if (ctx->comm_buf.p) (void)hipFree(ctx->comm_buf.p);
    if (ctx->ws.p) (void)hipFree(ctx->ws.p);
    if (ctx->stamps.p) (void)hipFree(ctx->stamps.p);
    if (ctx->res_stamps.p) (void)hipFree(ctx->res_stamps.p);
    if (ctx->gadj.p) (void)hipFree(ctx->gadj.p);
    if (ctx->panel.p) (void)hipFree(ctx->panel.p);
    if (ctx->pin_d.p) (void)hipFree(ctx->pin_d.p);
    if (ctx->pin_h) (void)hipHostFree(ctx->pin_h);
    if (ctx->out_h) (void)hipHostFree(ctx->out_h);
    if (ctx->status_word) (void)hipFree(ctx->status_word);
    if (ctx->res_gran) (void)hipFree(ctx->res_gran);
    for (auto& b : ctx->st)
        if (b.p) (void)hipFree(b.p);
    for (auto& b : ctx->lti)
        if (b.p) (void)hipFree(b.p);
    for (auto& b : ctx->wide)
        if (b.p) (void)hipFree(b.p);
    if (ctx->smp.p) (void)hipFree(ctx->smp.p);
    if (ctx->smp_wide.p) (void)hipFree(ctx->smp_wide.p);
    if (ctx->probe_host) (void)hipHostFree(ctx->probe_host);
    for (auto& e : ctx->ev_pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return PGPS_OK;
}

extern "C" int pgps_set_stream(pgps_ctx* ctx, void* s) {
    if (!ctx) return PGPS_E_INVALID;
    ctx->stream = (hipStream_t)s;       // NULL = the HIP null (default) stream, as in HIP itself
    return PGPS_OK;
}

extern "C" int pgps_use_own_stream(pgps_ctx* ctx) {
    if (!ctx) return PGPS_E_INVALID;
    ctx->stream = ctx->own_stream;
    return PGPS_OK;
}

extern "C" int pgps_synchronize(pgps_ctx* ctx) {
    if (!ctx) return PGPS_E_INVALID;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGPS_OK;
}

extern "C" int pgps_set_chunk(pgps_ctx* ctx, int c) {
    if (!ctx || c < 0) return PGPS_E_INVALID;
    ctx->chunk = c;
    return PGPS_OK;
}

// diagnostic build only: copy the (3, nblocks, 8) stamp buffer of the last scan to the host
extern "C" int pgps_debug_read_stamps(pgps_ctx* ctx, long long* out, long n_values) {
    if (!ctx || !out) return PGPS_E_INVALID;
    if (!ctx->stamps.p || (size_t)n_values * sizeof(long long) > ctx->stamps.cap) return PGPS_E_INVALID;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, ctx->stamps.p, (size_t)n_values * sizeof(long long), hipMemcpyDeviceToHost));
    return PGPS_OK;
}

// Diagnostic flags raised by kernels (bit 1: a look-back spin of the single-pass filter hit its bound).
// Synchronises, returns and clears them.
extern "C" int pgps_status(pgps_ctx* ctx, int* flags) {
    if (!ctx || !flags) return PGPS_E_INVALID;
    *flags = 0;
    if (!ctx->status_word) return PGPS_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(flags, ctx->status_word, sizeof(int), hipMemcpyDeviceToHost));
    if (*flags) HIPCHK(ctx, hipMemset(ctx->status_word, 0, sizeof(int)));
    *flags |= ctx->host_flags;
    ctx->host_flags = 0;
    return PGPS_OK;
}

extern "C" int pgps_set_f32_policy(pgps_ctx* ctx, int policy) {
    if (!ctx || policy < 0 || policy > 2) return PGPS_E_INVALID;
    ctx->f32_policy = policy;
    return PGPS_OK;
}

extern "C" int pgps_set_single_pass(pgps_ctx* ctx, int mode, int window) {
    if (!ctx || mode < -1 || mode > 1 || window < 0 || window > 256) return PGPS_E_INVALID;
    ctx->single_pass = mode;
    if (window > 0) ctx->lookback_window = window;
    return PGPS_OK;
}

extern "C" int pgps_set_shortcut(pgps_ctx* ctx, int on) {
    if (!ctx || on < 0 || on > 1) return PGPS_E_INVALID;
    ctx->shortcut = on;
    return PGPS_OK;
}

extern "C" int pgps_set_resident(pgps_ctx* ctx, int mode) {
    if (!ctx || mode < -1 || mode > 2) return PGPS_E_INVALID;
    ctx->resident = mode;
    return PGPS_OK;
}

// diagnostics: the cycle stamps of the last resident launch made with pgps_set_resident(ctx, 2): (workgroups, 16) long long
extern "C" int pgps_resident_stamps(pgps_ctx* ctx, long long* out, int max_blocks, int* n_blocks) {
    if (!ctx || !n_blocks) return PGPS_E_INVALID;
    *n_blocks = ctx->res_stamp_blocks;
    if (!out || max_blocks <= 0 || !ctx->res_stamps.p) return PGPS_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const int n = ctx->res_stamp_blocks < max_blocks ? ctx->res_stamp_blocks : max_blocks;
    HIPCHK(ctx, hipMemcpy(out, ctx->res_stamps.p, (size_t)n * 16 * sizeof(long long), hipMemcpyDeviceToHost));
    return PGPS_OK;
}

// diagnostics: every wave's end of the reduce and of the Kalman pass in the last resident launch made with
// pgps_set_resident(ctx, 2): (workgroups, 8) long long, [k * 4 + wave], after the (workgroups, 16) table on the device
extern "C" int pgps_resident_wave_stamps(pgps_ctx* ctx, long long* out, int max_blocks, int* n_blocks) {
    if (!ctx || !n_blocks) return PGPS_E_INVALID;
    *n_blocks = ctx->res_stamp_blocks;
    if (!out || max_blocks <= 0 || !ctx->res_stamps.p) return PGPS_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const int n = ctx->res_stamp_blocks < max_blocks ? ctx->res_stamp_blocks : max_blocks;
    const long long* waves = (const long long*)ctx->res_stamps.p + (size_t)ctx->res_stamp_blocks * 16;
    HIPCHK(ctx, hipMemcpy(out, waves, (size_t)n * 8 * sizeof(long long), hipMemcpyDeviceToHost));
    return PGPS_OK;
}

// diagnostics: start skew of the resident launch (pgps_resident.hip.h, res_skew)
extern "C" int pgps_debug_resident_delay(pgps_ctx* ctx, int tile, int phase, int microseconds) {
    if (!ctx || tile < -1 || tile > 255 || (tile >= 0 && (phase < 1 || phase > 2 || microseconds < 0 || microseconds > 10000)))
        return PGPS_E_INVALID;
    if (tile < 0) {
        ctx->res_delay_tile = -1;
        ctx->res_delay_phase = 0;
        ctx->res_delay_ticks = 0;
        return PGPS_OK;
    }
    int khz = 0;
    HIPCHK(ctx, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
    if (khz <= 0) return PGPS_E_HIP;
    ctx->res_delay_tile = tile;
    ctx->res_delay_phase = phase;
    ctx->res_delay_ticks = (long long)microseconds * khz / 1000;
    return PGPS_OK;
}

extern "C" int pgps_set_family(pgps_ctx* ctx, int family) {
    if (!ctx || family < 0 || family > 4) return PGPS_E_INVALID;
    ctx->family = family;
    return PGPS_OK;
}
extern "C" int pgps_set_block(pgps_ctx* ctx, int lanes) {
    if (!ctx || (lanes != 0 && lanes != kBlockNarrow && lanes != 256)) return PGPS_E_INVALID;
    ctx->block = lanes;
    return PGPS_OK;
}

extern "C" int pgps_set_one_launch(pgps_ctx* ctx, int max_steps) {
    if (!ctx || max_steps < -1 || max_steps > (1 << 16)) return PGPS_E_INVALID;
    ctx->one_launch = max_steps;
    return PGPS_OK;
}

extern "C" int pgps_set_grad_pack(pgps_ctx* ctx, long max_steps) {
    if (!ctx || max_steps < -1) return PGPS_E_INVALID;
    ctx->grad_pack = max_steps;
    return PGPS_OK;
}

extern "C" int pgps_set_rc_scan(pgps_ctx* ctx, int mode) {
    if (!ctx || mode < -1 || mode > 1) return PGPS_E_INVALID;
    ctx->rc_scan = mode;
    return PGPS_OK;
}

extern "C" int pgps_set_dma(pgps_ctx* ctx, int mode) {
    if (!ctx || mode < -1 || mode > 1) return PGPS_E_INVALID;
    ctx->dma = mode;
    return PGPS_OK;
}

extern "C" int pgps_set_stage(pgps_ctx* ctx, int g) {
    if (!ctx || !(g == -1 || g == 0 || g == 2 || g == 4)) return PGPS_E_INVALID;
    ctx->stage_g = g;
    return PGPS_OK;
}

extern "C" const char* pgps_last_hip_error(pgps_ctx* ctx) { return ctx ? ctx->hip_err.c_str() : ""; }

extern "C" int pgps_malloc(pgps_ctx* ctx, size_t bytes, void** dptr) {
    if (!ctx || !dptr) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 16);
    if (e != hipSuccess) { ctx->hip_err = hipGetErrorString(e); return PGPS_E_NOMEM; }
    return PGPS_OK;
}
extern "C" int pgps_free(pgps_ctx* ctx, void* dptr) {
    if (!ctx) return PGPS_E_INVALID;
    if (dptr) HIPCHK(ctx, hipFree(dptr));
    return PGPS_OK;
}
extern "C" int pgps_memcpy_h2d(pgps_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx || (!dst && bytes) || (!src && bytes)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGPS_OK;
}
extern "C" int pgps_memcpy_d2h(pgps_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx || (!dst && bytes) || (!src && bytes)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGPS_OK;
}

// ---------------------------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------------------------
static const char* kKernelNames[PGPS_K_COUNT] = {"k_filter_reduce", "k_filter_apply", "k_smoother_reduce",
                                                 "k_smoother_apply", "k_ll_finalize", "k_discretise", "k_pkfs_resident"};
extern "C" const char* pgps_kernel_name(int slot) {
    return (slot >= 0 && slot < PGPS_K_COUNT) ? kKernelNames[slot] : "";
}

namespace pgps {
int prof_flush(pgps_ctx* ctx) {
    if (ctx->ev_used == 0) return PGPS_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < ctx->ev_used; ++i) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev_pool[i].a, ctx->ev_pool[i].b));
        ctx->prof_ms[ctx->ev_pool[i].slot] += ms;
        ctx->prof_n[ctx->ev_pool[i].slot] += 1;
    }
    ctx->ev_used = 0;
    return PGPS_OK;
}

pgps_ctx::EvPair* prof_acquire(pgps_ctx* c, int slot) {
    if (!((c->profiling >> slot) & 1u)) return nullptr;
    if ((c->prof_seen[slot]++ % c->prof_every) != 0) return nullptr;
    if (c->ev_used == c->ev_pool.size()) {
        if (c->ev_pool.size() >= 1024) {
            if (prof_flush(c) != PGPS_OK) return nullptr;
        } else {
            pgps_ctx::EvPair p;
            if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return nullptr;
            c->ev_pool.push_back(p);
        }
    }
    pgps_ctx::EvPair* ev = &c->ev_pool[c->ev_used++];
    ev->slot = slot;
    return ev;
}
}  // namespace pgps

extern "C" int pgps_profile_enable(pgps_ctx* ctx, int on) {
    if (!ctx) return PGPS_E_INVALID;
    if (!on) { int rc = prof_flush(ctx); if (rc) return rc; }
    if (on && ctx->ev_pool.empty()) {
        // create the events (and exercise them once) up front: the first hipEventRecord on a fresh
        // event allocates its signal, which can stall the queue for milliseconds
        HIPCHK(ctx, hipSetDevice(ctx->device));
        for (int i = 0; i < 1024; ++i) {
            pgps_ctx::EvPair p;
            HIPCHK(ctx, hipEventCreate(&p.a));
            HIPCHK(ctx, hipEventCreate(&p.b));
            p.slot = 0;
            ctx->ev_pool.push_back(p);
            HIPCHK(ctx, hipEventRecord(p.a, ctx->stream));
            HIPCHK(ctx, hipEventRecord(p.b, ctx->stream));
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->profiling = (unsigned)on;
    for (int i = 0; i < PGPS_K_COUNT; ++i) ctx->prof_seen[i] = 0;
    return PGPS_OK;
}

// mean elapsed time of an EMPTY hipEvent pair on the context's stream: what a pair adds to the
// duration it brackets (subtract it to compare with a profiler's pure kernel time)
extern "C" int pgps_profile_calibrate(pgps_ctx* ctx, double* empty_pair_ms) {
    if (!ctx || !empty_pair_ms) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipEvent_t a, b;
    HIPCHK(ctx, hipEventCreate(&a));
    HIPCHK(ctx, hipEventCreate(&b));
    double acc = 0.0;
    const int reps = 64;
    for (int i = 0; i < reps + 8; ++i) {
        HIPCHK(ctx, hipEventRecord(a, ctx->stream));
        HIPCHK(ctx, hipEventRecord(b, ctx->stream));
        HIPCHK(ctx, hipEventSynchronize(b));
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, a, b));
        if (i >= 8) acc += ms;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *empty_pair_ms = acc / reps;
    return PGPS_OK;
}

extern "C" int pgps_profile_sample(pgps_ctx* ctx, int every_n) {
    if (!ctx || every_n < 1) return PGPS_E_INVALID;
    ctx->prof_every = every_n;
    return PGPS_OK;
}

extern "C" int pgps_profile_read(pgps_ctx* ctx, double* total_ms, long* launches, int reset) {
    if (!ctx) return PGPS_E_INVALID;
    int rc = prof_flush(ctx);
    if (rc) return rc;
    for (int i = 0; i < PGPS_K_COUNT; ++i) {
        if (total_ms) total_ms[i] = ctx->prof_ms[i];
        if (launches) launches[i] = ctx->prof_n[i];
        if (reset) { ctx->prof_ms[i] = 0; ctx->prof_n[i] = 0; }
    }
    return PGPS_OK;
}

// ---------------------------------------------------------------------------------------------
// launch geometry
// ---------------------------------------------------------------------------------------------
namespace pgps {
void geometry(const pgps_ctx* ctx, long N, int* Lc, int* nblocks, int d) {
    int c = ctx->chunk;
    if (c <= 0) {
        // 16 steps per lane (the lane-serial part then outweighs the scan trees: measured at 2^20)
        // until that would need more than 1024 workgroups (every workgroup folds the spine entries
        // on its side); shorter series use fewer steps per lane so the chip is still covered;
        // multiples of 4 = whole LDS-staged sub-tiles.
        long v = 16;
        // from 2^21 steps 32 per lane still fill every CU (>= 256 workgroups) and halve the scan trees and their scratch
        // per step: 2^21 0.166 -> 0.154 ms, 2^24 1.27 -> 1.13 ms; at 2^20 half the CUs would idle (0.086 -> 0.092 ms)
        if (d >= 1 && d <= 2 && N >= (long)kBlock * 32 * 256) v = 32;        // (measured on the array path at d = 2)
        // (2^24 steps, d = 2: 2048 workgroups of 32 steps per lane 1.13 ms, 1024 of 64 steps 1.29 ms)
        const long max_blocks = (d >= 1 && d <= 2) ? 2048 : 1024;
        if (N > (long)kBlock * v * max_blocks) v = (N + (long)kBlock * max_blocks - 1) / ((long)kBlock * max_blocks);
        while (v > 4 && (long)kBlock * v * 128 > N) v /= 2;   // keep >= 128 workgroups when N allows
        if (N < (long)kBlock * 4) v = (N + kBlock - 1) / kBlock;
        if (v < 1) v = 1;
        if (v > 4) v = (v + 3) / 4 * 4;
        c = (int)v;
    }
    long nb = (N + (long)kBlock * c - 1) / ((long)kBlock * c);
    if (nb < 1) nb = 1;
    *Lc = c;
    *nblocks = (int)nb;
}
// Steps per lane and workgroups of the 128-lane build.  Up to d = 3 one workgroup per CU where the series allows it (256
// workgroups, up to 32 steps per lane: measured at d = 2 from 2^17 to 2^20 steps and at d = 3), from d = 4 sixteen
// steps per lane (RBF order 4 / 6 at 2^20: 16 and 32 steps per lane 0.40 / 0.40 and 0.59 / 0.62 ms).
void geometry_narrow(const pgps_ctx* ctx, long N, int* Lc, int* nblocks, int d) {
    int c = ctx->chunk;
    if (c <= 0) {
        long v;
        if (d <= 3) {
            v = (N + (long)kBlockNarrow * 256 - 1) / ((long)kBlockNarrow * 256);
            v = v < 4 ? 4 : (v > 32 ? 32 : v);
            const long max_blocks = 4096;
            if (N > (long)kBlockNarrow * v * max_blocks) v = (N + (long)kBlockNarrow * max_blocks - 1) / ((long)kBlockNarrow * max_blocks);
        } else {
            v = 16;
            const long max_blocks = 2048;
            if (N > (long)kBlockNarrow * v * max_blocks) v = (N + (long)kBlockNarrow * max_blocks - 1) / ((long)kBlockNarrow * max_blocks);
            while (v > 4 && (long)kBlockNarrow * v * 256 > N) v /= 2;
        }
        if (N < (long)kBlockNarrow * 4) v = (N + kBlockNarrow - 1) / kBlockNarrow;
        if (v < 1) v = 1;
        if (v > 4) v = (v + 3) / 4 * 4;
        c = (int)v;
    }
    long nb = (N + (long)kBlockNarrow * c - 1) / ((long)kBlockNarrow * c);
    *Lc = c;
    *nblocks = (int)(nb < 1 ? 1 : nb);
}
// B models (or column groups) over one series of N steps, (workgroups, models) grids of 256-lane workgroups -- ONE statement
// for every batched fused launch: they promise results that do not depend on how a batch is split into groups, which holds
// only while they agree on the geometry.  pgps_set_chunk's value, else 16 steps per lane while the batch keeps the chip
// covered (>= 1024 workgroups: the serial part is the efficient one), halved towards 4 when B x N is small; a series shorter
// than four steps per lane of one workgroup takes one workgroup
int batch_steps_per_lane(const pgps_ctx* ctx, int B, long N) {
    int lc = ctx->chunk;
    if (lc <= 0) {
        lc = 16;
        while (lc > 4 && (long)B * ((N + (long)kBlock * lc - 1) / ((long)kBlock * lc)) < 1024) lc /= 2;
        if (N < (long)kBlock * 4) lc = (int)((N + kBlock - 1) / kBlock);
        if (lc < 1) lc = 1;
    }
    return lc;
}
// ... and the multi-output launches' steps per lane and workgroups by it, from the column groups of the whole call
void multi_geometry(const pgps_ctx* ctx, long N, int groups_all, int* Lc, int* nblocks) {
    *Lc = batch_steps_per_lane(ctx, groups_all, N);
    *nblocks = (int)((N + (long)kBlock * *Lc - 1) / ((long)kBlock * *Lc));
}
}  // namespace pgps

namespace pgps {
bool lane_narrow(const pgps_ctx* ctx, int d, long N) {
    return ctx->block != 256 && (ctx->block == kBlockNarrow || !(d <= 3 && N >= (1L << 22)));
}
}  // namespace pgps

namespace pgps {
// The resident launch (pgps_resident.hip.h) serves whole-series filter + smoother calls at d = 2 in fp64 whose
// 256 x 16-step workgroups are all resident at once (one per CU); automatic from kResAutoMin steps, where the scan's
// streaming outweighs the two grid barriers (below that the narrow build's smaller chunks cover more of the chip).
constexpr long kResAutoMin = 1L << 17;       // (2^17 steps: 26.9 against 28.8 us on three launches; equal at 2^16: profiles/r05_experiments.txt item 12)
bool resident_fits(const pgps_ctx* ctx, long N, int d, bool f32) {
    if (f32 || d != 2 || ctx->resident == 0 || ctx->n_cu <= 0) return false;
    // a pinned geometry or variant of the three-launch path was asked for (a chunk of 8 or 16 together with mode >= 1 pins the
    // resident launch's own steps per lane instead: tests, A/B)
    const bool own_chunk = ctx->resident > 0 && (ctx->chunk == 8 || ctx->chunk == 16);
    if ((ctx->chunk > 0 && !own_chunk) || ctx->block != 0 || ctx->stage_g >= 0 || ctx->single_pass > 0 || ctx->dma > 0) return false;
    if (ctx->family != 0 && ctx->family != 1) return false;
    // one workgroup per CU, and at most kResMaxBlocks of them (the hand-off records, one record per lane in the general fold)
    const long max_blocks = ctx->n_cu < kResMaxBlocks ? ctx->n_cu : kResMaxBlocks;
    if (N > (long)kBlock * (own_chunk ? ctx->chunk : kResLc) * max_blocks) return false;
    // not while the stream is being captured: the launch's barrier set and hand-off epoch are chosen per launch on the host,
    // and a replayed graph would present the same ones again (counters already at their targets, granule tags already equal)
    if (!(ctx->resident > 0 || N >= kResAutoMin)) return false;         // (before the query below: short series never pay for it)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs == hipStreamCaptureStatusNone;
}
}  // namespace pgps

extern "C" int pgps_get_geometry(pgps_ctx* ctx, long N, int d, int* lanes, int* Lc, int* nb) {
    if (!ctx || N < 1 || d < 1 || d > PGPS_MAX_DIM_LANE || !lanes || !Lc || !nb) return PGPS_E_INVALID;
    if (lane_narrow(ctx, d, N)) { *lanes = kBlockNarrow; geometry_narrow(ctx, N, Lc, nb, d); }
    else { *lanes = kBlock; geometry(ctx, N, Lc, nb, d); }
    return PGPS_OK;
}

extern "C" int pgps_get_chunk(pgps_ctx* ctx, long N, int* Lc, int* nb) {
    if (!ctx || N < 1 || !Lc || !nb) return PGPS_E_INVALID;
    geometry(ctx, N, Lc, nb);
    return PGPS_OK;
}
// ... and of the batched fused launches: batch_steps_per_lane and the workgroups per model by it (launch_gp_batch, form 2 of
// launch_gp_predict_batch, the four-launch road of launch_gp_adj_batch: pgps_inst.hip)
extern "C" int pgps_get_batch_chunk(pgps_ctx* ctx, int B, long N, int* Lc, int* nb) {
    if (!ctx || B < 1 || N < 1 || !Lc || !nb) return PGPS_E_INVALID;
    *Lc = batch_steps_per_lane(ctx, B, N);
    *nb = (int)((N + (long)kBlock * *Lc - 1) / ((long)kBlock * *Lc));
    return PGPS_OK;
}
// ... and of a panel launch (one workgroup per series): panel_steps_per_lane, the rule of every panel planner (pgps_scratch.h)
extern "C" int pgps_get_panel_chunk(pgps_ctx* ctx, long m, int* Lc) {
    if (!ctx || m < 1 || m > PGPS_PANEL_MAX_STEPS || !Lc) return PGPS_E_INVALID;
    *Lc = panel_steps_per_lane(m, ctx->chunk);
    return PGPS_OK;
}
// ---------------------------------------------------------------------------------------------
// batched predict_f: its settings, and its results on their way to the host
// ---------------------------------------------------------------------------------------------
extern "C" int pgps_set_batch_scratch(pgps_ctx* ctx, size_t bytes) {
    if (!ctx) return PGPS_E_INVALID;
    ctx->batch_scratch = bytes;
    return PGPS_OK;
}
extern "C" int pgps_set_batch_form(pgps_ctx* ctx, int form) {
    if (!ctx || form < 0 || form > 2) return PGPS_E_INVALID;
    ctx->batch_form = form;
    return PGPS_OK;
}

// Device results -> pageable host arrays through a pinned buffer of the context (kept, grown on demand) and a memcpy: an
// asynchronous copy straight into pageable memory pins the destination's pages on its way (measured on predict_f_batch:
// 3.2 MB of results took 19 ms of a 20 ms call that way).  Synchronises the stream.  Above kOutPinnedMax, or when the
// pinned allocation fails, the parts are copied directly.
constexpr size_t kOutPinnedMax = (size_t)1 << 30;
int pgps::copy_out(pgps_ctx* ctx, const OutPart* parts, int n) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (parts[i].bytes + 255) / 256 * 256;
    if (total <= kOutPinnedMax && total > ctx->out_cap) {
        if (ctx->out_h) (void)hipHostFree(ctx->out_h);
        ctx->out_h = nullptr;
        ctx->out_cap = 0;
        if (hipHostMalloc((void**)&ctx->out_h, total + total / 8, hipHostMallocDefault) == hipSuccess) ctx->out_cap = total + total / 8;
        else { ctx->out_h = nullptr; (void)hipGetLastError(); }
    }
    const bool pinned = total <= ctx->out_cap;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        void* dst = pinned ? (void*)(ctx->out_h + off) : parts[i].host;
        HIPCHK(ctx, hipMemcpyAsync(dst, parts[i].dev, parts[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
        off += (parts[i].bytes + 255) / 256 * 256;
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (pinned) {
        off = 0;
        for (int i = 0; i < n; ++i) {
            std::memcpy(parts[i].host, ctx->out_h + off, parts[i].bytes);
            off += (parts[i].bytes + 255) / 256 * 256;
        }
    }
    return PGPS_OK;
}

int pgps::batch_ll_result(int B, const double* llh, double* ll) {
    bool finite = true;
    for (int i = 0; i < B; ++i) {
        if (ll) ll[i] = llh[i];
        finite = finite && std::isfinite(llh[i]);
    }
    return finite ? PGPS_OK : PGPS_E_NUMERIC;
}

int pgps::copy_out_batch(pgps_ctx* ctx, int B, OutPart mean, OutPart var, const double* dll, double* ll) {
    std::vector<double> llh((size_t)B, 0.0);
    const OutPart parts[3] = {mean, var, {llh.data(), dll, (size_t)B * sizeof(double)}};
    TRY(copy_out(ctx, parts, 3));
    return batch_ll_result(B, llh.data(), ll);
}
