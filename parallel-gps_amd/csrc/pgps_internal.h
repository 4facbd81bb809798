// pgps_internal.h -- context, scratch and launch plumbing shared by the C-ABI translation
// unit (pgps_core.hip) and the per-(dtype, d) kernel translation units (pgps_inst.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <string>
#include <vector>

#include "../../include/pgps.h"
#include "pgps_dyn.h"

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct pgps_ctx {
    int device = 0;
    int n_cu = 0;                       // compute units of the device (hipDeviceAttributeMultiprocessorCount)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int chunk = 0;                      // 0 = auto
    int stage_g = -1;                   // LDS staging: -1 = auto, 0 = off, 2 / 4 = steps per sub-tile
    int single_pass = -1;               // single-pass filter kernel: -1 = auto, 0 = off, 1 = on
    int lookback_window = 256;          // tiles per look-back window (<= 256; small values are for tests)
    int block = 0;                      // lane-chunk workgroups: 0 = auto, 128 / 256 lanes (pgps_set_block)
    size_t batch_scratch = 0;           // batched predict: scratch budget in bytes, 0 = the family's default (pgps_scratch.h; pgps_set_batch_scratch)
    int batch_form = 0;                 // batched fused predict: 0 = automatic, 1 = one workgroup per model, 2 = three launches (pgps_set_batch_form)
    int one_launch = -1;                // fused (pgps_gp_*) calls of short series in ONE launch: -1 = auto (N <= kOneLaunchAuto), 0 = never, n > 0 = up to n steps
    long grad_pack = -1;                // gradient at d <= 2: one direction per model up to this many steps (-1 = automatic, 0 = never)
    int rc_scan = -1;                   // scans of the chain totals (row- / quad-cooperative families): -1 = auto, 0 = one launch per Kogge-Stone level, 1 = blocked (pgps_set_rc_scan)
    int dma = -1;                       // LDS-DMA ring in the Kalman pass (d = 2 fp64, 128-lane build): -1 = auto, 0 = off, 1 = on
    int shortcut = 1;                   // forgetting shortcut for the carry across workgroups (pgps_set_shortcut): 1 = where it applies, 0 = never
    int resident = -1;                  // one resident launch for filter + smoother (pgps_resident.hip.h): -1 = auto, 0 = off, 1 = on where it fits, 2 = on + phase stamps
    unsigned res_epoch = 0;             // launches of the resident kernel so far: picks the barrier's counter set
    unsigned long long* res_gran = nullptr;     // the resident kernel's hand-off records (tagged granules, kResGranBytes): made and zeroed with the context
    DevBuf res_stamps;                  // diagnostics: (workgroups, 16) cycle stamps of the last resident launch
    int res_stamp_blocks = 0;
    int res_delay_tile = -1;            // diagnostics (pgps_debug_resident_delay): the workgroup that waits before it publishes, -1 = none
    int res_delay_phase = 0;            // ... its phase-1 (1) or phase-2 (2) total
    long long res_delay_ticks = 0;      // ... for this many wall-clock ticks
    int family = 0;                     // 0 = auto (lane-chunk d <= 6; row-cooperative fp64 d <= 16; else wave-cooperative), 1 = lane, 2 = wave, 3 = row
    std::string hip_err;
    DevBuf ws;                          // scratch of the scan kernels
    DevBuf st[12];                      // staging buffers of the host entry points
    bool wc_attr_done[2][17] = {};      // wave-cooperative kernels: dynamic-LDS attributes set (by dtype, DP / 2)
    int wc_rows2 = 15;                  // d = 17..32: two-rows level-1 kernels (pgps_rc2.hip.h); 0 = the LDS-tile ones (env PGPS_WC_ROWS2)
    int wc_serial3 = 0;                 // wave-cooperative family: serial level 3 instead of Kogge-Stone (env PGPS_WC_SERIAL3)
    DevBuf lti[12];                     // general-LTI entry points: model, merged series, Fs, Qs, E, g (d > 16: moments)
    DevBuf stamps;                      // diagnostic build only
    int* status_word = nullptr;         // device word kernels raise flags in (pgps_status)
    int host_flags = 0;                 // flags raised on the host side (bit 2: a float32 call ran in fp64 arithmetic), reported and cleared by pgps_status
    int f32_policy = 0;                 // float32 series with a smoother: 0 = automatic promotion on dense grids, 1 = always native, 2 = always fp64 arithmetic (pgps_set_f32_policy)
    int* probe_host = nullptr;          // pinned word pair the dense-grid probe of a float32 call writes (and its device alias)
    int* probe_dev = nullptr;
    int probe_seq = 0;                  // sequence number of the last probe: its last workgroup writes it to probe_host[0] behind the verdict
    int f32_last_promoted = 0;          // which way the last probed call went: decides the ORDER of the next one (see pgps_core.hip)
    // small host-array calls (pgps_gp_predict_*, pgps_lti_predict_f64, ...): one pinned arena, ONE copy in and ONE copy out
    char* pin_h = nullptr;              // hipHostMalloc, kPinArena bytes, made at the first small call
    DevBuf pin_d;                       // its device twin
    char* out_h = nullptr;              // pinned staging of the batched predict's (B, K) results on their way to pageable host arrays
    size_t out_cap = 0;
    DevBuf panel;                       // ragged batch of series (pgps_panel_inst.hip): [model table | descriptor table]
    DevBuf gadj;                        // fused-path adjoint gradient (pgps_gpadj.hip.h): kept states of the forward pass, workgroup partials
    DevBuf wide[9];                     // fp64 copies of a promoted float32 call's arrays: P0, H, Fs, Qs, ys, fms, fPs, sms, sPs
    DevBuf smp;                         // backward sampler (pgps_sample.hip.h): lane suffixes and spine of every sample group
    DevBuf smp_wide;                    // ... a promoted float32 call's fp64 draws and output
    DevBuf cov[6];                      // joint covariance (pgps_cov.hip.h): scan workspace, step slots, gain products, selected sPs, tile products, staged selection
    DevBuf cov_wide;                    // ... a promoted float32 call's fp64 output
    void* comm = nullptr;               // ncclComm_t (RCCL) of a series sharded over GPUs: pgps_comm_init (pgps_comm.hip)
    int comm_rank = 0, comm_nranks = 0;
    DevBuf comm_buf;                    // [rec_f | rec_s | gathered_f | gathered_s] of pgps_pkfs_seg_dev_*
    // the three-phase segment protocol keeps state in `ws` between its calls: what the last phase left, and the
    // workspace epoch (bumped by every call that carves `ws`) it left it at
    struct SegTag { int phase = 0; long N = 0; int d = 0, rank = 0, nranks = 0, chunk = 0, block = 0, family = 0, stage_g = 0, dma = 0, rc_scan = 0; unsigned long epoch = 0; } seg_tag;
    unsigned long ws_epoch = 0;
    unsigned profiling = 0;             // bit i = time launches of slot PGPS_K_* i
    int prof_every = 1;                 // time every n-th launch of an enabled slot
    long prof_seen[PGPS_K_COUNT] = {0};
    struct EvPair { hipEvent_t a, b; int slot; };
    std::vector<EvPair> ev_pool;
    size_t ev_used = 0;
    double prof_ms[PGPS_K_COUNT] = {0};
    long prof_n[PGPS_K_COUNT] = {0};
};

// roctx range named after the reference's tf.name_scope of the same work (pssgp/kalman/parallel.py:122 "parallel_filter",
// pssgp/model.py:35 "merge_sorted", model.py:87 "make_model"): visible in `rocprofv3 --marker-trace`, a no-op otherwise
struct RoctxRange {
    explicit RoctxRange(const char* name) { pgps::dyn::range_push(name); }
    ~RoctxRange() { pgps::dyn::range_pop(); }
    RoctxRange(const RoctxRange&) = delete;
    RoctxRange& operator=(const RoctxRange&) = delete;
};

#define HIPCHK(ctx, expr)                                                        \
    do {                                                                         \
        hipError_t e_ = (expr);                                                  \
        if (e_ != hipSuccess) {                                                  \
            (ctx)->hip_err = std::string(#expr) + ": " + hipGetErrorString(e_);  \
            return PGPS_E_HIP;                                                   \
        }                                                                        \
    } while (0)

namespace pgps {

#ifndef PGPS_BLOCK
#define PGPS_BLOCK 256
#endif
constexpr int kBlock = PGPS_BLOCK;      // lanes per workgroup (experiments: make EXTRA=-DPGPS_BLOCK=128 ...)
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
// fused path: series up to this length run as one workgroup, one launch (pgps_set_one_launch).  c1 (4096 + 1024 steps):
// one launch 82 us per predict_f against 61 us for the three launches, 40 against 38 us for the log-likelihood; N = 1000:
// 57 against 89 us -- profiles/r03_small_n_latency.txt
constexpr int kOneLaunchAuto = 2048;

int ensure(pgps_ctx* ctx, DevBuf& b, size_t bytes);
// all-gather of `bytes` per rank on the context's stream through the context's RCCL communicator (pgps_comm.hip)
int comm_allgather(pgps_ctx* ctx, const void* send, void* recv, size_t bytes);
int prof_flush(pgps_ctx* ctx);
void geometry(const pgps_ctx* ctx, long N, int* Lc, int* nblocks, int d = 0);

// Per-kernel timing: when the launch is sampled (pgps_profile_enable / _sample) the kernel goes out
// through hipExtLaunchKernelGGL, which stamps the two events with the dispatch's own start / end
// timestamps (the same clock rocprofv3's kernel trace reads), not with separate event packets.
pgps_ctx::EvPair* prof_acquire(pgps_ctx* ctx, int slot);

template <typename T>
struct ScanArgs {
    long N;                 // steps in this segment
    int Lc;                 // steps per lane
    int nblocks;            // workgroups
    long nlanes;            // nblocks * kBlock (stride of the field-major workspaces)
    // segment position in the whole series (single GPU: first = last = 1)
    int seg_first;          // step 0 of this segment is the first step of the series
    int seg_last;           // step N-1 of this segment is the last step of the series
    // model
    const T* P0;            // (d, d) prior covariance              [device]
    const T* H;             // (d,)   observation row               [device]
    T R;                    // observation noise variance
    // series
    const T* Fs;            // (N, d, d)
    const T* Qs;            // (N, d, d)
    const T* ys;            // (N,)   NaN = missing
    // stitching across segments (multi-GPU); unused when seg_first / seg_last
    const T* carry_in;      // (d + d*d) filtered (m, P full) entering this segment
    const T* halo_FQ;       // (2, d, d) F, Q of the first step of the NEXT segment
    const T* carry_back;    // (d + d*d) smoothed (m, P full) of the first step of the NEXT segment
    // outputs
    T* fms; T* fPs; T* sms; T* sPs;
    double* ll;             // scalar log-likelihood (of this segment)
    // workspace
    T* spine;               // (nblocks, NFILT)
    T* lpre;                // (NFILT, nlanes)
    T* sspine;              // (nblocks, NSMTH)
    T* lsuf;                // (NSMTH, nlanes)
    double* llpart;         // (nblocks,)
    int* status;            // != 0: a non-positive innovation variance was met
    // multi-GPU stitching (pgps_seg_*): records exchanged between ranks
    int rank, nranks;
    T* rec_f;               // out: this segment's filter record  [NFILT total | F_0 | Q_0]
    const T* gathered_f;    // in : (nranks, REC_F) all ranks' filter records
    T* rec_s;               // out: this segment's smoother record [NSMTH total | pad | ll partial (double)]
    const T* gathered_s;    // in : (nranks, REC_S)
    T* seg_ws;              // scratch: carry_in (d+d*d) | halo_FQ (2 d*d) | carry_back (d+d*d)
    int nt;                 // streaming stores for the outputs (pass larger than the Infinity Cache)
    // single-pass filter (k_filter_single): inter-workgroup look-back state, zeroed before every launch
    int* ticket;            // dynamic tile counter
    int* flags;             // (nblocks,) 0 = nothing, 1 = aggregate published, 2 = inclusive prefix published
    int ll_in_apply;        // filter-only calls: the apply kernel's last workgroup sums the log-likelihood (no finalize launch)
    T* incl;                // (nblocks, d + d(d+1)/2) inclusive (m, P) of the window-closing tiles
    int win;                // look-back window (tiles); <= kBlock
    long long* stamps;      // diagnostic build only (-DPGPS_STAMPS): (3 kernels, nblocks, 8) s_memtime stamps
    int shortcut;           // try the forgetting shortcut for the carry across workgroups (pgps_kernels.hip.h): set by the launch code where a
                            // workgroup spans >= 2048 steps and pgps_set_shortcut has not turned it off
    int dform;              // lsuf / sspine hold smoothing totals in innovation form (pgps_math.h smth_extend_u): the smoother adds the
                            // filtered moments of the step a total was applied at.  Whole-series pkfs of the lane-chunk kernels only
};

// record lengths (in elements of T) of the segment exchange
inline int seg_rec_f_len(int d) { return d * d + d + d * (d + 1) + d + 2 * d * d; }
inline int seg_rec_s_pad(int d) { int n = d * d + d + d * (d + 1) / 2; return n + (n & 1); }
inline int seg_rec_s_len(int d) { return seg_rec_s_pad(d) + 2; }

template <typename... KArgs, typename... Args>
inline void timed_launch(pgps_ctx* ctx, int slot, void (*kernel)(KArgs...), dim3 grid, dim3 block, unsigned shmem,
                         Args... args) {
    pgps_ctx::EvPair* ev = prof_acquire(ctx, slot);
    if (ev) hipExtLaunchKernelGGL(kernel, grid, block, shmem, ctx->stream, ev->a, ev->b, 0, KArgs(args)...);
    else hipLaunchKernelGGL(kernel, grid, block, shmem, ctx->stream, KArgs(args)...);
}

template <typename T>
struct GpModel {
    double lam;             // F = -lam I + N
    double N1[9];           // N            (d x d, row-major, d <= 3)
    double N2[9];           // N^2 / 2      (zero for d <= 2)
    double Pinf[9];         // stationary covariance = P0
    T H[3];
    const T* ts;            // (N,) time stamps                     [device]
    T t_prev;               // time before the first step (t0)
};

template <typename T>
struct GpArgs {
    ScanArgs<T> s;          // N, geometry, ys, R, outputs, scratch (Fs, Qs, P0, H unused)
    GpModel<T> m;
    // projected-posterior mode of the smoother (pgps_gp_predict_*): step k writes H sm_k and H sP_k H^T
    // to slot qslot[k] when that is >= 0 and nothing otherwise; sms / sPs are not written
    const int* qslot;       // (N,) or null                         [device]
    T* pmean;               // (K,)                                 [device]
    T* pvar;                // (K,)                                 [device]
};

template <typename T, int D>
int launch_gp(pgps_ctx* ctx, GpArgs<T> g, int want_filtered, int want_smoothed);

// filter + log-likelihood + smoother of a whole series in one resident launch (pgps_resident.hip.h, pgps_res_inst.hip)
template <typename T>
struct ResArgs {
    ScanArgs<T> s;          // N, nblocks, model, series, outputs, spine / sspine / llpart, status, ll
    GpModel<T> m;           // fused form: the Matern model (F = -lam I + N) and the time stamps
    int* bar;               // this launch's barrier 1: 8 counter shards (32 ints apart) of first arrivals, zero on entry
    int* bar2;              // ... barrier 2: 8 shards of second arrivals (bar + kResBarSet / 2)
    int* bar_next;          // the next launch's set (both barriers): zeroed by this one
    unsigned long long* gran1;      // per workgroup: its filtering total as tagged granules (the neighbour hand-off and the general fold)
    unsigned long long* gran2;      // ... its smoothing total (its log-likelihood partial follows, before its arrival at bar2)
    int epoch;              // this launch's (never 0): the tag of every granule it publishes
    long long* stamps;      // diagnostics (pgps_set_resident(ctx, 2)): (nblocks, 16) cycle stamps, else null
    // diagnostics (pgps_debug_resident_delay): start skew.  Workgroup `delay_tile` (-1: none) waits `delay_ticks` wall-clock
    // ticks before it publishes its phase-`delay_phase` total; wstamps (null unless armed) = the stamps buffer, whose slots
    // 10 .. 13 then take wall-clock stamps (pgps.h)
    int delay_tile;
    int delay_phase;
    long long delay_ticks;
    long long* wstamps;
};
constexpr int kResLc = 16;                  // steps per lane: the chunk lives in registers
constexpr int kStatusBytes = 8192;          // the context's status buffer: word 0 flags, 16.. tickets, 512.. the resident kernel's barrier counters
constexpr int kResBarWord = 512;            // two sets (alternating launches) of two barriers x 8 shards x 32 ints (words 512 .. 1535)
constexpr int kResBarSet = 2 * 8 * 32;
constexpr int kResMaxBlocks = 256;          // workgroups of one resident launch: the hand-off records, one record per lane in the general fold
static_assert((kResBarWord + 2 * kResBarSet) * 4 <= kStatusBytes, "barrier counters outside the status buffer");
// A hand-off record: one 8-byte granule {low word: 32 bits of the total, high word: the launch's epoch} per 32-bit word of the
// total, each written by ONE 8-byte store, the record padded to whole 128-byte lines.  The largest record (the filtering total
// at d = 2 in fp64: 14 doubles = 28 granules) fits kResGranStride bytes; the context owns two arrays of kResMaxBlocks records
// (filtering, smoothing totals), outside the growable workspace and zeroed once: no tag ever equals a later epoch.
constexpr int kResGranStride = 256;
constexpr size_t kResGranBytes = 2 * (size_t)kResMaxBlocks * kResGranStride;
// does a whole-series filter + smoother call of N steps at dimension d (fp64 when !f32) take the resident launch?
bool resident_fits(const pgps_ctx* ctx, long N, int d, bool f32);
template <typename T, int D>
int launch_resident(pgps_ctx* ctx, ResArgs<T> ra, bool fused, bool smooth);
// log-likelihood and the model's adjoints on the fused path (pgps_gpadj.hip.h), fp64, d <= 3: out = 1 + d^2 + 2 d + 1 doubles [device]
// (T names the unit that holds the instantiation: call it with T = double)
template <typename T, int D>
int launch_gp_adj(pgps_ctx* ctx, GpArgs<double> g, double* out);

template <typename T>
struct GpBatchArgs {
    long N;
    int Lc, nblocks;
    long nlanes;
    const T* ts;
    const T* ys;
    T t_prev;
    const double* models;       // (B, kGpModelStride): lam | N1[9] | N2[9] | Pinf[9] | H[3] | R
    T* spine;                   // (B, nblocks, NFILT)
    T* lpre;                    // (B, NFILT, nlanes)
    double* llpart;             // (B, nblocks)
    double* ll;                 // (B,)
    // predict (pgps_gp_predict_batch_*; all null / 0 in the log-likelihood call): N counts the merged steps
    T* fms;                     // (B, bs_fm) filtered means of the merged steps, one slice per model
    T* fPs;                     // (B, bs_fP) filtered covariances
    long bs_fm, bs_fP;          // slice strides in elements (>= N d, N d^2; rounded so that every slice starts 256-byte aligned)
    T* sspine;                  // (B, nblocks, NSMTH)
    T* lsuf;                    // (B, NSMTH, nlanes)
    const int* qslot;           // (N,) slot of a query step in a model's output row, -1 at the training steps (shared)
    T* pmean;                   // (B, K)
    T* pvar;                    // (B, K)
    long K;
};
constexpr int kGpModelStride = 32;

template <typename T, int D>
int launch_gp_batch(pgps_ctx* ctx, int B, GpBatchArgs<T> b);
// predict_f of B models over one merged series (b.N merged steps, b.qslot, b.K, b.models, b.pmean, b.pvar, b.ll set by the
// caller): picks the form and the geometry once from (B, N), carves the scratch and runs the models in groups that fit the
// context's batch budget
template <typename T, int D>
int launch_gp_predict_batch(pgps_ctx* ctx, int B, GpBatchArgs<T> b);
// log-likelihood and the model's adjoints of B models over one series (pgps_gpadj.hip.h), fp64, d <= 3: b.N, b.ts, b.ys, b.t_prev,
// b.models set by the caller; out (B, 1 + d^2 + 2 d + 1) [device].  Geometry once per call from (B, N); the models run in groups
// that fit the context's batch budget (T names the unit that holds the instantiation: call it with T = double)
template <typename T, int D>
int launch_gp_adj_batch(pgps_ctx* ctx, int B, GpBatchArgs<double> b, double* out);
// form 1 of the batched fused predict (one workgroup per model, pgps_set_batch_form(ctx, 1)) is taken up to this many merged steps
constexpr long kBatchOneMax = 65536;

// M observation columns on one clock (pgps_multi.hip.h, pgps_multi_inst.hip): fp64, d <= 3.  One launch covers the column
// groups [c_base, c_base + MC * gridDim.y); every group has its own slices of the scan scratch and of fms
struct GpMultiArgs {
    long N;                     // steps (merged steps in a predict call)
    int M;                      // columns of ys, of pmean, entries of ll
    int c_base;                 // first column of this launch
    int Lc, nblocks;
    long nlanes;
    GpModel<double> m;          // the model and the (merged) times
    double R;
    const double* ys;           // (rows, M) row-major, NaN = missing: a row is missing in all columns or in none
    const double* rows;         // (N,) the row of ys a step reads, as a double; NaN at a query step.  nullptr: step k reads row k
    const int* qslot;           // (N,) slot of a query step in pmean / pvar, -1 at the training steps (predict only)
    int ys_aligned, mean_aligned;       // ys / pmean start on a 16-byte boundary
    double* spine;              // (groups, nblocks, NFILT_M)
    double* lpre;               // (groups, NFILT_M, nlanes)
    double* sspine;             // (groups, nblocks, NSMTH_M)
    double* lsuf;               // (groups, NSMTH_M, nlanes)
    double* llpart;             // (M, nblocks): all columns of the call
    double* fms;                // (N, ldm, d) filtered means of this launch's columns
    double* fPs;                // (N, d (d + 1) / 2) filtered covariances, packed upper triangles: written once per launch
    int ldm;                    // columns of fms = MC * groups of a launch
    double* pmean;              // (K, M)
    double* pvar;               // (K,)
};
// steps per lane of the batched fused launches, and the geometry of both multi-output launches by it (pgps_ctx.hip)
int batch_steps_per_lane(const pgps_ctx* ctx, int B, long N);
void multi_geometry(const pgps_ctx* ctx, long N, int groups_all, int* Lc, int* nblocks);
// ll (M,) [device] or null; predict != 0: a.rows, a.qslot, a.pmean, a.pvar set.  Picks the geometry once per call from
// (M, N), carves the scratch and runs the column groups in rounds that fit the context's batch budget
template <int D>
int launch_gp_multi(pgps_ctx* ctx, GpMultiArgs a, int predict, double* ll);
// log-likelihoods and the model's adjoints summed over the columns (pgps_multi_grad.hip.h, pgps_multi_grad_inst.hip): a.N, a.M,
// a.m, a.R, a.ys set by the caller (training steps only); out (M + d^2 + 2 d + 1) [device] = [ll (M) | Abar | Ubar | Hbar | Rbar].
// Geometry and rounds as launch_gp_multi
template <int D>
int launch_gp_multi_grad(pgps_ctx* ctx, GpMultiArgs a, double* out);
// whitened columns and their Gram matrix (pgps_whiten.hip.h, pgps_whiten_inst.hip): what the whitening flavour of the Kalman
// pass writes besides the scan scratch
struct GpWhitenOut {
    double* w;                  // (N, ldw) row-major standardised innovations, 0.0 at the steps that are not observed
    long ldw;
    int w_aligned;              // w starts on a 16-byte boundary
    double* ldpart;             // (2, nblocks): every workgroup's sum of log S_k and its count of observed steps
};
constexpr int kGramMax = 16;            // columns of the Gram kernels
constexpr int kGramSlab = 1024;         // rows of W per workgroup of k_gram_partial
constexpr int kPanelGramMax = 8;        // columns of the panel's Gram kernel (pgps_panel_gram.hip.h)
// a.N, a.M, a.m, a.R, a.ys set by the caller (training steps only); logdet, n_obs [device].  w (N, M) [device]: the whitened
// columns are stored there; w null: they stay in scratch and gram (M, M) [device], M <= kGramMax, is formed from them.
// Geometry and rounds as launch_gp_multi
template <int D>
int launch_gp_whiten(pgps_ctx* ctx, GpMultiArgs a, double* w, double* gram, double* logdet, long* n_obs);

// merge of two sorted time arrays on the device + NaN marking of the query rows (pgps_core.hip)
template <typename T>
int launch_merge(pgps_ctx* ctx, long N, long K, const T* ts, const T* ys, const T* tq, T* ts_m, T* ys_m, int* qslot);

// ... with a second payload, rs -> rs_m (per-observation noise variances, NaN at the query rows)
int launch_merge_het(pgps_ctx* ctx, long N, long K, const double* ts, const double* ys, const double* rs, const double* tq,
                     double* ts_m, double* ys_m, double* rs_m, int* qslot);

// per-observation noise variances on the fused path (pgps_het_inst.hip; fp64, d <= 3, three-launch forms): step k is observed
// with variance g.s.R + rs[k].  launch_gp_het: the log-likelihood (g.qslot null, g.s.ll set) or predict_f over a merged
// series (g.qslot, g.pmean, g.pvar, g.s.fms, g.s.fPs set); launch_gp_adj_het: out = [ll | Abar | Ubar | Hbar | Rbar] [device]
template <int D>
int launch_gp_het(pgps_ctx* ctx, GpArgs<double> g, const double* rs);
template <int D>
int launch_gp_adj_het(pgps_ctx* ctx, GpArgs<double> g, const double* rs, double* out);

// S independent series, each on its own clock and of its own length, in one launch per group (pgps_panel.hip.h,
// pgps_panel_inst.hip; fp64, d <= 3).  One record per series, in device memory:
struct PanelDesc {
    long row0;              // first row in the concatenated ts / ys / rs
    long q0;                // first query in tq / mean / var
    long m0;                // first row of its merged slot in ts_m / ys_m / rs_m / qslot (a multiple of kPanelAlign)
    long o_fm, o_fP;        // element offsets of its fms / fPs slices in its group's scratch (multiples of kPanelAlign)
    long o_xs;              // ... of its kept states, ((d + sym) Lc, kBlock)
    int n;                  // length
    int k;                  // queries (0 in the likelihood and gradient calls)
    int m;                  // merged length n + k
    int Lc;                 // steps per lane, from m and the pinned chunk alone
    int slot;               // its place in its group: the fixed-size records (lpre, lsuf, spine, sspine, llpart, gpart) of a
                            // series lie at slot * record length
    int model;              // its row of the model table
};
// Alignment of a panel's ragged slices, in ELEMENTS (doubles: 256 bytes; the int qslot: 128 bytes).
//   merged slots   k_panel_merge stores four outputs per lane as 16-byte vectors (merge_sorted_body): it relies on outputs that
//                  start 16-byte aligned.  Ragged series' slots would start anywhere: every slot is padded to kPanelAlign.
//   fms / fPs      the staged stores of gp_apply_body and the staged loads of gp_smooth_body go through GpLds::stage in 16-byte
//                  pieces from the slice's base: every series' slice starts on a multiple of kPanelAlign.
constexpr int kPanelAlign = 32;
// what one launch (one group of series: series blockIdx.y of the launch) sees
struct PanelArgs {
    const PanelDesc* desc;      // the group's records
    const double* models;       // (nmodels, kGpModelStride) rows [lam | N1 | N2 | Pinf | H | R]
    const double *ts, *ys, *rs; // concatenated training series (rs: null = scalar noise)
    const double* tq;           // concatenated queries
    double *ts_m, *ys_m, *rs_m; // merged slots of the group's series that have queries
    int* qslot;                 // ... a query row's GLOBAL position in pmean / pvar, -1 at the training rows
    double *pmean, *pvar;       // (all queries of the call,)
    double* ll;                 // (the group's series,)
    double* out;                // (the group's series, 1 + d^2 + 2 d + 1): gradient rows
    double *spine, *lpre, *sspine, *lsuf, *llpart, *fms, *fPs, *xs, *gpart;     // the group's scratch
    int* status;
};
// a call as the C ABI hands it over: offs / qoffs / models HOST, everything else device
struct PanelCall {
    long S;
    const long* offs;           // (S + 1)
    const long* qoffs;          // (S + 1), predict only
    int nmodels;                // 1 or S
    const double* models;       // (nmodels, kGpModelStride)
    const double *ts, *ys, *rs, *tq;
    double *mean, *var;         // predict
    double* ll;                 // (S,)
    double* out;                // gradient: (S, 1 + d^2 + 2 d + 1)
    double *osa_mean, *osa_var, *loo_mean, *loo_var;    // predictive checks: (offs[S],) each, or null
    double* sums;               // predictive checks: (S, 2) {ll, loo_lpd}
};
enum PanelWhat { PANEL_LL = 0, PANEL_GRAD = 1, PANEL_PREDICT = 2, PANEL_LOO = 3 };
// lays the series out in groups that fit the context's batch budget, copies the two tables in (ONE stream synchronisation),
// then merge (predict) and one launch per group.  The caller has checked the arguments
template <int D>
int launch_gp_panel(pgps_ctx* ctx, const PanelCall& c, PanelWhat what);
// the segmented merge of one group (the d = 1 unit holds it): grid (tiles, series)
int launch_panel_merge(pgps_ctx* ctx, const PanelArgs& p, unsigned tiles, unsigned series);
// The whitened Gram matrix of C columns of every series (pgps_panel_gram.hip.h, pgps_panel_gram_inst.hip).
// offs / models HOST as in PanelCall, everything else device: V (offs[S], C) row-major, out (S, C C + 2) records
// [G | logdet | n_obs].  Groups, tables and the one synchronisation as launch_gp_panel.  The caller has checked the arguments
struct PanelGramCall {
    long S;
    const long* offs;
    int nmodels;
    const double* models;       // (nmodels, kGpModelStride)
    int C;
    const double *ts, *V, *rs;
    double* out;
};
template <int D>
int launch_gp_panel_gram(pgps_ctx* ctx, const PanelGramCall& c);
// ys_out[k] = V[k, 0] - sum_j V[k, 1 + j] betas[s, j] over the rows of every series (the d = 1 unit holds it); offs HOST
int launch_panel_residual(pgps_ctx* ctx, long S, const long* offs, int C, const double* V, const double* betas, double* ys_out);

// predictive checks of a fitted model against its own data on the fused path (pgps_loo_inst.hip; fp64, d <= 3):
// what the OSA flavour of the Kalman pass and the LOO flavour of the smoother write
template <typename T>
struct GpLooOut {
    T* osa_mean;            // (N,) H m_k^-: mean of y_k given the observations before it                [device], or null
    T* osa_var;             // (N,) H P_k^- H^T + R: its variance                                        [device], or null
    T* loo_mean;            // (N,) mean of y_k given all other observations                             [device], or null
    T* loo_var;             // (N,) its variance (noise included)                                        [device], or null
    double* lpd_part;       // (nblocks,) workgroup sums of log N(y_k | loo_mean, loo_var), observed steps [scratch: set by the launch]
};
// reduce / Kalman pass (OSA) / smoother (LOO) / finalize over g (g.s.fms, g.s.fPs set: the filtered moments the smoother
// reads); sums[2] = {log-likelihood, sum of the leave-one-out log densities over the observed steps} [device]
template <int D>
int launch_gp_loo(pgps_ctx* ctx, GpArgs<double> g, GpLooOut<double> o, double* sums);

// One Newton step of a Laplace approximation on the fused path (pgps_site_inst.hip; fp64, d <= 3): what the SITE
// flavour of the smoother reads besides the sites' means (g.s.ys) and writes.  All arrays (N,) [device]
template <typename T>
struct GpSiteOut {
    int lik;                // PGPS_LIK_*
    double par;             // its parameter
    const T* ys;            // the observations, NaN = missing (g.s.ys holds the sites' means zs, NaN at the same rows)
    const T* ss;            // the sites' variances of this pass
    const T* f_prev;        // the iterate the sites were formed at, or null
    T* f_out;               // smoothed mean of f_k = H x_k: the new iterate
    T* v_out;               // its smoothed variance
    T* alpha_out;           // (zs - f_out) / ss, 0 at the missing rows
    T* zs_out;              // the sites formed at f_out: means (NaN at the missing rows) ...
    T* ss_out;              // ... and variances (1 at the missing rows)
    double* part;           // (kSiteParts, nblocks) workgroup partials                                    [scratch: set by the launch]
};
constexpr int kSiteParts = 5;       // sum lp | sum f alpha | sum [lp - log N(z | f, s)] | max |f - f_prev| | observed steps
// reduce / Kalman pass (both of the per-observation-noise flavour, on (g.s.ys, o.ss) with g.s.R = 0) / smoother (SITE) /
// finalize; g.s.fms, g.s.fPs set; sums[6] [device] as pgps_gp_newton_dev_f64 documents them
template <int D>
int launch_gp_newton(pgps_ctx* ctx, GpArgs<double> g, GpSiteOut<double> o, double* sums);
// the sites at f = f_a + step (f_b - f_a) (f_b null: f_a), elementwise, and sums[3] [device] (pgps_site_inst.hip, the d = 1 unit)
struct LikSitesArgs {
    long N;
    int lik;
    double par;
    const double *ys, *f_a, *alpha_a, *f_b, *alpha_b;
    double step;
    double *f_out, *alpha_out, *zs_out, *ss_out;
    double* part;           // (3, nblocks) workgroup partials                                             [scratch: set by the launch]
    int nblocks;
};
int launch_lik_sites(pgps_ctx* ctx, LikSitesArgs a, double* sums);

// log-likelihood + gradient on the fused path (pgps_grad.hip); all array pointers device
int launch_grad(pgps_ctx* ctx, long N, int d, int np, const double* model, const double* ts, double t0,
                const double* ys, double* out_dev);

// the same for block-nilpotent composite models (sums / products of Matern kernels), d = 2..6 (pgps_gradb.hip, one
// instantiation per d): model rows [lam (4) | N (d*d) | Pinf (d*d) | H (d) | R], bsize = the nblk block sizes
template <int D>
int launch_gradb(pgps_ctx* ctx, long N, int nblk, const int* bsize, int np, const double* model, const double* ts, double t0,
                 const double* ys, double* out_dev);

enum Mode { MODE_PKF, MODE_PKS, MODE_PKFS, MODE_SEG_REDUCE, MODE_SEG_FILTER, MODE_SEG_SMOOTHER };

// Joint posterior draws by backward sampling (pgps_sample.hip.h): one (dtype, d) unit per
// 1 <= d <= PGPS_MAX_DIM_LANE (pgps_sample_inst.hip).  Sample s (0 <= s < S) uses the draws of global index s0 + s.
template <typename T>
struct SampleArgs {
    long N;
    const T* Fs;
    const T* Qs;
    const T* fms;
    const T* fPs;
    int S;
    long s0;
    unsigned long long seed;
    const T* z;             // (S, N, d) standard normals of the caller, or nullptr = the library's (pgps_philox.h)
    int proj;               // 1: write H x_k (h below), 0: the states
    T h[PGPS_MAX_DIM_LANE];
    T* out;                 // sample s, column c: out[(s * out_rows + c) * (proj ? 1 : d)]
    long out_rows;
    const int* qslot;       // nullptr: column = step; else the column of step k is qslot[k], none where < 0
    // launch geometry and workspace (filled by launch_sample)
    int Lc, nblocks, ngroups;
    long nlanes;
    T* lsuf;                // (ngroups, NREC, nlanes) field-major
    T* spine;               // (ngroups, nblocks, NREC)
};
template <typename T, int D>
int launch_sample(pgps_ctx* ctx, SampleArgs<T> a);
// z (S, N, d) = the library's draws of samples s0 .. s0 + S - 1 (any d)
template <typename T>
int launch_sample_normals(pgps_ctx* ctx, long N, int d, int S, long s0, unsigned long long seed, T* z);

// Joint posterior covariance between selected steps (pgps_cov.hip.h): one (dtype, d) unit per
// 1 <= d <= PGPS_MAX_DIM_LANE (pgps_cov_inst.hip).
template <typename T>
struct CovArgs {            // the gain products B_a = E_{sel[a]} .. E_{sel[a+1]-1}: a segmented scan over the N steps
    long N;
    const T* Fs;
    const T* Qs;
    const T* fPs;
    const int* slot;        // (N,) position of step k in the selection, < 0 where it is not selected (k_merge_sorted's qslot)
    long n;                 // selected steps
    T* B;                   // (n - 1, d, d)
    // launch geometry and workspace (filled by launch_cov_gains)
    int Lc, nblocks;
    long nlanes;
    T* lsuf;                // (NREC, nlanes) field-major lane suffixes
    T* spine;               // (nblocks, NREC)
};
constexpr int kCovTile = 64;    // rows of a fill tile = lanes of the wave that fills it
template <typename T>
struct CovFillArgs {        // out[a, b] = B_a .. B_{b-1} sP_b (a <= b), mirrored below the diagonal
    long n;
    const T* B;             // (n - 1, d, d)
    const T* sP;            // (n, d, d) smoothed covariances of the selected steps
    int proj;               // 1: out (n, n) = h^T Cov h, 0: out (n, n, d, d)
    T h[PGPS_MAX_DIM_LANE];
    T* out;
    // workspace (filled by launch_cov_fill)
    int nt;                 // row tiles, ceil(n / kCovTile)
    T* U;                   // (n, d, d) U_j = B_{tT-1} .. B_{j-1}, t = j / T: carries column j to the row above its tile
    T* M;                   // (nt, nt, d, d) M[s][t] = U_{(s+2)T-1} .. U_{tT-1}: from above tile t to the top row of tile s
};
template <typename T, int D>
int launch_cov_gains(pgps_ctx* ctx, CovArgs<T> a);
template <typename T, int D>
int launch_cov_fill(pgps_ctx* ctx, CovFillArgs<T> a);

// defined in pgps_inst.hip, one explicit instantiation per compiled (T, D)
template <typename T, int D>
int launch_scan(pgps_ctx* ctx, ScanArgs<T> a, Mode mode);
// the same scan built a second time with 128-lane workgroups (pgps_inst.hip with -DPGPS_NARROW -DPGPS_BLOCK=128)
template <typename T, int D>
int launch_scan_narrow(pgps_ctx* ctx, ScanArgs<T> a, Mode mode);
constexpr int kBlockNarrow = 128;
void geometry_narrow(const pgps_ctx* ctx, long N, int* Lc, int* nblocks, int d);      // pgps_core.hip
// wave-cooperative family (pgps_wc.hip): runtime state dimension, 1 <= d <= 32
template <typename T>
int launch_scan_wc(pgps_ctx* ctx, ScanArgs<T> a, int d, Mode mode);
// row-cooperative family (pgps_rc.hip.h): fp64 and fp32, 2 <= d <= 16
template <typename Real>
int launch_scan_rc(pgps_ctx* ctx, ScanArgs<Real> a, int d, Mode mode);
// the same with nothing written per step: MODE_PKF = log-likelihood only; MODE_PKFS = H sm, H sP H^T at the steps
// qslot marks (a.sPs / a.sms are then scratch of N d^2 / N d doubles for the smoothing elements)
// (MODE_PKF with a.Qs == nullptr: implicit process noise Q_k = P0 - F_k P0 F_k^T, P0 must be stationary)
// nfun > 0 (MODE_PKFS): the functionals flavour -- pmean (K, nfun) = C sm, pcov (K, nfun, nfun) = C sP C^T for C (nfun, d)
// [device], pvar unused; same chain length as the plain projection
int launch_scan_rc_proj(pgps_ctx* ctx, ScanArgs<double> a, int d, Mode mode, const int* qslot, double* pmean,
                        double* pvar, int nfun = 0, const double* C = nullptr, double* pcov = nullptr);
int launch_disc_rc(pgps_ctx* ctx, long N, int d, const double* F, const double* Pinf, const double* ts, double t0,
                   double* Fs, double* Qs, int batch = 1, long bs_model = 0);
// log-likelihoods of `batch` models over one series: table = batch x [F | Pinf | H | R] (stride bs_model, device),
// Fs / Qs = (batch, N, d, d) discretised arrays, ll = (batch,) device
int launch_ll_batch_rc(pgps_ctx* ctx, long N, int d, int batch, const double* table, long bs_model, const double* Fs,
                       const double* Qs, const double* ys, double* ll);
// predict_f of `batch` models over one MERGED series of N steps (qslot marks the K query rows): table / Fs as above, Es / gs
// = (batch, N, d, d) / (batch, N, d) scratch for the smoothing elements, pmean / pvar (batch, K), ll (batch,), all device.
// geom_batch (>= batch) = the models of the whole call: the chain length is fixed from it, so a group's results do not
// depend on how the call was split
int launch_predict_batch_rc(pgps_ctx* ctx, long N, long K, int d, int batch, int geom_batch, const double* table, long bs_model,
                            const double* Fs, const double* ys, const int* qslot, double* Es, double* gs, double* pmean,
                            double* pvar, double* ll);
namespace rc {
constexpr int kDimMin = 2, kDimMax = 16;
constexpr int kScanBlockedDimMax = 15;     // blocked scans of the chain totals: the dimensions whose kernels need no scratch
template <typename Real>
struct RcArgsT {
    long N;
    int Lw;                     // steps per chain
    long nchunk;                // chains
    long wfast;                 // waves [1, wfast) lie inside the series, halo step included: predicate-free body
    const Real *P0, *H;
    Real R;
    const Real *Fs, *Qs, *ys;
    Real *fms, *fPs, *sms, *sPs;
    Real* agg1;               // (nchunk, nfilt) chunk totals
    const Real* pre;          // (nchunk, nfilt) inclusive prefixes of agg1
    Real* sagg1;              // (nchunk, nsmth) smoothing totals
    const Real* suf;          // (nchunk, nsmth) inclusive suffixes of sagg1
    Real *Es, *gs;            // (N, d, d), (N, d) the smoothing elements' E and g: sPs / sms themselves (overwritten
                                // in place by the smoother) unless those are not there yet (segments, projections)
    Real* Lws;                // (N, d, d) the smoothing elements' L
    double* llpart;             // (nchunk,)
    int seg_first, seg_last;    // this launch covers the first / last step of the whole series (multi-GPU segments)
    const Real* carry;        // !seg_first: compact filter record of everything before the segment
    const Real *halo_F, *halo_Q;  // !seg_last: F, Q of the first step of the next segment
    const Real* carry_back;   // !seg_last: compact smoother record of everything after the segment
    int batch;                  // models evaluated over the same series (blockIdx.y); 0 / 1 = one
    long bs_F, bs_agg, bs_model;    // per-model strides of Fs / Qs, of agg1 / pre, of the model table
    long bs_sagg, bs_g, bs_out;     // batched predict (0 otherwise): per-model strides of sagg1 / suf, of gs (Es / Lws: bs_F), of pmean / pvar
    const Real* Rs;           // batch entry point: observation noise of model b at Rs[b * bs_model] (else null)
    int implicit_q;             // Qs is not there: Q_k = P0 - F_k P0 F_k^T is folded into the predict (P0 stationary)
    int store_f;                // write fms / fPs (0: log-likelihood-only and projected-posterior calls)
    const int* qslot;           // projected-posterior mode: (N,) slot of step k in pmean / pvar, or -1
    Real *pmean, *pvar;       // (K,) H sm and H sP H^T at the query steps
    int dform;                  // the chains' smoothing totals are in innovation form (rc_apply1 DFORM): rc_smooth1 adds the filtered moments
    int quad;                   // level-1 kernels of the quad-cooperative family (pgps_qc.hip.h: fp32, 5 <= d <= 8, 16 chains per wave)
    // functionals flavour of the projected-posterior mode (pgps_lti_predict_lin_*, fp64; nfun = 0 otherwise): pmean (K, nfun)
    // = C sm, pcov (K, nfun, nfun) = C sP C^T at the query steps; pvar is not written
    int nfun;                   // rows of C, 1 .. PGPS_MAX_FUNCTIONALS
    const Real* C;              // (nfun, d)
    Real* pcov;
};
using RcArgs = RcArgsT<double>;
// defined in pgps_rc_inst.hip, one explicit instantiation per (scalar type, d)
template <typename Real, int D>
int launch_rc_level1(pgps_ctx* ctx, const RcArgsT<Real>& a, int phase);
template <typename Real, int D>
int launch_rc_ks(pgps_ctx* ctx, int which, long n, long stride, const Real* in, Real* out, int batch, long bstride,
                 const Real* fixed);
template <typename Real, int D>
int launch_rc_scan_blocked(pgps_ctx* ctx, int which, long n, Real* data, Real* scratch);
template <typename Real, int D>
int launch_rc_seg_carry(pgps_ctx* ctx, int which, const Real* gathered, int rank, int nranks, int reclen, Real* out);
template <int D>
int launch_rc_disc(pgps_ctx* ctx, long N, const double* F, const double* Pinf, const double* ts, double t0, double* Fs,
                   double* Qs, int batch, long bs_model);
}  // namespace rc
// quad-cooperative level-1 kernels (pgps_qc.hip.h): fp32, 5 <= d <= 8; they speak the row-cooperative protocol
namespace qc {
constexpr int kDimMin = 5, kDimMax = 8;
template <int D>
int launch_qc_level1(pgps_ctx* ctx, const rc::RcArgsT<float>& a, int phase);
}  // namespace qc
template <typename T>
int launch_disc_wc(pgps_ctx* ctx, long N, int d, const T* F, const T* Pinf, const T* ts, T t0, T* Fs, T* Qs);

template <typename T, int D>
int launch_disc(pgps_ctx* ctx, long N, const T* F, const T* Pinf, const T* ts, T t0, T* Fs, T* Qs);

}  // namespace pgps
