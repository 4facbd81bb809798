/* pgps.h -- C ABI of libpgps.so: the parallel Kalman filter / RTS smoother scan of
 * EEA-sensors/parallel-gps (`pssgp`) as hand-written HIP kernels for MI355X (gfx950).
 *
 * The reference has no native boundary (it is pure Python on TensorFlow); the boundary it
 * does have is the Python signature of the functions below, so every entry point names the
 * reference function whose arguments and results it carries (paths relative to the
 * reference checkout).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - plain pointers and sizes only; row-major, time-major arrays: Fs[k][i][j].
 *   - `_f64` / `_f32` = the dtype every array of that call has (ll is always double).
 *   - host entry points take HOST pointers: the library stages to the device, runs, copies
 *     back and returns when the results are in the caller's buffers.
 *   - `_dev` entry points take DEVICE pointers (16-byte aligned) and are asynchronous on the
 *     context's stream (pgps_set_stream / pgps_synchronize).
 *   - the caller owns every buffer; the library owns only the context (stream, scratch).
 *   - return value 0 = PGPS_OK, negative = error (pgps_strerror); nothing throws across the
 *     ABI; outputs are undefined after an error.
 *   - one call in flight per context; contexts are independent (one per GPU / per thread).
 *   - state dimension d: 1..PGPS_MAX_DIM_LANE use the lane-chunk kernels (one lane owns whole d x d operands), fp64
 *     series with 5 <= d <= 16 and fp32 series with 7 <= d <= 16 the row-cooperative ones (built natively in both
 *     precisions for 2 <= d <= 16), fp32 series at d = 8 -- and at d = 6 away from 2^19 .. 2^20 steps -- the
 *     quad-cooperative level-1 kernels under the row-cooperative driver, up to PGPS_MAX_DIM the wave-cooperative ones
 *     (from d = 17 on with the two-rows level-1 kernels: a chain on two DPP rows, the products in registers);
 *     pgps_set_family overrides.
 *     Every call takes every d <= PGPS_MAX_DIM, the segment calls (pgps_seg_*, pgps_pkfs_seg_*) included.
 *   - NaN in `ys` marks a missing observation (parallel.py:42,86-95).
 */
#ifndef PGPS_H_
#define PGPS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGPS_OK 0
#define PGPS_E_INVALID (-1)         /* bad argument (null pointer, N < 1, misaligned device pointer) */
#define PGPS_E_UNSUPPORTED_DIM (-2) /* state dimension outside the compiled kernels */
#define PGPS_E_HIP (-3)             /* a HIP runtime call failed (pgps_last_hip_error) */
#define PGPS_E_NOMEM (-4)           /* device or host allocation failed */
#define PGPS_E_NUMERIC (-5)         /* non-finite result (reference: TF raises on CPU, NaNs on GPU) */
#define PGPS_E_NO_DEVICE (-6)       /* no HIP device visible */
#define PGPS_E_COMM (-7)            /* an RCCL call failed (pgps_last_hip_error carries RCCL's message) */

#define PGPS_MAX_DIM_LANE 6   /* lane-chunk kernels: one lane holds whole d x d operands */
#define PGPS_MAX_DIM 32       /* wave-cooperative kernels: operands in LDS, 64 lanes share each operation (levels 2, 3);
                                 level 1 from d = 17: two-rows kernels, a row of every operand per lane */

typedef struct pgps_ctx pgps_ctx;

/* ---- library / context ---------------------------------------------------------------- */
int pgps_version(void);
const char* pgps_strerror(int code);
int pgps_device_count(int* n);
/* Create a context on HIP device `device` (own non-blocking stream + scratch). */
int pgps_create(int device, pgps_ctx** out);
int pgps_destroy(pgps_ctx* ctx);
/* Launch on an external hipStream_t (e.g. the caller's framework stream).  NULL is the HIP null
 * (default) stream, exactly as in HIP; pgps_use_own_stream goes back to the context's own
 * non-blocking stream (the state after pgps_create). */
int pgps_set_stream(pgps_ctx* ctx, void* hip_stream);
int pgps_use_own_stream(pgps_ctx* ctx);
int pgps_synchronize(pgps_ctx* ctx);
/* Steps per lane of the scan kernels; 0 = automatic. */
int pgps_set_chunk(pgps_ctx* ctx, int steps_per_lane);
/* Single-pass filter kernel (d <= 2, 16 steps per lane, whole series on one GPU): mode -1 = automatic,
 * 0 = off (three-launch reduce-then-scan), 1 = on; window = tiles per look-back window (1..256, 0 = keep). */
int pgps_set_single_pass(pgps_ctx* ctx, int mode, int window);
/* Filter + log-likelihood + smoother of a whole series in ONE resident launch (csrc/pgps_resident.hip.h): fp64, d = 2,
 * series of up to 4096 steps per compute unit (2^20 on MI355X); taken by pgps_pkfs_dev_f64 / pgps_pkfs_f64 and by
 * pgps_gp_dev_f64 / pgps_gp_f64, and -- in its filter-only form, without the smoothing phase -- by pgps_pkf_dev_f64 /
 * pgps_pkf_f64 and by pgps_gp_* calls that ask for no smoothed moments.  Fs, Qs, ys are read once and every output is
 * written once (the reference's pkf + pks contract, pssgp/kalman/parallel.py:121-201); the launch needs every workgroup
 * resident, so another stream's kernel holding compute units makes it give up (bounded spins) with bit 1 of
 * pgps_status set and undefined outputs.  A call made while the stream is being captured into a hipGraph takes the three
 * launches (the resident launch's barrier set and hand-off epoch are per-launch host state: a replay would reuse them).
 * Series of up to 2048 steps per compute unit run it with 8 steps per lane (twice the workgroups), longer ones with 16;
 * pgps_set_chunk(ctx, 8 or 16) under mode >= 1 pins that choice (any other pinned chunk selects the three launches).
 * mode -1 = automatic (from 2^17 steps), 0 = never (three launches),
 * 1 = wherever the series fits, 2 = as 1 with in-kernel phase stamps kept for pgps_resident_stamps (diagnostics). */
int pgps_set_resident(pgps_ctx* ctx, int mode);
/* The forgetting shortcut of the lane-chunk and resident kernels (csrc/pgps_kernels.hip.h): a workgroup whose neighbour's total
 * has |A| (smoother: |E|) <= 2^-120 (fp64) / 2^-60 (fp32) -- a filter that has forgotten what came before those thousands of
 * steps -- takes the neighbour's (b, C) ((g, L)) as its carry instead of folding every total on that side: same bits, ten
 * combine levels less.  Decided from the data per workgroup; 1 (default) = where a workgroup spans >= 2048 steps, 0 = never
 * (every carry by the general fold: what the tests compare it with). */
int pgps_set_shortcut(pgps_ctx* ctx, int on);
/* Diagnostics: cycle stamps of the last resident launch made under mode 2: out = (n_blocks, 16) long long (host), at most
 * max_blocks rows copied; out may be NULL to ask for n_blocks only. */
int pgps_resident_stamps(pgps_ctx* ctx, long long* out, int max_blocks, int* n_blocks);
/* Diagnostics: per-wave stamps of the same launch (mode 2): out = (n_blocks, 8) long long, entry k * 4 + wave = the cycle
 * count at which that wave ended its reduce (k = 0) / its Kalman pass (k = 1); slots 1 and 5 of pgps_resident_stamps are
 * wave 0's, after it has waited for the slower waves at a barrier. */
int pgps_resident_wave_stamps(pgps_ctx* ctx, long long* out, int max_blocks, int* n_blocks);
/* Diagnostics: a deterministic start skew for the resident launch's hand-offs (the tests' view of a shared GPU).  Armed
 * (tile 0..255), every following resident launch makes workgroup `tile` wait `microseconds` (0..10000) of the wall clock
 * before it publishes its phase-1 total (phase 1: the filtering total) or its phase-2 total (phase 2: the smoothing total
 * and log-likelihood partial); the launch's spine records are filled with NaN first, so a record read before it is
 * published shows.  pgps_resident_stamps then also returns wall-clock stamps (device wall clock, constant rate) in
 * slots 10 .. 13 of every row: 10 / 11 = that workgroup's phase-1 / phase-2 publish, 12 = the start of the armed
 * workgroup's wait, 13 = its length in wall-clock ticks (both in the armed workgroup's row); the cycle stamps of slots
 * 0 .. 9 only under pgps_set_resident(ctx, 2).  tile = -1 disarms it (the state after pgps_create). */
int pgps_debug_resident_delay(pgps_ctx* ctx, int tile, int phase, int microseconds);
/* Kernel family: 0 = automatic (lane-chunk for d <= 4 and for fp32 up to PGPS_MAX_DIM_LANE; row-cooperative for
 * fp64 with 5 <= d <= 16 and fp32 with 7 <= d <= 16, segments use it above d = 6; quad-cooperative for whole fp32
 * series at d = 8 and, up to 3 * 2^17 and from 3 * 2^19 steps, at d = 6; wave-cooperative otherwise, d <= 32),
 * 1 = lane-chunk (d <= PGPS_MAX_DIM_LANE), 2 = wave-cooperative, 3 = row-cooperative (fp64 and fp32, 2 <= d <= 16),
 * 4 = quad-cooperative level-1 kernels under the row-cooperative driver (fp32 only, 5 <= d <= 8; pkf / pkfs / segments:
 * outside that range, for fp64 and for pks a forced family 4 returns PGPS_E_UNSUPPORTED_DIM -- until round 3 it fell
 * back to the row-cooperative kernels there). */
int pgps_set_family(pgps_ctx* ctx, int family);
/* Lanes per workgroup of the lane-chunk kernels (d <= PGPS_MAX_DIM_LANE): 0 = automatic (128 -- half the scan tree per
 * step at the same number of workgroups -- except d <= 3 from 2^22 steps of this call / this rank's segment), 128, 256.
 * The library carries both builds; the fused (pgps_gp_*) kernels always use 256.  Do not change it between the phases
 * of a segment pass (refused).  pgps_get_chunk reports the geometry of the 256-lane build. */
int pgps_set_block(pgps_ctx* ctx, int lanes);
/* Kalman pass of the 128-lane lane-chunk kernels at d = 2, fp64 (16 or 32 steps per lane): inputs through a ring of
 * LDS-DMA slots (buffer_load ... lds) requested before the workgroup folds the spine, instead of register staging.
 * -1 = automatic (= off: measured slower at 2^20 steps, profiles/r03_experiments.txt), 0 = off, 1 = on (the ring takes
 * 128 KiB of LDS: one workgroup per CU). */
int pgps_set_dma(pgps_ctx* ctx, int mode);
/* Scans over the chain totals of the row- and quad-cooperative families: -1 = automatic (blocked from 64 chains: log2(B)
 * levels per launch through LDS, B <= 64 records per workgroup), 0 = one launch per Kogge-Stone level, 1 = blocked. */
int pgps_set_rc_scan(pgps_ctx* ctx, int mode);
/* Fused (pgps_gp_*) calls of short series -- the reference's own lengths, N = 200 .. 10^4 per evaluation
 * (pssgp/experiments/toy_models/mcmc.py:55) -- run as ONE workgroup in ONE launch (reduce, scan, Kalman pass, smoother,
 * projection) up to max_steps steps: -1 = automatic (2048: at 4096 + 1024 steps the three launches are ahead again), 0 = never,
 * n > 0 = up to n steps. */
int pgps_set_one_launch(pgps_ctx* ctx, int max_steps);
/* pgps_gp_ll_grad_* at d <= 2: series up to max_steps take ONE derivative direction per model, the directions side by side
 * in the same launches (a Dual<1> scan tree is less than half of a Dual<3> one, and for a short series the tree's latency
 * is the whole cost); longer ones carry all directions in one dual number (the primal arithmetic is shared).
 * -1 = automatic (2^18 steps), 0 = never.  d = 3 always runs one direction per model. */
int pgps_set_grad_pack(pgps_ctx* ctx, long max_steps);
/* What a lane-chunk call (or one rank's segment) of N steps at state dimension d <= PGPS_MAX_DIM_LANE runs with: lanes per
 * workgroup (128 / 256), steps per lane, workgroups -- after pgps_set_block / pgps_set_chunk. */
int pgps_get_geometry(pgps_ctx* ctx, long N, int d, int* lanes, int* steps_per_lane, int* workgroups);
/* (Diagnostic, environment: PGPS_WC_SERIAL3=1 when a context is created makes the wave-cooperative family walk its
 * group totals with one wave instead of the Kogge-Stone scan -- the cross-check of tests/test_gpu_wavecoop.py.
 * PGPS_WC_ROWS2=<mask> selects, per level-1 kernel of d >= 17, the two-rows kernels (bit set) or the LDS-tile kernels
 * they replaced: 1 reduce, 2 Kalman pass without and 4 with the smoothing total, 8 smoother; default 15, 0 = the
 * LDS-tile kernels throughout -- the cross-check of tests/test_gpu_tworows.py.  The Kogge-Stone levels of the filter scan
 * follow bit 1; PGPS_WC_KS2=0 keeps the LDS-tile level on its own.) */
/* LDS staging of the lane-chunk kernels: -1 = automatic, 0 = off (direct global accesses),
 * 2 or 4 = steps per lane per staged sub-tile (2: fp64 only).  Tuning / A-B knob. */
int pgps_set_stage(pgps_ctx* ctx, int steps_per_subtile);
int pgps_get_chunk(pgps_ctx* ctx, long n_steps, int* steps_per_lane, int* n_workgroups);
/* What the batched fused launches of B models over n_steps steps run with (pgps_gp_ll_batch_*, the three-launch form of
 * pgps_gp_predict_batch_* -- n_steps = N + K there -- and the four-launch road of pgps_gp_ll_grad_adj_batch_*): steps per
 * lane -- pgps_set_chunk's value, else 16 while B x workgroups >= 1024, halved towards 4 -- and the 256-lane workgroups per
 * model by it.  Read-only.  Errors: B < 1, n_steps < 1, a null pointer: PGPS_E_INVALID. */
int pgps_get_batch_chunk(pgps_ctx* ctx, int B, long n_steps, int* steps_per_lane, int* n_workgroups);
/* What a panel launch (pgps_gp_panel_*: one 256-lane workgroup per series) gives a series of m steps -- counted MERGED, n + k,
 * in predict: steps per lane -- the series' own, max(1, ceil(m / 256)), or pgps_set_chunk's value where it covers the series
 * (chunk x 256 >= m).  Read-only.  Errors: m < 1, m > PGPS_PANEL_MAX_STEPS, a null pointer: PGPS_E_INVALID. */
int pgps_get_panel_chunk(pgps_ctx* ctx, long m, int* steps_per_lane);
/* Which kernel family a pkf (what = 0) / pks (1) / pkfs (2) call -- or a phase of the segment protocol (3) -- of n_steps at
 * state dimension d will run on under the context's settings (float32 arithmetic if f32 != 0; a float32 smoother call that
 * is promoted to fp64 arithmetic, pgps_set_f32_policy, takes the fp64 answer): what a benchmark needs to name the kernels it
 * timed without repeating the library's dispatch rule. */
#define PGPS_FAMILY_LANE 1          /* lane-chunk kernels, 256-lane workgroups (d <= 6) */
#define PGPS_FAMILY_WAVE 2          /* wave-cooperative LDS-tile kernels (d <= 32) */
#define PGPS_FAMILY_ROW 3           /* row-cooperative kernels (2 <= d <= 16) */
#define PGPS_FAMILY_QUAD 4          /* quad-cooperative level-1 kernels under the row-cooperative driver (fp32, 5 <= d <= 8) */
#define PGPS_FAMILY_TWO_ROWS 5      /* two-rows level-1 kernels under the wave-cooperative driver (17 <= d <= 23 fp64, <= 31 fp32) */
#define PGPS_FAMILY_LANE_NARROW 11  /* lane-chunk kernels, 128-lane workgroups */
#define PGPS_FAMILY_RESIDENT 12     /* filter + smoother in one resident launch (pkfs, fp64, d = 2, up to 4096 steps per CU: pgps_set_resident) */
int pgps_get_family(pgps_ctx* ctx, long n_steps, int d, int f32, int what, int* family);
const char* pgps_last_hip_error(pgps_ctx* ctx);
/* Diagnostic flags raised since the last call (synchronises; 0 = none; bit 1: a bounded spin of the single-pass filter
 * or of the resident launch's grid barrier gave up -- results of that pass are invalid; PGPS_STATUS_F32_PROMOTED: a float32 call ran in fp64
 * arithmetic, see pgps_set_f32_policy). */
#define PGPS_STATUS_F32_PROMOTED 4
int pgps_status(pgps_ctx* ctx, int* flags);
/* float32 series whose call runs a smoother (pgps_pkfs_f32, pgps_pks_f32 and their _dev forms).  The reference's own
 * benchmark grid -- np.linspace(0, 4, N), pssgp/experiments/toy_models/common.py:31-32, with --dtype float32,
 * speed_and_stability.py:68 -- is so dense at N >= 2^15 that float32 ARITHMETIC cannot hold 1e-3 on the smoothed moments
 * (pssgp/kalman/parallel.py:159-166 and sequential.py:57-61 alike rebuild a covariance from a cancellation behind an
 * ill-conditioned solve).  policy 0 (default): such calls probe a sample of the transition matrices on the device and,
 * where the grid is that dense, run in fp64 arithmetic on the float32 arrays (widened into scratch, results rounded
 * back; state dimensions above 16 always do) -- the arrays, the entry points and the tolerances stay the float32 ones;
 * 1: float32 arithmetic whatever the grid; 2: always fp64 arithmetic.  pgps_status tells which way the calls went.
 * Under policy 0 a float32 smoother call is NOT asynchronous: the host waits for the probe's verdict (an event on a
 * stream of the library's own, ordered behind everything already queued on the context's stream), so such a call must
 * not be made while the caller's stream is being captured into a hipGraph -- use policy 1 or 2 there -- and the outputs
 * of pgps_pks_* must not alias its inputs (a promoted call reads fms / fPs after the float32 pass may have written
 * sms / sPs). */
int pgps_set_f32_policy(pgps_ctx* ctx, int policy);

/* ---- device memory helpers (for hosts without a device-array library) ----------------- */
int pgps_malloc(pgps_ctx* ctx, size_t bytes, void** dptr);
int pgps_free(pgps_ctx* ctx, void* dptr);
int pgps_memcpy_h2d(pgps_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int pgps_memcpy_d2h(pgps_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/* ---- per-kernel timing (hipEvents on the context's stream) ----------------------------- */
#define PGPS_K_FILTER_REDUCE 0
#define PGPS_K_FILTER_APPLY 1
#define PGPS_K_SMOOTHER_REDUCE 2
#define PGPS_K_SMOOTHER_APPLY 3
#define PGPS_K_LL_FINALIZE 4
#define PGPS_K_DISCRETISE 5
#define PGPS_K_RESIDENT 6           /* the one-launch filter + smoother pass (pgps_set_resident) */
#define PGPS_K_COUNT 7
/* mask: bit i set = record a hipEvent pair around every launch of slot i; 0 = off. */
int pgps_profile_enable(pgps_ctx* ctx, int mask);
/* Time only every n-th launch of an enabled slot (default 1): keeps the events' own cost
 * (a few microseconds per pair) out of a throughput measurement. */
int pgps_profile_sample(pgps_ctx* ctx, int every_n);
/* Mean elapsed milliseconds of an empty hipEvent pair on the context's stream. */
int pgps_profile_calibrate(pgps_ctx* ctx, double* empty_pair_ms);
/* Synchronises, then returns accumulated milliseconds and launch counts per PGPS_K_* slot
 * since the last reset (arrays of PGPS_K_COUNT). */
int pgps_profile_read(pgps_ctx* ctx, double* total_ms, long* launches, int reset);
const char* pgps_kernel_name(int slot);

/* ---- LTI discretisation: pssgp/kernels/base.py:29-47 (_get_ssm) ------------------------
 * ts (N,), F (d,d), Pinf (d,d) -> Fs (N,d,d), Qs (N,d,d);  dt_0 = ts[0] - t0.
 * Qs = Pinf - Fs Pinf Fs^T (Pinf must be the stationary covariance of the SDE). */
int pgps_discretise_f64(pgps_ctx*, long N, int d, const double* F, const double* Pinf, const double* ts,
                        double t0, double* Fs, double* Qs);
int pgps_discretise_f32(pgps_ctx*, long N, int d, const float* F, const float* Pinf, const float* ts,
                        float t0, float* Fs, float* Qs);
int pgps_discretise_dev_f64(pgps_ctx*, long N, int d, const double* F, const double* Pinf, const double* ts,
                            double t0, double* Fs, double* Qs);
int pgps_discretise_dev_f32(pgps_ctx*, long N, int d, const float* F, const float* Pinf, const float* ts,
                            float t0, float* Fs, float* Qs);

/* ---- parallel filter: pssgp/kalman/parallel.py:121-152 (pkf) ---------------------------
 * LGSSM (P0 (d,d), Fs (N,d,d), Qs (N,d,d), H (1,d), R scalar) + observations ys (N,)
 *   -> fms (N,d), fPs (N,d,d), and the log-likelihood if `ll` != NULL
 * (return_loglikelihood=True, parallel.py:135-151).  m0 = 0 (parallel.py:125). */
int pgps_pkf_f64(pgps_ctx*, long N, int d, const double* P0, const double* Fs, const double* Qs,
                 const double* H, double R, const double* ys, double* fms, double* fPs, double* ll);
int pgps_pkf_f32(pgps_ctx*, long N, int d, const float* P0, const float* Fs, const float* Qs,
                 const float* H, float R, const float* ys, float* fms, float* fPs, double* ll);
int pgps_pkf_dev_f64(pgps_ctx*, long N, int d, const double* P0, const double* Fs, const double* Qs,
                     const double* H, double R, const double* ys, double* fms, double* fPs, double* ll);
int pgps_pkf_dev_f32(pgps_ctx*, long N, int d, const float* P0, const float* Fs, const float* Qs,
                     const float* H, float R, const float* ys, float* fms, float* fPs, double* ll);

/* ---- parallel smoother: pssgp/kalman/parallel.py:187-196 (pks) -------------------------
 * Fs, Qs + filtered fms (N,d), fPs (N,d,d) -> sms (N,d), sPs (N,d,d). */
int pgps_pks_f64(pgps_ctx*, long N, int d, const double* Fs, const double* Qs, const double* fms,
                 const double* fPs, double* sms, double* sPs);
int pgps_pks_f32(pgps_ctx*, long N, int d, const float* Fs, const float* Qs, const float* fms,
                 const float* fPs, float* sms, float* sPs);
int pgps_pks_dev_f64(pgps_ctx*, long N, int d, const double* Fs, const double* Qs, const double* fms,
                     const double* fPs, double* sms, double* sPs);
int pgps_pks_dev_f32(pgps_ctx*, long N, int d, const float* Fs, const float* Qs, const float* fms,
                     const float* fPs, float* sms, float* sPs);

/* ---- joint posterior draws: parallel backward sampling ---------------
 * S joint draws of x_0..x_{N-1} | ys from Fs, Qs and pgps_pkf_* output; d <= PGPS_MAX_DIM_LANE (else
 * PGPS_E_UNSUPPORTED_DIM).  x_{N-1} = fm_{N-1} + C(fP_{N-1}) z_{N-1}, x_k = E_k x_{k+1} + g_k + C(L_k) z_k with
 * (E_k, g_k, L_k) the smoothing element of step k and C the lower semidefinite Cholesky factor.
 * z (S,N,d) caller's standard normals, or NULL = the library's draws for samples s0..s0+S-1 under seed (Philox4x32-10 +
 * Box-Muller: a fixed function of (seed, s0 + s, k, i), whatever the launch geometry; s0 + S <= 2^32).
 * out: (S,N,d) states if H == NULL, else (S,N) of H x_k  (H: d values, host memory).
 * float32 obeys pgps_set_f32_policy as pgps_pks_f32 does: a promoted call runs in fp64 on the fp64 draws, rounds its
 * results and raises PGPS_STATUS_F32_PROMOTED. */
int pgps_pks_sample_f64(pgps_ctx*, long N, int d, const double* Fs, const double* Qs, const double* fms, const double* fPs,
                        int S, long s0, unsigned long long seed, const double* z, const double* H, double* out);
int pgps_pks_sample_f32(pgps_ctx*, long N, int d, const float* Fs, const float* Qs, const float* fms, const float* fPs,
                        int S, long s0, unsigned long long seed, const float* z, const float* H, float* out);
int pgps_pks_sample_dev_f64(pgps_ctx*, long N, int d, const double* Fs, const double* Qs, const double* fms,
                            const double* fPs, int S, long s0, unsigned long long seed, const double* z, const double* H,
                            double* out);
int pgps_pks_sample_dev_f32(pgps_ctx*, long N, int d, const float* Fs, const float* Qs, const float* fms,
                            const float* fPs, int S, long s0, unsigned long long seed, const float* z, const float* H,
                            float* out);
/* the library's draws themselves, (S,N,d), device pointer */
int pgps_sample_normals_dev_f64(pgps_ctx*, long N, int d, int S, long s0, unsigned long long seed, double* z);
int pgps_sample_normals_dev_f32(pgps_ctx*, long N, int d, int S, long s0, unsigned long long seed, float* z);

/* ---- joint posterior covariance between selected steps ----------------
 * Cov(x_i, x_j | ys) = E_i E_{i+1} .. E_{j-1} sP_j for i < j, E_k the smoother gain of step k (the E of its smoothing
 * element, from Fs, Qs and pgps_pkf_* output fPs) and sPs the pgps_pks_* output.  sel: n step indices, strictly
 * increasing, 0 <= sel < N (else PGPS_E_INVALID); n = 1 is valid.  out: (n,n,d,d) blocks Cov(x_sel[a], x_sel[b]) if
 * H == NULL, else (n,n) of H Cov H^T (H: d values, host memory); symmetric bit for bit.  d <= PGPS_MAX_DIM_LANE (else
 * PGPS_E_UNSUPPORTED_DIM); an output that cannot be allocated returns PGPS_E_NOMEM.  float32 obeys pgps_set_f32_policy as
 * pgps_pks_sample_f32 does.  _dev: every array but H is a device pointer (sel included). */
int pgps_pks_cov_f64(pgps_ctx*, long N, int d, const double* Fs, const double* Qs, const double* fPs, const double* sPs,
                     long n, const long* sel, const double* H, double* out);
int pgps_pks_cov_f32(pgps_ctx*, long N, int d, const float* Fs, const float* Qs, const float* fPs, const float* sPs, long n,
                     const long* sel, const float* H, float* out);
int pgps_pks_cov_dev_f64(pgps_ctx*, long N, int d, const double* Fs, const double* Qs, const double* fPs,
                         const double* sPs, long n, const long* sel, const double* H, double* out);
int pgps_pks_cov_dev_f32(pgps_ctx*, long N, int d, const float* Fs, const float* Qs, const float* fPs, const float* sPs,
                         long n, const long* sel, const float* H, float* out);
/* its two passes on their own (native arithmetic of the type, device pointers): the gain products between consecutive
 * selected steps, B (n-1,d,d), B_a = E_{sel[a]} .. E_{sel[a+1]-1} (a segmented scan over the N steps; n >= 2), and the
 * fill of out from B and the n selected smoothed covariances sPsel (n,d,d) */
int pgps_pks_cov_gains_dev_f64(pgps_ctx*, long N, int d, const double* Fs, const double* Qs, const double* fPs, long n,
                               const long* sel, double* B);
int pgps_pks_cov_gains_dev_f32(pgps_ctx*, long N, int d, const float* Fs, const float* Qs, const float* fPs, long n,
                               const long* sel, float* B);
int pgps_cov_fill_dev_f64(pgps_ctx*, long n, int d, const double* B, const double* sPsel, const double* H, double* out);
int pgps_cov_fill_dev_f32(pgps_ctx*, long n, int d, const float* B, const float* sPsel, const float* H, float* out);

/* ---- filter + smoother: pssgp/kalman/parallel.py:199-201 (pkfs) ------------------------
 * One fused three-launch pass.  Also returns the filtered moments and the log-likelihood
 * (the reference's pkfs drops them; StateSpaceGP runs the filter a second time for ll,
 * pssgp/model.py:113-117).  fms / fPs / ll may be NULL for the host entry points; the
 * device entry points need fms and fPs (the smoother reads them back). */
int pgps_pkfs_f64(pgps_ctx*, long N, int d, const double* P0, const double* Fs, const double* Qs,
                  const double* H, double R, const double* ys, double* fms, double* fPs, double* sms,
                  double* sPs, double* ll);
int pgps_pkfs_f32(pgps_ctx*, long N, int d, const float* P0, const float* Fs, const float* Qs,
                  const float* H, float R, const float* ys, float* fms, float* fPs, float* sms,
                  float* sPs, double* ll);
int pgps_pkfs_dev_f64(pgps_ctx*, long N, int d, const double* P0, const double* Fs, const double* Qs,
                      const double* H, double R, const double* ys, double* fms, double* fPs, double* sms,
                      double* sPs, double* ll);
int pgps_pkfs_dev_f32(pgps_ctx*, long N, int d, const float* P0, const float* Fs, const float* Qs,
                      const float* H, float R, const float* ys, float* fms, float* fPs, float* sms,
                      float* sPs, double* ll);

/* ---- fused path: times and observations in, posterior and log-likelihood out ------------------
 * Replaces the chain  _get_ssm (pssgp/kernels/base.py:29-47) -> pkf / pkfs (parallel.py:121-201) that
 * StateSpaceGP runs (pssgp/model.py:92-117) for SDEs whose drift is  F = -lam I + N  with N
 * nilpotent (every Matern kernel; d <= 3):  Fs[k] = exp(-lam dt)(I + dt N1 + dt^2 N2), N1 = N,
 * N2 = N^2/2, and Qs[k] = Pinf - Fs[k] Pinf Fs[k]^T are formed in registers inside the scan kernels,
 * so a pass reads (t, y) instead of the (N, d, d) arrays.  The small model (lam, N1, N2 (may be NULL
 * for d <= 2), Pinf (d,d), H (d)) is always passed from HOST memory; ts, ys and the outputs are
 * device pointers for pgps_gp_dev_* and host pointers for pgps_gp_*.
 *   fms/fPs == NULL and sms/sPs == NULL : log-likelihood only (nothing is written per step)
 *   sms/sPs == NULL                     : filter (pkf with return_loglikelihood=True)
 *   all given                           : filter + smoother (pkfs) + log-likelihood
 *   fms/fPs == NULL, sms/sPs given      : smoother + log-likelihood without the filtered moments.  pgps_gp_f64 stages them
 *                                         itself on every road; pgps_gp_dev_f64 takes the call only where the resident
 *                                         launch runs it (d = 2, pgps_get_family says PGPS_FAMILY_RESIDENT): the three
 *                                         launches hand the filtered moments to the smoother through fms / fPs and
 *                                         answer PGPS_E_INVALID. */
int pgps_gp_dev_f64(pgps_ctx*, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                    const double* H, double R, const double* ts, double t0, const double* ys, double* fms,
                    double* fPs, double* sms, double* sPs, double* ll);
int pgps_gp_dev_f32(pgps_ctx*, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                    const double* H, double R, const float* ts, double t0, const float* ys, float* fms, float* fPs,
                    float* sms, float* sPs, double* ll);
int pgps_gp_f64(pgps_ctx*, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                const double* H, double R, const double* ts, double t0, const double* ys, double* fms, double* fPs,
                double* sms, double* sPs, double* ll);
int pgps_gp_f32(pgps_ctx*, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                const double* H, double R, const float* ts, double t0, const float* ys, float* fms, float* fPs,
                float* sms, float* sPs, double* ll);

/* ---- general LTI models on the device: any kernel, fp64, 2 <= d <= 32 ------------------------------
 * (row-cooperative kernels up to d = 16; 17..32 on the wave-cooperative kernels, with whole moments in device scratch
 * and the projection at the query rows by a separate kernel; the batch entry points cover d <= 16)
 * The chain  _get_ssm (pssgp/kernels/base.py:29-47) -> pkf / pkfs (parallel.py:121-201) that StateSpaceGP runs
 * (pssgp/model.py:92-117) for kernels without the closed-form discretisation (RBF, Periodic, sums, products),
 * with only the results leaving the GPU.  The model F (d,d), Pinf (d,d) (= P0, the stationary covariance: Qs =
 * Pinf - Fs Pinf Fs^T), H (d) is always passed from HOST memory; ts, ys, tq, mean, var, ll are host pointers for
 * the plain entry points and device pointers for the _dev ones.
 *   pgps_lti_ll_*      : discretise, filter, log-likelihood -- nothing is written per step
 *   pgps_lti_predict_* : merge of the sorted ts (N) and tq (K) exactly as _merge_sorted (model.py:15-55), missing
 *                        observations at the query rows, discretise, filter + smoother over the N + K steps,
 *                        mean[j] = H sm, var[j] = H sP H^T of query j; ll (nullable) = log-likelihood of the
 *                        training series.  N + K < 2^31. */
int pgps_lti_ll_f64(pgps_ctx*, long N, int d, const double* F, const double* Pinf, const double* H, double R,
                    const double* ts, const double* ys, double t0, double* ll);
int pgps_lti_ll_dev_f64(pgps_ctx*, long N, int d, const double* F, const double* Pinf, const double* H, double R,
                        const double* ts, const double* ys, double t0, double* ll);
int pgps_lti_predict_f64(pgps_ctx*, long N, long K, int d, const double* F, const double* Pinf, const double* H,
                         double R, const double* ts, const double* ys, double t0, const double* tq, double* mean,
                         double* var, double* ll);
int pgps_lti_predict_dev_f64(pgps_ctx*, long N, long K, int d, const double* F, const double* Pinf, const double* H,
                             double R, const double* ts, const double* ys, double t0, const double* tq, double* mean,
                             double* var, double* ll);
/* linear functionals of the state (additive components of a sum kernel, derivatives of f: DESIGN.md 4z)
 * as pgps_lti_predict_*: merge, missing observations at the query rows, discretise, filter + smoother over N + K steps;
 * C (J,d) HOST, 1 <= J <= PGPS_MAX_FUNCTIONALS (else PGPS_E_INVALID); mean (K,J) = C sm, cov (K,J,J) = C sP C^T of
 * query k, each (J,J) block symmetric bit for bit; ll nullable.  H stays the observation row.  2 <= d <= PGPS_MAX_DIM.
 * d <= 16: 8 K J^2 <= 0x7fff0000 bytes, i.e. K J^2 <= 268427264 = 2^28 - 2^13 (the smoother addresses its outputs with
 * 32-bit byte offsets inside one buffer descriptor; else PGPS_E_INVALID). */
#define PGPS_MAX_FUNCTIONALS 8
int pgps_lti_predict_lin_f64(pgps_ctx*, long N, long K, int d, int J, const double* F, const double* Pinf, const double* H,
                             const double* C, double R, const double* ts, const double* ys, double t0, const double* tq,
                             double* mean, double* cov, double* ll);
int pgps_lti_predict_lin_dev_f64(pgps_ctx*, long N, long K, int d, int J, const double* F, const double* Pinf,
                                 const double* H, const double* C, double R, const double* ts, const double* ys, double t0,
                                 const double* tq, double* mean, double* cov, double* ll);
/* model-level sampler, as pgps_lti_predict_*: merge sorted ts / tq (its query slots give the output column), missing
 * observations at the query rows, discretise, filter, sample; out (S,K) = H x at the K queries of samples s0..s0+S-1
 * (the library's draws under seed); ll (nullable) = training log-likelihood.  1 <= d <= PGPS_MAX_DIM_LANE, fp64. */
int pgps_lti_sample_f64(pgps_ctx*, long N, long K, int d, const double* F, const double* Pinf, const double* H, double R,
                        const double* ts, const double* ys, double t0, const double* tq, int S, long s0,
                        unsigned long long seed, double* out, double* ll);
int pgps_lti_sample_dev_f64(pgps_ctx*, long N, long K, int d, const double* F, const double* Pinf, const double* H,
                            double R, const double* ts, const double* ys, double t0, const double* tq, int S, long s0,
                            unsigned long long seed, double* out, double* ll);

/* model-level joint predictive, as pgps_lti_predict_*: merge sorted ts / tq, missing observations at the query rows,
 * discretise, filter + smoother over the N + K steps, gain products between the query rows, fill.  mean (K) = H sm,
 * cov (K,K) = H Cov(x_i, x_j) H^T of the queries, symmetric bit for bit, its diagonal the variances; ll (nullable) =
 * training log-likelihood.  1 <= d <= PGPS_MAX_DIM_LANE, fp64. */
int pgps_lti_predict_cov_f64(pgps_ctx*, long N, long K, int d, const double* F, const double* Pinf, const double* H,
                             double R, const double* ts, const double* ys, double t0, const double* tq, double* mean,
                             double* cov, double* ll);
int pgps_lti_predict_cov_dev_f64(pgps_ctx*, long N, long K, int d, const double* F, const double* Pinf, const double* H,
                                 double R, const double* ts, const double* ys, double t0, const double* tq, double* mean,
                                 double* cov, double* ll);

/* B models over the same series in one set of launches (hyper-parameter grids, HMC chains, multi-start optimisation
 * -- the realistic series, N = 1e3..1e5, are launch-latency bound one model at a time).  `models` is HOST memory,
 * B rows of [F (d*d) | Pinf (d*d) | H (d) | R]; ll receives B log-likelihoods (host pointer; device for _dev). */
int pgps_lti_ll_batch_f64(pgps_ctx*, int B, long N, int d, const double* models, const double* ts, const double* ys,
                          double t0, double* ll);
int pgps_lti_ll_batch_dev_f64(pgps_ctx*, int B, long N, int d, const double* models, const double* ts, const double* ys,
                              double t0, double* ll);

/* ---- predict_f on the device (fused path, d <= 3) --------------------------------------------------
 * StateSpaceGP.predict_f (pssgp/model.py:92-111) in one call: the sorted training times `ts` (N) and
 * sorted query times `tq` (K) are merged on the device exactly as _merge_sorted does (model.py:15-55:
 * on equal times the shorter array's point comes first), query rows carry missing observations, the
 * fused filter + smoother runs over the N + K steps and only  mean[j] = H sm,  var[j] = H sP H^T  of
 * query j are written -- 2 scalars per query instead of (d^2 + d) per merged step.  ll (nullable)
 * receives the log-likelihood of the training series (query rows contribute nothing).
 * Host pointers; the _dev form takes device pointers for ts, ys, tq, mean, var, ll.  N + K < 2^31. */
int pgps_gp_predict_f64(pgps_ctx*, long N, long K, int d, double lam, const double* N1, const double* N2,
                        const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                        const double* tq, double* mean, double* var, double* ll);
int pgps_gp_predict_f32(pgps_ctx*, long N, long K, int d, double lam, const double* N1, const double* N2,
                        const double* Pinf, const double* H, double R, const float* ts, const float* ys, double t0,
                        const float* tq, float* mean, float* var, double* ll);
int pgps_gp_predict_dev_f64(pgps_ctx*, long N, long K, int d, double lam, const double* N1, const double* N2,
                            const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                            double t0, const double* tq, double* mean, double* var, double* ll);
int pgps_gp_predict_dev_f32(pgps_ctx*, long N, long K, int d, double lam, const double* N1, const double* N2,
                            const double* Pinf, const double* H, double R, const float* ts, const float* ys,
                            double t0, const float* tq, float* mean, float* var, double* ll);

/* ---- batched log-likelihood (fused path, d <= 3) ---------------------------------------------------
 * B hyper-parameter settings evaluated over the SAME series in one pair of launches (HMC leapfrogs,
 * grid search, multi-start optimisation at the reference's typical N of 1e3..1e5: SURVEY.md section
 * 8f rank 3).  `models` (HOST memory): B consecutive blocks [lam | N1 (d*d) | N2 (d*d) | Pinf (d*d) |
 * H (d) | R].  ll: B doubles.  Each ll[m] is bit-identical to what pgps_gp_* returns for model m at
 * the same steps-per-lane geometry.  ts, ys, ll: host pointers; device pointers for the _dev form.
 * B <= 65535. */
int pgps_gp_ll_batch_f64(pgps_ctx*, int B, long N, int d, const double* models, const double* ts, double t0,
                         const double* ys, double* ll);
int pgps_gp_ll_batch_f32(pgps_ctx*, int B, long N, int d, const double* models, const float* ts, double t0,
                         const float* ys, double* ll);
int pgps_gp_ll_batch_dev_f64(pgps_ctx*, int B, long N, int d, const double* models, const double* ts, double t0,
                             const double* ys, double* ll);
int pgps_gp_ll_batch_dev_f32(pgps_ctx*, int B, long N, int d, const double* models, const float* ts, double t0,
                             const float* ys, double* ll);

/* ---- predict_f at B hyper-parameter settings (fused path, d <= 3) --------------------------------
 * The posterior of f at K query times for B models over the SAME series and the SAME query grid in one set of launches:
 * one merge (shared), then B filters + smoothers + projections side by side -- the last step of the reference's MCMC
 * drivers (pssgp/experiments/sunspot/mcmc.py:78-97: predict_f at the draws of the chain), one launch-latency-bound call
 * per draw otherwise.  `models` (HOST memory) as pgps_gp_ll_batch_*: B blocks [lam | N1 | N2 | Pinf | H | R]; ts (N), tq (K)
 * sorted, ties merged as in pgps_gp_predict_*; mean, var: (B, K) row-major; ll: B training log-likelihoods or NULL.
 * Host pointers; device pointers (except models) for the _dev forms, which return with the launches enqueued (they
 * synchronise the stream ONCE, before the launches, to copy the model table in).  Row b equals
 * pgps_gp_predict_* of model b up to rounding (another bracketing of the same scans), and does not depend on the other
 * rows, on its position, on B's split into groups (pgps_set_batch_scratch) -- the geometry is fixed per call from
 * (B, N + K).  Errors: B, N, K < 1, a null pointer, lam <= 0 or R <= 0 in a row: PGPS_E_INVALID; d outside 1..3:
 * PGPS_E_UNSUPPORTED_DIM; a non-finite log-likelihood (host forms): PGPS_E_NUMERIC; no scratch: PGPS_E_NOMEM. */
int pgps_gp_predict_batch_f64(pgps_ctx*, int B, long N, long K, int d, const double* models, const double* ts,
                              const double* ys, double t0, const double* tq, double* mean, double* var, double* ll);
int pgps_gp_predict_batch_f32(pgps_ctx*, int B, long N, long K, int d, const double* models, const float* ts,
                              const float* ys, double t0, const float* tq, float* mean, float* var, double* ll);
int pgps_gp_predict_batch_dev_f64(pgps_ctx*, int B, long N, long K, int d, const double* models, const double* ts,
                                  const double* ys, double t0, const double* tq, double* mean, double* var, double* ll);
int pgps_gp_predict_batch_dev_f32(pgps_ctx*, int B, long N, long K, int d, const double* models, const float* ts,
                                  const float* ys, double t0, const float* tq, float* mean, float* var, double* ll);
/* The same for ANY kernel's LTI model (fp64, 2 <= d <= 16; d outside: PGPS_E_UNSUPPORTED_DIM): `models` (HOST) as
 * pgps_lti_ll_batch_*, B rows [F | Pinf | H | R].  One merge, one batched discretisation, then the row-cooperative filter +
 * smoother + projection of all models side by side (one model per blockIdx.y): the launches of ONE predict whatever B,
 * in groups that fit the batch budget (default 1 GiB here; about 3 (N + K) d^2 doubles per model).  The chain length is
 * fixed per call from (B, N + K), so a row does not depend on the grouping, on its position or on the other rows. */
int pgps_lti_predict_batch_f64(pgps_ctx*, int B, long N, long K, int d, const double* models, const double* ts,
                               const double* ys, double t0, const double* tq, double* mean, double* var, double* ll);
int pgps_lti_predict_batch_dev_f64(pgps_ctx*, int B, long N, long K, int d, const double* models, const double* ts,
                                   const double* ys, double t0, const double* tq, double* mean, double* var, double* ll);
/* Moments of the mixture sum_b w_b N(mean_b, var_b), column by column of (B, K) device arrays: mean_out = sum_b w_b mean_b,
 * var_out = sum_b w_b (var_b + (mean_b - mean_out)^2) -- two passes, every term non-negative; w (B, device) is used as
 * given (normalise it), NULL = 1 / B each.  fp64, deterministic (fixed summation order).  Does not synchronise. */
int pgps_mix_moments_dev_f64(pgps_ctx*, int B, long K, const double* mean, const double* var, const double* w,
                             double* mean_out /* K */, double* var_out /* K */);
/* Scratch budget of the batched predict in bytes (0 = the defaults: 64 MiB for pgps_gp_predict_batch_*, 1 GiB for
 * pgps_lti_predict_batch_*): the models run in groups whose filtered
 * moments and scan records fit it (one model at least).  Results do not depend on it. */
int pgps_set_batch_scratch(pgps_ctx* ctx, size_t bytes);
/* Launch form of pgps_gp_predict_batch_*: 0 = automatic (form 2), 1 = one workgroup per model in one launch (taken up to
 * 65 536 merged steps, form 2 beyond), 2 = three launches of (workgroups, models) grids. */
int pgps_set_batch_form(pgps_ctx* ctx, int form);

/* ---- log-likelihood and its gradient (fused path, d <= 3, fp64) --------------------------------
 * What the reference gets from TensorFlow autodiff through the scan (tests/test_gp_vs_kfs.py:53-78;
 * SURVEY.md section 8f, rank 1): forward-mode dual numbers carried through every filtering element and
 * every application of the associative operator.  `model` (HOST memory) holds 1 + np blocks of
 * [lam | N1 (d*d) | Pinf (d*d) | H (d) | R]: block 0 the values, block p the partial derivatives with
 * respect to hyper-parameter p (np <= 3).  out[0] = log-likelihood, out[1..np] = its gradient.
 * ts, ys, out: host pointers for pgps_gp_ll_grad_f64, device pointers for the _dev form, whose `out`
 * must hold 1 + 3 np doubles (the tail is scratch for the d = 3 one-direction-per-pass schedule). */
int pgps_gp_ll_grad_f64(pgps_ctx*, long N, int d, int np, const double* model, const double* ts, double t0,
                        const double* ys, double* out);
int pgps_gp_ll_grad_dev_f64(pgps_ctx*, long N, int d, int np, const double* model, const double* ts, double t0,
                            const double* ys, double* out);

/* The same for composite kernels whose drift is block diagonal with blocks  F_b = -lam_b I + N_b,  N_b nilpotent --
 * sums and products of Matern kernels, balanced or not (kernels/base.py:130-244; a product of Matern kernels is one
 * block: lam = the sum of the factors', N = the Kronecker sum of theirs) -- state dimension 2 <= d <= 6, nblk <= 4
 * blocks of sizes bsize[] (sum d), np <= 16 hyper-parameters: the reference's gradient test kernels `Matern32 +
 * Matern52` and `Matern32 * Matern52` (tests/test_gp_vs_kfs.py:40-41,53-78) differentiated exactly, by dual numbers
 * through the scan, one direction per pass.  `model` (HOST memory): 1 + np rows of
 * [lam (4, unused ones 0) | N (d*d) | Pinf (d*d) | H (d) | R], row 0 the values, row p the partial derivatives with
 * respect to hyper-parameter p.  out[0] = log-likelihood, out[1..np] = gradient; the _dev form takes device pointers
 * for ts, ys, out, and its `out` must hold 1 + 3 np doubles (the tail is scratch). */
int pgps_gp_ll_grad_blocks_f64(pgps_ctx*, long N, int d, int nblk, const int* bsize, int np, const double* model,
                               const double* ts, double t0, const double* ys, double* out);
int pgps_gp_ll_grad_blocks_dev_f64(pgps_ctx*, long N, int d, int nblk, const int* bsize, int np, const double* model,
                                   const double* ts, double t0, const double* ys, double* out);

/* ---- one series sharded over several GPUs (contiguous time segments) -------------------
 * No reference equivalent (the reference is single-device).  Rank r of
 * `nranks` owns steps [r*N, (r+1)*N) -- every rank passes its own N -- and calls, in order:
 *   1. pgps_seg_filter_reduce_dev   -> rec_f  (pgps_seg_record_len: rec_filter elements)
 *      caller all-gathers rec_f over the ranks -> gathered_f (nranks, rec_filter)
 *   2. pgps_seg_filter_apply_dev    -> fms, fPs, rec_s (rec_smoother elements)
 *      caller all-gathers rec_s -> gathered_s (nranks, rec_smoother)
 *   3. pgps_seg_smoother_apply_dev  -> sms, sPs, ll (log-likelihood of the WHOLE series)
 * The three calls of one pass must use the same context, N and d (they share its scratch).
 * rec_f = [segment total (A, b, C, J, eta) | F, Q of the segment's first step];
 * rec_s = [segment total (E, g, L) | pad | the segment's log-likelihood as a double]. */
int pgps_seg_record_len(int d, int* rec_filter, int* rec_smoother);
int pgps_seg_filter_reduce_dev_f64(pgps_ctx*, long N, int d, int rank, int nranks, const double* P0,
                                   const double* Fs, const double* Qs, const double* H, double R,
                                   const double* ys, double* rec_f);
int pgps_seg_filter_reduce_dev_f32(pgps_ctx*, long N, int d, int rank, int nranks, const float* P0,
                                   const float* Fs, const float* Qs, const float* H, float R, const float* ys,
                                   float* rec_f);
int pgps_seg_filter_apply_dev_f64(pgps_ctx*, long N, int d, int rank, int nranks, const double* P0,
                                  const double* Fs, const double* Qs, const double* H, double R,
                                  const double* ys, const double* gathered_f, double* fms, double* fPs,
                                  double* rec_s);
int pgps_seg_filter_apply_dev_f32(pgps_ctx*, long N, int d, int rank, int nranks, const float* P0,
                                  const float* Fs, const float* Qs, const float* H, float R, const float* ys,
                                  const float* gathered_f, float* fms, float* fPs, float* rec_s);
int pgps_seg_smoother_apply_dev_f64(pgps_ctx*, long N, int d, int rank, int nranks, const double* Fs,
                                    const double* Qs, const double* fms, const double* fPs,
                                    const double* gathered_s, double* sms, double* sPs, double* ll);
int pgps_seg_smoother_apply_dev_f32(pgps_ctx*, long N, int d, int rank, int nranks, const float* Fs,
                                    const float* Qs, const float* fms, const float* fPs, const float* gathered_s,
                                    float* sms, float* sPs, double* ll);

/* The three calls of a pass keep state in the context's scratch between them (chain totals, their scans, for
 * d > 6 the stored smoothing elements): no other call on the same context, and no pgps_set_chunk, may come between
 * phase 1 and phase 3 of a pass.  The library checks it -- a phase whose predecessor was not the previous call on the
 * context with the same (N, d, rank, nranks) returns PGPS_E_INVALID instead of reading stale scratch. */

/* ---- the same pass with the exchange inside the library: RCCL over xGMI ----------------------------
 * The context owns the communicator (one process per GPU, one context per process).
 *   rank 0:      pgps_comm_get_unique_id(id)   -> hand the PGPS_COMM_ID_BYTES bytes to every rank (any transport)
 *   every rank:  pgps_comm_init(ctx, id, rank, nranks)        (collective: returns when all ranks have joined)
 *   every rank:  pgps_pkfs_seg_dev_*(ctx, N_local, d, ...)    per pass, as often as wanted
 *   every rank:  pgps_comm_destroy(ctx)                       (pgps_destroy does it too)
 * pgps_pkfs_seg_dev_* = pkfs (pssgp/kalman/parallel.py:199-201) + log-likelihood for the segment [rank's steps] of a
 * series sharded over the communicator's ranks in rank order: reduce -> ncclAllGather (segment totals + first-step
 * halo, (3d^2+3d+d(d+1)) scalars per rank) -> filter -> ncclAllGather (smoothing totals + log-likelihood partial) ->
 * smoother, ALL enqueued on the context's stream: no host synchronisation, no framework.  Arguments as
 * pgps_pkfs_dev_* with this rank's arrays; P0 is the prior of the WHOLE series (used by rank 0), ll receives the
 * log-likelihood of the whole series on every rank.  d <= PGPS_MAX_DIM, fp64 and fp32 natively.  nranks = 1 works
 * (RCCL copies locally).  pgps_comm_allgather_dev is the bare collective on the context's stream (bytes per rank). */
#define PGPS_COMM_ID_BYTES 128
int pgps_comm_get_unique_id(void* id);
int pgps_comm_init(pgps_ctx* ctx, const void* id, int rank, int nranks);
int pgps_comm_destroy(pgps_ctx* ctx);
int pgps_comm_info(pgps_ctx* ctx, int* rank, int* nranks);      /* nranks = 0: no communicator */
int pgps_comm_count(pgps_ctx* ctx, int* nranks, int* rank);     /* as RCCL reports them (ncclCommCount / ncclCommUserRank); rank may be NULL */
/* RCCL is loaded on first use of a pgps_comm_* call (the copy already in the process, else the loader's librccl.so.1):
 * buf <- what was loaded, or why nothing was (PGPS_E_COMM).  A context without a communicator never needs RCCL. */
int pgps_comm_library(char* buf, size_t n);
int pgps_comm_allgather_dev(pgps_ctx* ctx, const void* send, void* recv, size_t bytes_per_rank);
int pgps_pkfs_seg_dev_f64(pgps_ctx*, long N, int d, const double* P0, const double* Fs, const double* Qs, const double* H,
                          double R, const double* ys, double* fms, double* fPs, double* sms, double* sPs, double* ll);
int pgps_pkfs_seg_dev_f32(pgps_ctx*, long N, int d, const float* P0, const float* Fs, const float* Qs, const float* H,
                          float R, const float* ys, float* fms, float* fPs, float* sms, float* sPs, double* ll);

/* ---- observations with error bars: per-observation noise variances (fused path, fp64, d <= 3) ----------
 * The model  y_k = H x_k + e_k,  e_k ~ N(0, R + rs[k]):  `rs` (N) are GIVEN variances (the squares of the error bars), R the one
 * shared, trainable jitter.  Each entry point is its scalar namesake (pgps_gp_dev_f64 with only ll asked for /
 * pgps_gp_predict_f64 / pgps_gp_ll_grad_adj_dev_f64) with `rs` behind `ys`; out = [ll | Abar | Ubar | Hbar | Rbar] as
 * pgps_gp_ll_grad_adj_dev_f64 lays it out, Rbar = d ll / d R = sum_k d ll / d (R + rs[k]).  The predict call merges the sorted
 * ts and tq as pgps_gp_predict_* does (equal times: the shorter array's point first) and carries ys and rs through the merge.
 * rs[k] is read at observed steps only: where ys[k] is NaN it may hold anything, NaN included.  R >= 0 is accepted; the
 * requirement is rs[k] finite, rs[k] >= 0 and R + rs[k] > 0 at every observed step.  The host-array forms scan rs once and
 * return PGPS_E_INVALID where that fails; for the _dev forms (device pointers ts, ys, rs, tq, mean, var, ll / out; asynchronous on
 * the context's stream) it is a PRECONDITION.  A null pointer (rs included), N < 1, K < 1, lam <= 0, R < 0 or not finite:
 * PGPS_E_INVALID; d outside 1..3: PGPS_E_UNSUPPORTED_DIM; host forms: a non-finite ll: PGPS_E_NUMERIC.  Three launches per
 * call whatever N (pgps_set_chunk honoured; pgps_set_one_launch and pgps_set_resident do not apply). */
int pgps_gp_ll_het_f64(pgps_ctx*, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                       const double* H, double R, const double* ts, const double* ys, const double* rs, double t0, double* ll);
int pgps_gp_ll_het_dev_f64(pgps_ctx*, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                           const double* H, double R, const double* ts, const double* ys, const double* rs, double t0,
                           double* ll);
int pgps_gp_predict_het_f64(pgps_ctx*, long N, long K, int d, double lam, const double* N1, const double* N2,
                            const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                            const double* rs, double t0, const double* tq, double* mean, double* var, double* ll);
int pgps_gp_predict_het_dev_f64(pgps_ctx*, long N, long K, int d, double lam, const double* N1, const double* N2,
                                const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                const double* rs, double t0, const double* tq, double* mean, double* var, double* ll);
int pgps_gp_ll_grad_adj_het_f64(pgps_ctx*, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                                const double* H, double R, const double* ts, double t0, const double* ys, const double* rs,
                                double* out /* 1 + d d + 2 d + 1 */);
int pgps_gp_ll_grad_adj_het_dev_f64(pgps_ctx*, long N, int d, double lam, const double* N1, const double* N2,
                                    const double* Pinf, const double* H, double R, const double* ts, double t0,
                                    const double* ys, const double* rs, double* out /* 1 + d d + 2 d + 1 */);

/* ---- a panel: S independent series, each on its own clock and of its own length (fused path, fp64, d <= 3) ----
 * Light curves of a survey, one record per patient or sensor, the folds of a cross-validation: series of 10^2 .. 10^3 points,
 * where one evaluation is bound by launch latency.  A panel call gives every series ONE workgroup of ONE launch.
 *   offs    (S + 1) HOST, strictly increasing from 0: series s is rows offs[s] .. offs[s + 1] of the concatenated ts, ys, rs
 *           (each series sorted by time, NaN in ys = missing)
 *   qoffs   (S + 1) HOST, non-decreasing from 0: its queries are rows qoffs[s] .. qoffs[s + 1] of tq (sorted per series), and of
 *           mean / var; a series may have none (it still returns its ll); qoffs[S] >= 1
 *   models  HOST, nmodels rows [lam | N1 (d d) | N2 (d d) | Pinf (d d) | H (d) | R] as pgps_gp_ll_batch_* takes them; nmodels = 1
 *           (shared by all series) or S (row s for series s)
 *   rs      per-observation noise variances as pgps_gp_ll_het_* take them (read at observed rows only, R + rs[k] > 0), or NULL:
 *           scalar noise R
 *   ll      (S); out (S, 1 + d d + 2 d + 1) rows [ll | Abar | Ubar | Hbar | Rbar] as pgps_gp_ll_grad_adj_dev_f64 lays them out.
 * Row s is what the single-series call on series s computes (t0 = the series' first time; the predict call merges as
 * pgps_gp_predict_* does, per series).  A series is limited to PGPS_PANEL_MAX_STEPS steps, counted MERGED (n + k) in predict.  Each
 * series takes max(1, ceil(steps / 256)) steps per lane (pgps_set_chunk: the pinned value wherever it covers the series), so a
 * row's bits depend on that series alone: not on the other series, on its place, on repetition, or on how the series are split
 * into groups that fit pgps_set_batch_scratch (at most 65535 series per launch).
 * Host forms take host arrays, scan rs once (PGPS_E_INVALID where the rule fails) and return PGPS_E_NUMERIC on a non-finite ll;
 * _dev forms take device pointers for everything but offs / qoffs / models, synchronise the context's stream ONCE to copy their
 * tables in and are asynchronous afterwards (the rule of rs is a PRECONDITION).  Errors: S < 1, a null pointer (rs, and ll of
 * predict, excepted), an empty series, a series above PGPS_PANEL_MAX_STEPS, qoffs[S] < 1, nmodels not 1 or S, lam <= 0 or R < 0
 * in a row, R <= 0 in a row when rs is NULL: PGPS_E_INVALID; d outside 1..3: PGPS_E_UNSUPPORTED_DIM. */
#define PGPS_PANEL_MAX_STEPS 2048
int pgps_gp_panel_ll_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, const double* ts,
                         const double* ys, const double* rs, double* ll);
int pgps_gp_panel_ll_dev_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, const double* ts,
                             const double* ys, const double* rs, double* ll);
int pgps_gp_panel_ll_grad_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, const double* ts,
                              const double* ys, const double* rs, double* out);
int pgps_gp_panel_ll_grad_dev_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models,
                                  const double* ts, const double* ys, const double* rs, double* out);
int pgps_gp_panel_predict_f64(pgps_ctx*, long S, const long* offs, const long* qoffs, int d, int nmodels, const double* models,
                              const double* ts, const double* ys, const double* rs, const double* tq, double* mean,
                              double* var, double* ll);
int pgps_gp_panel_predict_dev_f64(pgps_ctx*, long S, const long* offs, const long* qoffs, int d, int nmodels,
                                  const double* models, const double* ts, const double* ys, const double* rs, const double* tq,
                                  double* mean, double* var, double* ll);

/* ---- predictive checks of a fitted model against its own data (fused path, fp64, d <= 3) --------------
 * Two laws of every y_k, from ONE filter and ONE smoother pass over the N training steps (no merge, no query rows):
 *   osa_mean, osa_var   y_k given the observations BEFORE it: N(H m_k^-, H P_k^- H^T + R), the pair the Kalman pass hands to its
 *                       log-likelihood accumulator (the first-step rule included); their log densities sum to the log-likelihood;
 *   loo_mean, loo_var   y_k given ALL OTHER observations (leave-one-out): with (m, v) the smoothed mean and variance of
 *                       f_k = H x_k,  N((m R - y_k v) / (R - v), R^2 / (R - v)).
 * Both variances include R.  Where ys[k] is NaN the laws are those of an observation there (leave-one-out: nothing is left
 * out, N(m, v + R)) and the step adds nothing to either sum.  Each of the four arrays (N doubles) may be NULL: that store is
 * skipped.  sums[2] = {log-likelihood, sum over the observed steps of log N(y_k | loo_mean, loo_var)} is always written; the
 * workgroups' partials are added in index order, so equal calls give equal bits, with or without the arrays.  Log densities
 * per step are not stored: they follow from (y, mean, var).  Arguments as pgps_gp_ll_het_f64 takes them, without rs.
 * The _dev form takes device pointers (ts, ys, the arrays, sums) and is asynchronous on the context's stream; the host form
 * copies back only the arrays asked for (none: two doubles).  A null ts / ys / sums, N < 1, lam <= 0, R <= 0 or not finite
 * (leaving out a noise-free observation is undefined): PGPS_E_INVALID; d outside 1..3: PGPS_E_UNSUPPORTED_DIM; host form: a
 * non-finite sum: PGPS_E_NUMERIC.  Four launches per call whatever N (pgps_set_chunk honoured; pgps_set_one_launch and
 * pgps_set_resident do not apply). */
int pgps_gp_loo_f64(pgps_ctx*, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                    const double* H, double R, const double* ts, const double* ys, double t0, double* osa_mean, double* osa_var,
                    double* loo_mean, double* loo_var, double* sums /* 2 */);
int pgps_gp_loo_dev_f64(pgps_ctx*, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                        const double* H, double R, const double* ts, const double* ys, double t0, double* osa_mean,
                        double* osa_var, double* loo_mean, double* loo_var, double* sums /* 2 */);

/* ---- ... of every series of a panel, in one launch per group ------------------------------------------
 * offs, models, rs, PGPS_PANEL_MAX_STEPS and the host / device conventions are those of pgps_gp_panel_ll_*; the four arrays hold
 * one value per row of the concatenated series (offs[S] doubles), each may be NULL; sums (S, 2) = {ll, loo_lpd} per series is
 * always written.  Row s is what pgps_gp_loo_* computes on series s alone (t0 = the series' first time), with the step's noise
 * variance R + rs[k] where rs is given.  At a row where ys is NaN the stored variances are ... + R + rs[k] with rs[k] AS STORED (a
 * NaN there gives a NaN variance at that row only; it never enters the recursions).  A row's bits depend on that series alone
 * (the list at pgps_gp_panel_ll_*), and they do not change when arrays are NULL.
 * Errors (no output is touched): those of pgps_gp_panel_ll_*, among them R <= 0 in a row when rs is NULL, and a null sums:
 * PGPS_E_INVALID; d outside 1..3: PGPS_E_UNSUPPORTED_DIM.  The host form scans rs once (finite, >= 0 and R + rs[k] > 0 at the
 * observed rows, else PGPS_E_INVALID: a PRECONDITION of the _dev form), copies back only the arrays asked for and returns
 * PGPS_E_NUMERIC on a non-finite sum. */
int pgps_gp_panel_loo_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, const double* ts,
                          const double* ys, const double* rs, double* osa_mean, double* osa_var, double* loo_mean,
                          double* loo_var, double* sums /* (S, 2) */);
int pgps_gp_panel_loo_dev_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, const double* ts,
                              const double* ys, const double* rs, double* osa_mean, double* osa_var, double* loo_mean,
                              double* loo_var, double* sums /* (S, 2) */);

/* ---- mean functions of a panel: the whitened Gram matrix of 1 + p columns of every series -------------
 * V (offs[S], C) row-major over the concatenated rows, C = 1 + p in 1 .. 8: column 0 is y, columns 1 .. p the basis functions of
 * the series' trend at its own times.  With K_y = K + diag(R + rs) on the observed rows of series s, record s of out is
 *   [G (C, C) row-major | logdet | n_obs],  G = V_s^T K_y^-1 V_s,  logdet = log det K_y,  n_obs = observed rows (as a double),
 * which holds the GLS trend coefficients of that series, their covariance and the profile likelihood (pgps_gp_gram_multi_* for
 * one series; with C = 1, -(n_obs log 2 pi + logdet + G[0]) / 2 is the row of pgps_gp_panel_ll_*).  A row that is NaN in column 0
 * is a missing step: the other columns are not read there and the row contributes nothing.  G is symmetric bit for bit.
 * offs, models, rs, PGPS_PANEL_MAX_STEPS, steps per lane, groups and the host / device conventions are those of pgps_gp_panel_ll_*; a
 * record's bits depend on that series' rows, its model row, C and the pinned chunk alone.  One launch per group.
 * Errors (no output is touched): those of pgps_gp_panel_ll_*, C outside 1 .. 8, a null out: PGPS_E_INVALID; d outside 1..3:
 * PGPS_E_UNSUPPORTED_DIM.  The host form also scans V and rs once: a row that is NaN in some columns only, or rs against its rule
 * at an observed row: PGPS_E_INVALID (PRECONDITIONS of the _dev form); a non-finite logdet: PGPS_E_NUMERIC.
 * pgps_gp_panel_residual_dev_f64: ys_out[k] = V[k, 0] - sum_j V[k, 1 + j] betas[s, j] for the rows k of series s, the sum taken
 * left to right, every product and sum rounded once; NaN in column 0 stays NaN.  betas (S, C - 1) [device] (may be NULL at
 * C = 1), V and ys_out [device]; ys_out may be the ys of another panel call.  Synchronises the stream once to copy offs in. */
int pgps_gp_panel_gram_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, int C, const double* ts,
                           const double* V, const double* rs, double* out /* (S, C C + 2) */);
int pgps_gp_panel_gram_dev_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, int C,
                               const double* ts, const double* V, const double* rs, double* out /* (S, C C + 2) */);
int pgps_gp_panel_residual_dev_f64(pgps_ctx*, long S, const long* offs, int C, const double* V, const double* betas,
                                   double* ys_out);

/* ---- the panel's GLS solves on the device, and the profile gradient of every series in one call --------
 * pgps_gp_panel_trend_solve_*: records (S, C C + 2) as pgps_gp_panel_gram_* writes them, C = 1 + p in 1 .. 8.  With g_yy = G[0,0],
 * b = G[1:,0], A = G[1:,1:] of series s, one lane solves A beta = b by a Cholesky factor of the unit-diagonal scaling of A
 * (s_i = 1 / sqrt(A_ii), Au = diag(s) A diag(s) = L L^T in a fixed order, every product and sum rounded once):
 *   betas (S, p)       beta_hat = s o L^-T L^-1 (s o b): exactly what pgps_gp_panel_residual_dev_f64 takes
 *   sol (S, p p + 4)   [cov (p, p) row-major | profile | flat | logdet_A | status]
 *                      cov = s o (L^-T L^-1) o s, symmetric bit for bit;  logdet_A = 2 sum log L_ii - 2 sum log s_i;
 *                      profile = -(n_obs log 2 pi + logdet + g_yy - b . beta_hat) / 2;  flat = profile - logdet_A / 2 + p log 2 pi / 2
 *   status (a double)  0 solved; 1 an entry of A is not finite or a diagonal entry is <= 0; 2 a pivot's square is <= 0 or not
 *                      finite; 3 the smallest pivot squared is <= 64 p eps (A is rank deficient to working precision).
 *                      At status != 0 that series' betas, cov, profile, flat and logdet_A are NaN; no other series is touched.
 * At C = 1 nothing is solved: status 0, flat = profile = -(n_obs log 2 pi + logdet + g_yy) / 2, logdet_A = 0, betas is not
 * written and may be NULL.  A series' outputs depend on its own record and C alone.  One launch.  The _dev form (records, betas,
 * sol device) queues the launch and does not synchronise; the host form returns through vectors of the call.
 * Errors (no output is touched): S < 1, C outside 1 .. 8, null records or sol, null betas with C > 1: PGPS_E_INVALID.  A
 * rank-deficient series is data, not an error: PGPS_OK and its status says so.
 *
 * pgps_gp_panel_profile_grad_*: for every series the Gram record of V (pgps_gp_panel_gram_*), its solve (above), the residuals
 * y - Phi beta_hat into ys_work (pgps_gp_panel_residual_dev_f64) and the adjoint pass on them (pgps_gp_panel_ll_grad_*):
 *   betas (S, C - 1), sol (S, (C-1)^2 + 4) as above;  out (S, 2 + d d + 2 d): row s = [profile ll | Abar | Ubar | Hbar | Rbar],
 * the record of pgps_gp_panel_ll_grad_* on the residual series (out[s, 0] and sol's profile are one quantity by two routes).  By
 * definition the bits are those of the four separate _dev calls: the same kernels, steps per lane and grouping rule.  All tables
 * of both phases ([models | Gram records | adjoint records | offs]) go up in ONE copy behind ONE stream synchronisation before
 * the first launch; the _dev form (ts .. out device, ys_work (offs[S]) device) then queues every launch and does not synchronise
 * again.  The host form stages as pgps_gp_panel_gram_f64 does (same scans of V and rs) and returns through vectors of the call.
 * Errors (no output is touched): those of pgps_gp_panel_gram_*; null sol, out or ys_work, null betas with C > 1: PGPS_E_INVALID.
 * The host form returns PGPS_E_NUMERIC (outputs written) when a series of status 0 has a non-finite profile or out[s, 0]; a series
 * whose status != 0 has NaN rows of betas, sol and out, and the call returns PGPS_OK. */
int pgps_gp_panel_trend_solve_f64(pgps_ctx*, long S, int C, const double* records /* (S, C C + 2) */, double* betas /* (S, C-1) */,
                                  double* sol /* (S, (C-1)^2 + 4) */);
int pgps_gp_panel_trend_solve_dev_f64(pgps_ctx*, long S, int C, const double* records, double* betas, double* sol);
int pgps_gp_panel_profile_grad_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, int C,
                                   const double* ts, const double* V, const double* rs, double* betas, double* sol,
                                   double* out /* (S, 2 + d d + 2 d) */);
int pgps_gp_panel_profile_grad_dev_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, int C,
                                       const double* ts, const double* V, const double* rs, double* betas, double* sol,
                                       double* ys_work /* (offs[S]) */, double* out /* (S, 2 + d d + 2 d) */);

/* ---- Laplace inference for non-Gaussian observations (fused path, fp64, d <= 3) -------------------------
 * Observations y_k ~ p(y | f(t_k)) with a log-concave likelihood, `lik` one of PGPS_LIK_* with one parameter `par` (csrc/
 * pgps_lik.h: lp = log p, g = lp', W = -lp'' floored at 1e-10, d3 = lp''').  A SITE formed at f is the Gaussian factor
 * N(z | f, s), s = 1 / W, z = f + g / W; at a NaN row of ys, z = NaN and s = 1 (the filter skips the row).
 *
 * pgps_gp_newton_*: ONE Newton step of the mode search = one Gaussian smoothing pass over the sites (zs, ss) with R = 0 (the
 * per-observation-noise reduce and Kalman pass as they are, a smoother that projects at EVERY training step, a finalize):
 *   f_out      H x smoothed mean at every step = K (K + S)^-1 z, the new iterate;     v_out   its smoothed variance;
 *   alpha_out  (zs - f_out) / ss = K^-1 f_out, 0 at the NaN rows;
 *   zs_out, ss_out   the sites formed at f_out (what the next step takes as zs, ss);
 *   sums[6]    [0] the Gaussian log-likelihood of (zs, ss)      [1] sum lp(ys | f_out)      [2] sum f_out alpha_out
 *              [3] sum [lp - log N(zs_out | f_out, ss_out)]     [4] max |f_out - f_prev| over all steps (0 when f_prev is NULL)
 *              [5] the number of observed steps.
 * lp and [3] run over the observed steps.  The log of the Laplace evidence at a fixed point is [0] + [3] of consecutive passes.
 * The outputs must not overlap zs, ss, f_prev.  Workgroup partials are added in index order and the maximum is exact in any
 * order: equal calls give equal bits.  The smoothed states are not stored.  Four launches whatever N (pgps_set_chunk
 * honoured; pgps_set_one_launch and pgps_set_resident do not apply).
 *
 * pgps_lik_sites_*: the elementwise start and the damped steps: f = f_a + step (f_b - f_a), alpha likewise (f_b NULL: f_a, alpha_a
 * as they are), the sites at f, sums[3] = {sum lp, sum f alpha, sum [lp - log N(zs_out | f, ss_out)]}.  Outputs may be the
 * inputs' own arrays.  Two launches.
 *
 * The _dev forms take device pointers for every array and for sums and are asynchronous on the context's stream; the host forms
 * also check that ss is finite and > 0 wherever zs is observed (PGPS_E_INVALID) and return PGPS_E_NUMERIC on a non-finite sum.
 * A null pointer (f_prev, f_b, alpha_b excepted), N < 1, lam <= 0, an unknown lik, a Gaussian or Poisson par that is not finite
 * and > 0: PGPS_E_INVALID; d outside 1..3: PGPS_E_UNSUPPORTED_DIM. */
#define PGPS_LIK_GAUSSIAN 0         /* y ~ N(f, par) */
#define PGPS_LIK_BERNOULLI_LOGIT 1  /* y in {0, 1}, p(y = 1) = 1 / (1 + exp(-f)); par unused */
#define PGPS_LIK_POISSON_EXP 2      /* y ~ Poisson(par exp(f)); lp leaves out -lgamma(y + 1) */
int pgps_gp_newton_f64(pgps_ctx*, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                       const double* H, int lik, double par, const double* ts, const double* ys, const double* zs,
                       const double* ss, const double* f_prev /* may be NULL */, double t0, double* f_out, double* v_out,
                       double* alpha_out, double* zs_out, double* ss_out, double* sums /* 6 */);
int pgps_gp_newton_dev_f64(pgps_ctx*, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                           const double* H, int lik, double par, const double* ts, const double* ys, const double* zs,
                           const double* ss, const double* f_prev /* may be NULL */, double t0, double* f_out, double* v_out,
                           double* alpha_out, double* zs_out, double* ss_out, double* sums /* 6 */);
int pgps_lik_sites_f64(pgps_ctx*, long N, int lik, double par, const double* ys, const double* f_a, const double* alpha_a,
                       const double* f_b /* may be NULL */, const double* alpha_b /* may be NULL */, double step, double* f_out,
                       double* alpha_out, double* zs_out, double* ss_out, double* sums /* 3 */);
int pgps_lik_sites_dev_f64(pgps_ctx*, long N, int lik, double par, const double* ys, const double* f_a, const double* alpha_a,
                           const double* f_b /* may be NULL */, const double* alpha_b /* may be NULL */, double step,
                           double* f_out, double* alpha_out, double* zs_out, double* ss_out, double* sums /* 3 */);

/* ---- Laplace inference for a panel: the mode search of S series in ONE launch (fused path, fp64, d <= 3) -------
 * The data of Laplace inference is usually a panel (spike trains of many neurons, counts per patient or sensor): S series cut
 * out of concatenated ts, ys by offs as the pgps_gp_panel_* calls take them, one likelihood `lik`.  pgps_gp_panel_laplace_*
 * gives every series ONE workgroup that runs the WHOLE damped Newton search from f = 0 inside the kernel -- start, passes
 * (the three bodies of pgps_gp_newton_* back to back), halvings, accept, the closing pass -- with its own iteration count;
 * nothing comes back before the mode is found.  The rule is csrc/pgps_newton.h: a proposal is accepted when its Psi is finite
 * and >= Psi - 1e-12 |Psi|, else halved (at most 20 times per step); converged when a pass moves f by <= tol; unconverged
 * after max_iter steps the last iterate is kept.  At most max_iter + 1 passes and 20 max_iter damped updates per series.
 *   models   the panel's table, nmodels = 1 or S rows [lam | N1 | N2 | Pinf | H | R]; R is IGNORED and taken as 0
 *   pars     HOST, npars = 1 or S likelihood parameters (Poisson: the exposure of series s; Bernoulli: unused)
 *   f, v, zs, ss   (offs[S]) each, in the rows' order: the mode, its variances, the sites at the mode (zs NaN and ss 1 at the
 *            missing rows, as pgps_gp_newton_* leaves them)
 *   info     (S, 8): [ll_sites | corr | psi | iterations | halvings | converged (0 / 1) | last move | observed rows].  The log of
 *            the Laplace evidence is ll_sites + corr plus the likelihood's constant, which the caller adds.
 * pgps_gp_panel_laplace_grad_*: from (f, v, zs, ss) of the call above, the three observation arrays of the identity
 * grad log q = grad [G(z + w) - G(w) + G(0)], w = v d3 / (2 W), three launches of the panel's adjoint pass with rs = ss, R = 0,
 * and their combination on the device: out (S, 1 + d d + 2 d + 1) rows [c | Abar | Ubar | Hbar | Rbar] as
 * pgps_gp_panel_ll_grad_* lays them out.  The first column c is the COMBINATION G(z + w) - G(w) + G(0), not the evidence.
 * Prediction needs no entry point of its own: pgps_gp_panel_predict_dev_f64 with ys = zs, rs = ss and R = 0 in the table.
 * Host forms take host arrays and return PGPS_E_NUMERIC where an info row (the first column of an out row) is not finite;
 * _dev forms take device pointers for everything but offs / models / pars, synchronise the context's stream ONCE to copy their
 * tables in and are asynchronous afterwards.  Steps per lane, groups and bit-repeatability as the pgps_gp_panel_* calls.
 * Profiling: the search kernel has no timer slot of its own.  pgps_profile_* charge a whole search (and the gradient's input
 * kernel) to PGPS_K_SMOOTHER_APPLY, the adjoint passes to PGPS_K_FILTER_APPLY and the combination to PGPS_K_LL_FINALIZE; the
 * roctx ranges are "laplace_panel_search" and "laplace_panel_grad".
 * Errors (no output is touched): S < 1, a null pointer, an empty series, a series above PGPS_PANEL_MAX_STEPS, nmodels or npars
 * not 1 or S, lam <= 0 in a row, an unknown lik, a Gaussian or Poisson par that is not finite and > 0, tol not finite or < 0,
 * max_iter outside 1 .. 1000: PGPS_E_INVALID; d outside 1..3: PGPS_E_UNSUPPORTED_DIM. */
int pgps_gp_panel_laplace_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, int lik, int npars,
                              const double* pars, const double* ts, const double* ys, double tol, int max_iter, double* f,
                              double* v, double* zs, double* ss, double* info /* S 8 */);
int pgps_gp_panel_laplace_dev_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, int lik,
                                  int npars, const double* pars, const double* ts, const double* ys, double tol, int max_iter,
                                  double* f, double* v, double* zs, double* ss, double* info /* S 8 */);
int pgps_gp_panel_laplace_grad_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, int lik,
                                   int npars, const double* pars, const double* ts, const double* ys, const double* f,
                                   const double* v, const double* zs, const double* ss, double* out);
int pgps_gp_panel_laplace_grad_dev_f64(pgps_ctx*, long S, const long* offs, int d, int nmodels, const double* models, int lik,
                                       int npars, const double* pars, const double* ts, const double* ys, const double* f,
                                       const double* v, const double* zs, const double* ss, double* out);

/* ---- the hyper-parameter fit of every series of a panel in ONE launch (fused path, fp64, d <= 3) --------
 * What a survey does with a panel is fit every light curve's own variance, lengthscale and noise variance.  pgps_gp_panel_fit_*
 * gives every series ONE workgroup that runs the WHOLE search inside the kernel: each evaluation forms the fused model of a
 * single Matern-1/2, -3/2 or -5/2 kernel (d = 1, 2, 3) in registers from theta = (variance, lengthscales, noise_variance),
 * runs the three bodies of pgps_gp_panel_ll_grad_* back to back on the series' own scratch and contracts the adjoints to
 * f = -ll / max(1, n_obs) and its gradient in x = log theta; nothing comes back before the search has ended.  The rule is
 * csrc/pgps_fit.h: BFGS on the inverse matrix with a backtracking Armijo search (c = 1e-4, at most 21 trials, a trial that is
 * no descent step is skipped without an evaluation) and projection onto the box lo <= theta <= hi; converged when the
 * projected gradient's largest component is <= gtol.  At most 1 + 42 max_iter evaluations per series.
 *   unit     HOST, ONE model row [lam | N1 | N2 | Pinf | H | R] as the panel's tables hold them: the Matern-5/2 SDE at lam = 1,
 *            variance 1 (F = lam F1, Pinf = s2 P1, H = H1).  Read at d = 3 only (may be NULL at d = 1, 2); R is ignored
 *   rs       per-observation noise variances (the step's variance is noise_variance + rs[k]), or NULL
 *   theta0, lo, hi   HOST (S, 3): every series' start and box, in theta
 *   free3    HOST (3): a coordinate with free3[i] = 0 keeps theta0[s, i] exactly (never through log / exp; lo, hi unread).  A
 *            fixed noise_variance may be 0 where rs is given
 *   thetas   (S, 3): the last accepted iterate.  A coordinate that never moved is theta0 bit for bit, one that ended on a bound
 *            is that bound bit for bit
 *   info     (S, 8): [ll | ll at the start | iterations | evaluations | status | max |q| | observed rows | 0];  status 0 converged,
 *            1 max_iter iterations made, 2 the line search failed, 3 f or g not finite at the start (max |q| is then NaN).  A
 *            series without an observed row returns its start with status 0 and 0 iterations.
 * The host form takes host arrays and returns PGPS_E_NUMERIC (outputs written) where a series' ll is not finite; the _dev form
 * takes device pointers for ts, ys, rs, thetas, info, synchronises the context's stream ONCE to copy its tables in and is
 * asynchronous afterwards.  Steps per lane, groups and bit-repeatability as the pgps_gp_panel_* calls: a row's bits depend on
 * that series alone.
 * Profiling: the search kernel has no timer slot of its own; pgps_profile_* charge a whole search to PGPS_K_FILTER_APPLY; the
 * roctx range is "panel_fit".
 * Errors (no output is touched): S < 1, a null pointer (unit at d = 3), an empty series, a series above PGPS_PANEL_MAX_STEPS,
 * lam <= 0 in the unit row at d = 3, a free coordinate whose theta0, lo or hi is not finite and > 0 or whose lo >= hi, a fixed
 * variance or lengthscale that is not finite and > 0, a fixed noise_variance that is not finite, < 0, or <= 0 without rs, gtol not
 * finite or < 0, max_iter outside 1 .. 200: PGPS_E_INVALID (the host form also: rs not finite, < 0, or noise_variance + rs <= 0
 * with a fixed noise_variance, at an observed row); d outside 1..3: PGPS_E_UNSUPPORTED_DIM. */
int pgps_gp_panel_fit_f64(pgps_ctx*, long S, const long* offs, int d, const double* unit, const double* ts, const double* ys,
                          const double* rs, const double* theta0, const double* lo, const double* hi, const int* free3,
                          double gtol, int max_iter, double* thetas /* S 3 */, double* info /* S 8 */);
int pgps_gp_panel_fit_dev_f64(pgps_ctx*, long S, const long* offs, int d, const double* unit, const double* ts, const double* ys,
                              const double* rs, const double* theta0, const double* lo, const double* hi, const int* free3,
                              double gtol, int max_iter, double* thetas /* S 3 */, double* info /* S 8 */);

/* ---- sequential mode: pssgp/kalman/sequential.py:11-73 (kf, ks) ------------------------
 * StateSpaceGP(parallel=False).  Host arithmetic on HOST pointers, as in the reference (its
 * sequential mode is the CPU `tf.scan`).  No context needed.  mps / Pps (predicted moments,
 * return_predicted=True) and ll may be NULL in kf. */
int pgps_seq_kf_f64(long N, int d, const double* P0, const double* Fs, const double* Qs, const double* H,
                    double R, const double* ys, double* fms, double* fPs, double* ll, double* mps, double* Pps);
int pgps_seq_kf_f32(long N, int d, const float* P0, const float* Fs, const float* Qs, const float* H, float R,
                    const float* ys, float* fms, float* fPs, double* ll, float* mps, float* Pps);
/* ... with the noise variance of EVERY step, Rs (N), in place of R (read where ys[k] is not NaN only; null: PGPS_E_INVALID) */
int pgps_seq_kf_het_f64(long N, int d, const double* P0, const double* Fs, const double* Qs, const double* H,
                        const double* Rs, const double* ys, double* fms, double* fPs, double* ll, double* mps, double* Pps);
int pgps_seq_kf_het_f32(long N, int d, const float* P0, const float* Fs, const float* Qs, const float* H, const float* Rs,
                        const float* ys, float* fms, float* fPs, double* ll, float* mps, float* Pps);
int pgps_seq_ks_f64(long N, int d, const double* Fs, const double* ms, const double* Ps, const double* mps,
                    const double* Pps, double* sms, double* sPs);
int pgps_seq_ks_f32(long N, int d, const float* Fs, const float* ms, const float* Ps, const float* mps,
                    const float* Pps, float* sms, float* sPs);
/* host twins of the sampler (any d <= PGPS_MAX_DIM): the same definition and the same draws as pgps_pks_sample_* /
 * pgps_sample_normals_dev_*, host pointers, no context */
int pgps_seq_ks_sample_f64(long N, int d, const double* Fs, const double* Qs, const double* fms, const double* fPs, int S,
                           long s0, unsigned long long seed, const double* z, const double* H, double* out);
int pgps_seq_ks_sample_f32(long N, int d, const float* Fs, const float* Qs, const float* fms, const float* fPs, int S,
                           long s0, unsigned long long seed, const float* z, const float* H, float* out);
int pgps_seq_sample_normals_f64(long N, int d, int S, long s0, unsigned long long seed, double* z);
int pgps_seq_sample_normals_f32(long N, int d, int S, long s0, unsigned long long seed, float* z);
/* host twin of pgps_pks_cov_* (any d <= PGPS_MAX_DIM): the same definition, host pointers, no context */
int pgps_seq_ks_cov_f64(long N, int d, const double* Fs, const double* Qs, const double* fPs, const double* sPs, long n,
                        const long* sel, const double* H, double* out);
int pgps_seq_ks_cov_f32(long N, int d, const float* Fs, const float* Qs, const float* fPs, const float* sPs, long n,
                        const long* sel, const float* H, float* out);

/* ---- host helper: the balancing sweep of balance_ss (pssgp/kernels/math_utils.py:10-29, numba in the reference) ----
 * scale[d] = accumulated diagonal scaling after n_iter sweeps over F (d,d).  Host pointers, no context. */
int pgps_host_balance_f64(int d, const double* F, int n_iter, double* scale);

/* ---- a series kept on the device across calls (round 3) ------------------------------------------------------------
 * What the reference's drivers do thousands of times per run is evaluate ONE (ts, ys) at changing hyper-parameters
 * (StateSpaceGP.maximum_log_likelihood_objective / training_loss under L-BFGS and HMC: pssgp/model.py:113-117 called from
 * pssgp/experiments/sunspot/map.py:74-82, experiments/common.py:95-133) and predict on a fixed grid (predict_f,
 * pssgp/model.py:92-111 from toy_models/speed_and_stability.py:73-87).  A pgps_series holds ts, ys -- and the query grid
 * merged with them by _merge_sorted's rule (pssgp/model.py:15-55) -- on the device, so a call moves the model's scalars
 * in and the results out, nothing else.  fp64; the fused (Matern-family, d <= 3) model of pgps_gp_*: F = -lam I + N1,
 * N2 = N1^2 / 2, Pinf, H, R.  The handle belongs to its context (one in-flight call per context); destroy it before it. */
typedef struct pgps_series pgps_series;
int pgps_series_create_f64(pgps_ctx* ctx, long N, const double* ts, const double* ys, double t0, pgps_series** out);
int pgps_series_set_queries_f64(pgps_series* s, long K, const double* tq);     /* sorted query times; K = 0 drops them */
int pgps_series_info(pgps_series* s, long* N, long* K);
int pgps_series_destroy(pgps_series* s);
/* results are on the HOST when these return (they synchronise the context's stream) */
int pgps_series_gp_ll_f64(pgps_series* s, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                          const double* H, double R, double* ll);
int pgps_series_gp_ll_grad_f64(pgps_series* s, int d, int np, const double* model, double* out /* 1 + np */);
int pgps_series_gp_predict_f64(pgps_series* s, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                               const double* H, double R, double* mean /* K */, double* var /* K */, double* ll /* or NULL */);
/* pgps_gp_predict_batch_f64 on a resident series with its query grid set (pgps_series_set_queries_f64).  w == NULL: mean, var receive
 * (B, K); w = B mixture weights (host, used as given): the (B, K) results stay on the device and mean, var receive the K
 * moments of the mixture (pgps_mix_moments_dev_f64). */
int pgps_series_gp_predict_batch_f64(pgps_series* s, int B, int d, const double* models, const double* w, double* mean,
                                     double* var, double* ll /* B, or NULL */);
int pgps_series_lti_predict_batch_f64(pgps_series* s, int B, int d, const double* models /* [F | Pinf | H | R] */, const double* w,
                                      double* mean, double* var, double* ll /* B, or NULL */);
/* Log-likelihood and the ADJOINTS of the fused model by one filter pass and one reverse pass (csrc/pgps_gpadj.hip.h; the
 * lane-chunk twin of pgps_lti_ll_grad_*): out = [ll | Abar (d d, row-major) | Ubar (d) | Hbar (d) | Rbar], 1 + d d + 2 d + 1
 * doubles, with  d ll / d theta = <Abar, dF> + Ubar^T dPinf H^T + Hbar . dH + Rbar dR  for every dF that commutes with F -- for
 * the Matern family: dF = -F / lengthscale, dPinf = Pinf / variance.  What the reference takes from tf.GradientTape over
 * maximum_log_likelihood_objective (tests/test_gp_vs_kfs.py:53-78; pssgp/kalman/parallel.py:121-152 differentiated), at
 * the cost of about two likelihoods whatever the number of hyper-parameters.  fp64, d <= 3.  The _dev form takes device
 * pointers ts, ys, out and is asynchronous on the context's stream. */
int pgps_series_gp_ll_grad_adj_f64(pgps_series* s, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                                   const double* H, double R, double* out /* 1 + d d + 2 d + 1 */);
int pgps_gp_ll_grad_adj_dev_f64(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2,
                                const double* Pinf, const double* H, double R, const double* ts, double t0, const double* ys,
                                double* out);
/* The same at B hyper-parameter settings over one series in one set of launches: `models` (HOST memory) as
 * pgps_gp_ll_batch_* takes it, B rows [lam | N1 | N2 | Pinf | H | R]; out (B, 1 + d d + 2 d + 1), row b what
 * pgps_gp_ll_grad_adj_dev_f64 returns for model b.  One workgroup per model in ONE launch where the single call takes its
 * one-launch form, four launches of (workgroups, models) grids otherwise; steps per lane are fixed once per call from (B, N)
 * (pgps_set_chunk honoured) and the models run in groups that fit pgps_set_batch_scratch, so a row does not depend on its
 * place in the table, on the other rows or on the groups.  The _dev form takes device pointers ts, ys, out, synchronises the
 * stream once to copy the table in, and is asynchronous afterwards.  B or N < 1, a null pointer, lam <= 0 or R <= 0 in a
 * row: PGPS_E_INVALID; d outside 1..3: PGPS_E_UNSUPPORTED_DIM; host forms: a non-finite ll in a row: PGPS_E_NUMERIC. */
int pgps_gp_ll_grad_adj_batch_f64(pgps_ctx* ctx, int B, long N, int d, const double* models, const double* ts, double t0,
                                  const double* ys, double* out);
int pgps_gp_ll_grad_adj_batch_dev_f64(pgps_ctx* ctx, int B, long N, int d, const double* models, const double* ts, double t0,
                                      const double* ys, double* out);
int pgps_series_gp_ll_grad_adj_batch_f64(pgps_series* s, int B, int d, const double* models, double* out);
/* ... and for B general LTI models on the row-cooperative kernels (fp64, 2 <= d <= 16; other d: PGPS_E_UNSUPPORTED_DIM):
 * `models` (HOST memory) as pgps_lti_ll_batch_* takes it, B rows [F | Pinf | H | R]; out (B, 1 + d d + 2 d + 1), row b what
 * pgps_lti_ll_grad_dev_f64 returns for model b.  The chain length is fixed once per call from (B, N) (pgps_set_chunk
 * honoured); the models run in groups under the batch budget (default 1 GiB; about 2 N d d doubles per model).  Errors as
 * above (R <= 0 in a row: PGPS_E_INVALID). */
int pgps_lti_ll_grad_batch_f64(pgps_ctx* ctx, int B, long N, int d, const double* models, const double* ts, const double* ys,
                               double t0, double* out);
int pgps_lti_ll_grad_batch_dev_f64(pgps_ctx* ctx, int B, long N, int d, const double* models, const double* ts,
                                   const double* ys, double t0, double* out);
int pgps_series_lti_ll_grad_batch_f64(pgps_series* s, int B, int d, const double* models, double* out);
/* ... and for ANY kernel's LTI model (F, Pinf, H: host pointers; fp64, 2 <= d <= PGPS_MAX_DIM): pgps_lti_ll_f64 /
 * pgps_lti_predict_f64 / pgps_lti_ll_batch_f64 (models: B rows [F | Pinf | H | R], d <= 16) on the resident series and its
 * merged query grid -- the evaluation loop of an optimiser or sampler over an RBF / Periodic / composite kernel. */
int pgps_series_lti_ll_f64(pgps_series* s, int d, const double* F, const double* Pinf, const double* H, double R, double* ll);
int pgps_series_lti_predict_f64(pgps_series* s, int d, const double* F, const double* Pinf, const double* H, double R,
                                double* mean /* K */, double* var /* K */, double* ll /* or NULL */);
int pgps_series_lti_ll_batch_f64(pgps_series* s, int B, int d, const double* models, double* ll /* B */);

/* ---- log-likelihood AND its gradient for any kernel's LTI model, in two passes (round 4) ---------------------------
 * What the reference obtains from tf.GradientTape over maximum_log_likelihood_objective (tests/test_gp_vs_kfs.py:53-78;
 * pssgp/model.py:113-117 through pssgp/kalman/parallel.py:121-152 and pssgp/kernels/base.py:29-47), consumed by its
 * L-BFGS and HMC drivers (pssgp/experiments/sunspot/map.py:74-82, experiments/common.py:95-133): one filter pass and
 * one reverse (adjoint) pass return the adjoints of the MODEL, whatever the number of hyper-parameters:
 *   out[0]                    ll
 *   out[1 .. d d]             Abar (d, d) row-major = sum_k dt_k Fbar_k F_k^T : d ll / d theta gets <Abar, dF> for every
 *                             dF = dF/dtheta that commutes with F (d expm(dt F) = dt dF expm(dt F); true of every
 *                             hyper-parameter of every kernel of the reference in a frozen state basis -- time scalings of
 *                             block / Kronecker factors: pssgp/kernels/sde_grads.py)
 *   out[1 + d d ..]           Ubar (d):  d ll / d Pinf = sym(Ubar H), i.e. + Ubar^T dPinf H^T
 *   out[1 + d d + d ..]       Hbar (d):  + Hbar . dH
 *   out[1 + d d + 2 d]        Rbar    :  + Rbar dR
 * (1 + d d + 2 d + 1 doubles).  F, Pinf (stationary: F Pinf + Pinf F^T + L Q L^T = 0), H from HOST memory; ts, ys host
 * pointers for the plain entry point, device pointers for _dev (out device too: asynchronous on the context's stream);
 * the series entry point leaves `out` on the host.  fp64, 2 <= d <= PGPS_MAX_DIM. */
int pgps_lti_ll_grad_f64(pgps_ctx*, long N, int d, const double* F, const double* Pinf, const double* H, double R,
                         const double* ts, const double* ys, double t0, double* out);
int pgps_lti_ll_grad_dev_f64(pgps_ctx*, long N, int d, const double* F, const double* Pinf, const double* H, double R,
                             const double* ts, const double* ys, double t0, double* out);
int pgps_series_lti_ll_grad_f64(pgps_series* s, int d, const double* F, const double* Pinf, const double* H, double R,
                                double* out);

/* ---- several outputs on one clock (fused path, fp64, d <= 3) ---------------------------------------------------------
 * ys (N, M) row-major: M independent GPs that share the kernel, the noise and the inputs (GPflow's Y (N, M) with
 * num_latent_gps = M).  Covariances, gains and innovation variances do not depend on y, so ONE covariance pass serves the M
 * columns: the scan runs on column-tiled elements (shared A, C, J plus a tile of (b, eta) pairs; csrc/pgps_multi.hip.h) and
 * reads the times, merges and discretises once per tile instead of once per column.
 *   ll    (M,)    log-likelihood of every column (NULL allowed in the predict calls)
 *   mean  (K, M)  row-major posterior means at the sorted query times tq (merged as in pgps_gp_predict_*)
 *   var   (K,)    posterior variance: the same for every column
 * A row of ys is observed in all columns or missing (NaN) in all columns.  The host-array forms check that (a mixed row:
 * PGPS_E_INVALID) and return PGPS_E_NUMERIC when some ll[j] is not finite; for the _dev forms (device pointers for ts, ys,
 * tq, mean, var, ll; they return with the launches enqueued) it is a PRECONDITION: a step counts as missing when the first
 * column of a tile is NaN, and a NaN in another column of an observed row makes that column's results (and its ll)
 * non-finite and leaves the other columns untouched.  Column j equals pgps_gp_predict_* on column j up to rounding (another
 * bracketing of the same scans); a column's result depends neither on the other columns' data nor on its position; repeated
 * calls agree bit for bit (no floating-point atomics).  When the filtered means of all columns exceed the batch budget
 * (pgps_set_batch_scratch) the column tiles run in rounds.  Errors: M, N, K < 1, a null pointer, R <= 0, lam <= 0,
 * N + K >= 2^31: PGPS_E_INVALID; d outside 1..3: PGPS_E_UNSUPPORTED_DIM. */
int pgps_gp_ll_multi_f64(pgps_ctx*, long N, int M, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                         const double* H, double R, const double* ts, const double* ys, double t0, double* ll);
int pgps_gp_ll_multi_dev_f64(pgps_ctx*, long N, int M, int d, double lam, const double* N1, const double* N2,
                             const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                             double* ll);
int pgps_gp_predict_multi_f64(pgps_ctx*, long N, long K, int M, int d, double lam, const double* N1, const double* N2,
                              const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                              const double* tq, double* mean, double* var, double* ll);
int pgps_gp_predict_multi_dev_f64(pgps_ctx*, long N, long K, int M, int d, double lam, const double* N1, const double* N2,
                                  const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                  double t0, const double* tq, double* mean, double* var, double* ll);
/* Log-likelihoods and the model's adjoints of the M columns in ONE filter pass and ONE reverse pass (csrc/pgps_multi_grad.hip.h):
 *   out = [ll (M) | Abar (d d) | Ubar (d) | Hbar (d) | Rbar]
 * ll[j] as pgps_gp_ll_multi_*; the statistics are those of pgps_series_gp_ll_grad_adj_f64 SUMMED over the columns, i.e. the
 * adjoints of sum_j ll[j] -- the contraction with the model's derivatives is linear in them (d ll / d l = -<Abar, F> / l,
 * d ll / d s2 = Ubar^T Pinf H^T / s2, d ll / d R = Rbar).  The reverse sweep carries one a = d ll / d m per column and ONE
 * B = d ll / d P for the tile, so its matrix work is done once per tile of columns.  Rows of ys, errors and the _dev form
 * (device pointers for ts, ys, out; returns with the launches enqueued; all-or-none rows are a precondition) as above; the
 * host-array form returns PGPS_E_NUMERIC when some ll[j] is not finite.  Workgroup partials are summed in a fixed order: results
 * repeat bit for bit and do not depend on how pgps_set_batch_scratch splits the column tiles into rounds. */
int pgps_gp_ll_grad_multi_f64(pgps_ctx*, long N, int M, int d, double lam, const double* N1, const double* N2,
                              const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                              double* out);
int pgps_gp_ll_grad_multi_dev_f64(pgps_ctx*, long N, int M, int d, double lam, const double* N1, const double* N2,
                                  const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                                  double* out);
/* Whitened columns and their Gram matrix (csrc/pgps_whiten.hip.h).  With K_y = K + R I = L L^T on the observed rows in time
 * order, the standardised innovations of column c, w[k, c] = (ys[k, c] - mu_c[k]) / sqrt(S_k), are W = L^-1 ys: any quadratic
 * form a^T K_y^-1 b over the training points is a dot product of whitened columns, and gram = W^T W = ys^T K_y^-1 ys.
 *   w       (N, M)  row-major; 0.0 at the rows that are not observed
 *   gram    (M, M)  symmetric, gram[i, j] and gram[j, i] equal bit for bit; 1 <= M <= 16 (more: PGPS_E_INVALID).  W stays in
 *                   the context's scratch and never reaches the host
 *   logdet          sum of log S_k over the observed steps = log |K_y|: shared by the columns
 *   n_obs           number of observed steps
 * The Kalman pass is the one of pgps_gp_ll_multi_* (same scans, same rounds under pgps_set_batch_scratch) with the store of w
 * added; the Gram matrix is summed from per-workgroup partials in a fixed order (no floating-point atomics): results repeat
 * bit for bit.  Rows of ys, the other errors and the _dev forms (device pointers for ts, ys, w, gram, logdet, n_obs; they
 * return with the launches enqueued; all-or-none rows are a precondition) as above.  The host-array forms return
 * PGPS_E_NUMERIC when logdet or an entry of w / gram is not finite. */
int pgps_gp_whiten_multi_f64(pgps_ctx*, long N, int M, int d, double lam, const double* N1, const double* N2,
                             const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                             double* w, double* logdet, long* n_obs);
int pgps_gp_whiten_multi_dev_f64(pgps_ctx*, long N, int M, int d, double lam, const double* N1, const double* N2,
                                 const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                                 double* w, double* logdet, long* n_obs);
int pgps_gp_gram_multi_f64(pgps_ctx*, long N, int M, int d, double lam, const double* N1, const double* N2,
                           const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                           double* gram, double* logdet, long* n_obs);
int pgps_gp_gram_multi_dev_f64(pgps_ctx*, long N, int M, int d, double lam, const double* N1, const double* N2,
                               const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                               double* gram, double* logdet, long* n_obs);

#ifdef __cplusplus
}
#endif
#endif /* PGPS_H_ */
