// pgps_scan_api.hip -- the array path of the C ABI (include/pgps.h): which kernel family a scan takes, the float32
// dense-grid policy and the promotion of float32 calls to fp64 arithmetic, pkf / pks / pkfs / discretise on device and host
// arrays, and the segment protocol of a series sharded over GPUs.  The scan kernels live in the per-(dtype, d) units.
#include <chrono>

#include "pgps_host.h"
#include "pgps_wc_args.h"

using namespace pgps;

// fp32 <-> fp64 conversion passes (the discretisation kernels of 7 <= d <= 16 compute in fp64 whatever the series' type)
namespace pgps {
static __global__ void k_narrow(long n, const double* in, float* out) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = (float)in[i];
}
static __global__ void k_widen_many(ConvJobs j) {
    const float* in = (const float*)j.src[blockIdx.y];
    double* out = (double*)j.dst[blockIdx.y];
    const long n = j.n[blockIdx.y];
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = (double)in[i];
}
static __global__ void k_narrow_many(ConvJobs j) {
    const double* in = (const double*)j.src[blockIdx.y];
    float* out = (float*)j.dst[blockIdx.y];
    const long n = j.n[blockIdx.y];
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = (float)in[i];
}

void WideConv::add(const void* src, void* dst, size_t n) {
    if (!src || !dst || !n) return;
    jobs_.src[nj_] = src; jobs_.dst[nj_] = dst; jobs_.n[nj_] = (long)n;
    most_ = std::max(most_, n);
    ++nj_;
}
void WideConv::widen() {
    if (nj_) hipLaunchKernelGGL(k_widen_many, grid(most_, nj_), dim3(256), 0, ctx_->stream, jobs_);
    nj_ = 0; most_ = 0;
}
void WideConv::narrow() {
    if (nj_) hipLaunchKernelGGL(k_narrow_many, grid(most_, nj_), dim3(256), 0, ctx_->stream, jobs_);
    nj_ = 0; most_ = 0;
}
void WideConv::narrow_one(const double* src, float* dst, size_t n) {
    hipLaunchKernelGGL(k_narrow, grid(n, 1), dim3(256), 0, ctx_->stream, (long)n, src, dst);
}
int WideConv::finish(bool promoted) {
    HIPCHK(ctx_, hipGetLastError());
    if (promoted) ctx_->host_flags |= PGPS_STATUS_F32_PROMOTED;
    return PGPS_OK;
}
}  // namespace pgps

// Which kernel family a scan call of N steps at state dimension d takes (PGPS_FAMILY_*, include/pgps.h): the ONE place
// that decides -- dispatch_scan launches what this returns, pgps_get_family reports it (bench.py names the measured
// kernels from it instead of repeating the rule).
template <typename T>
static int choose_family(const pgps_ctx* ctx, int d, long N, Mode mode) {
    const bool rc_ok = d >= rc::kDimMin && d <= rc::kDimMax;
    if constexpr (sizeof(T) == 4) {
        // row-cooperative family in fp32: its own instantiations (16-lane rows, v_fmac_f32_dpp), every mode; automatic
        // above the lane-chunk kernels' range (at d = 6 those still win in fp32: 0.71 against 0.85 ms at 2^20 steps)
        bool to_rc = rc_ok && (ctx->family == 3 || ((ctx->family == 0 || ctx->family == 4) && d > PGPS_MAX_DIM_LANE));
        // d = 6, whole-series filter / filter + smoother: the quad-cooperative kernels are ahead of the lane-chunk ones on
        // short series; from 2^19 steps the lane-chunk kernels' workgroups span >= 2048 steps and take their carries by the
        // forgetting shortcut (round 5), which put them ahead at every longer size (same box, ms per pass, lane-chunk / quad,
        // profiles/r05_d6_crossover.txt: 2^14 0.177 / 0.128, 2^16 0.191 / 0.146, 2^17 0.202 / 0.182, 2^18 0.245 / 0.222,
        // 2^19 0.258 / 0.354, 2^20 0.549 / 0.628, 2^21 1.042 / 1.163, 2^22 2.039 / 2.204; round 4, without the shortcut:
        // 2^19 0.395 / 0.398, 2^20 0.627 / 0.650, 2^21 1.266 / 1.217, 2^22 2.566 / 2.357)
        if (ctx->family == 0 && d == 6 && (mode == MODE_PKF || mode == MODE_PKFS) && ctx->chunk == 0 && ctx->stage_g < 0 &&
            N <= (3L << 17) && N >= 64)
            to_rc = true;
        // quad-cooperative level-1 kernels under the row-cooperative driver: family 4 (fp32, 5 <= d <= 8)
        if (ctx->family == 4) {
            if (d < qc::kDimMin || d > qc::kDimMax || mode == MODE_PKS) return PGPS_E_UNSUPPORTED_DIM;
            to_rc = true;
        }
        if (to_rc) {
            // (what scan_rc_entry then decides: the quad level-1 kernels at d = 8 and, where this rule sends it there, d = 6)
            const bool quad = (ctx->family == 4 || (ctx->family == 0 && (d == 8 || d == 6))) && d >= qc::kDimMin && d <= qc::kDimMax &&
                              mode != MODE_PKS;
            return quad ? PGPS_FAMILY_QUAD : PGPS_FAMILY_ROW;
        }
    }
    if constexpr (sizeof(T) == 8) {
        // filter + smoother of a whole series that fits the chip: one resident launch (pgps_resident.hip.h)
        if ((mode == MODE_PKFS || mode == MODE_PKF) && resident_fits(ctx, N, d, false)) return PGPS_FAMILY_RESIDENT;
        // row-cooperative family: fp64, d <= 16, whole-series filter / filter+smoother
        const bool whole = mode == MODE_PKF || mode == MODE_PKFS || mode == MODE_PKS;
        // automatic choice from d = 5: at d = 6 the lane-chunk kernels spill (2^18 steps: 1.29 ms against 0.53 ms);
        // the segment protocol (multi-GPU) moves over where the lane-chunk family ends
        if (rc_ok && (ctx->family == 3 || (ctx->family == 0 && (whole ? d >= 5 : d > PGPS_MAX_DIM_LANE)))) return PGPS_FAMILY_ROW;
    }
    if (ctx->family == 3) return PGPS_E_UNSUPPORTED_DIM;
    if (ctx->family == 2 || (ctx->family == 0 && d > PGPS_MAX_DIM_LANE)) {
        if (d > 32 || mode == MODE_PKS) return PGPS_E_UNSUPPORTED_DIM;
        return (wc::rc2_covers<T>(d) && ctx->wc_rows2) ? PGPS_FAMILY_TWO_ROWS : PGPS_FAMILY_WAVE;
    }
    if (d < 1 || d > PGPS_MAX_DIM_LANE) return PGPS_E_UNSUPPORTED_DIM;
    // Lane-chunk family: whole-series calls run the build with 128-lane workgroups (pgps_inst.hip, PGPS_NARROW) --
    // except the long series of the LDS-staged dimensions: from 2^22 steps there are two waves per SIMD to cover each
    // other's loads, and the narrow build's prefetch registers cost it that (d = 2, 2^22 steps: 0.303 ms against 0.307 for
    // 256 lanes; 2^24: 1.28 against 1.25).  The three phases of the segment protocol follow the same rule (it depends on
    // this rank's N and d only, so they agree with each other: a rank's 2^21 steps of c4 0.152 -> 0.147 ms).
    return lane_narrow(ctx, d, N) ? PGPS_FAMILY_LANE_NARROW : PGPS_FAMILY_LANE;
}

template <typename T>
static int dispatch_scan(pgps_ctx* ctx, int d, const ScanArgs<T>& a, Mode mode) {
    int fam = choose_family<T>(ctx, d, a.N, mode);
    if (fam < 0) return fam;
    if constexpr (sizeof(T) == 8) {
        if (fam == PGPS_FAMILY_RESIDENT) {
            if (aligned16(a.ys)) {
                ResArgs<double> ra{};
                ra.s = a;
                return launch_resident<double, 2>(ctx, ra, false, mode == MODE_PKFS);
            }
            fam = lane_narrow(ctx, d, a.N) ? PGPS_FAMILY_LANE_NARROW : PGPS_FAMILY_LANE;      // (a misaligned ys: three launches)
        }
    }
    if (fam == PGPS_FAMILY_ROW || fam == PGPS_FAMILY_QUAD) return launch_scan_rc<T>(ctx, a, d, mode);
    if (fam == PGPS_FAMILY_WAVE || fam == PGPS_FAMILY_TWO_ROWS) return launch_scan_wc<T>(ctx, a, d, mode);
    if (fam == PGPS_FAMILY_LANE_NARROW) return for_dim<1, 6>(d, [&](auto D) { return launch_scan_narrow<T, D()>(ctx, a, mode); });
    return for_dim<1, 6>(d, [&](auto D) { return launch_scan<T, D()>(ctx, a, mode); });
}

// `what`: 0 = pkf, 1 = pks, 2 = pkfs, 3 = a phase of the segment protocol; fp64 unless f32 != 0
extern "C" int pgps_get_family(pgps_ctx* ctx, long N, int d, int f32, int what, int* family) {
    if (!ctx || N < 1 || !family || what < 0 || what > 3) return PGPS_E_INVALID;
    const Mode mode = what == 0 ? MODE_PKF : what == 1 ? MODE_PKS : what == 2 ? MODE_PKFS : MODE_SEG_FILTER;
    const int fam = f32 ? choose_family<float>(ctx, d, N, mode) : choose_family<double>(ctx, d, N, mode);
    if (fam < 0) return fam;
    *family = fam;
    return PGPS_OK;
}


// ---------------------------------------------------------------------------------------------
// float32 series on DENSE grids: fp64 arithmetic behind float32 arrays, chosen per call.
// The reference's speed protocol takes --dtype (pssgp/experiments/toy_models/speed_and_stability.py:68) on
// np.linspace(0, 4, N) (toy_models/common.py:31-32): at 2^20 points F_k is the identity to five digits, and the smoothing
// elements' L = P - E Pp E^T (pssgp/kalman/parallel.py:159-166) -- like the sequential form P + G (sP' - Pp) G^T of
// sequential.py:57-61 -- is a difference of nearly equal matrices behind a solve with cond(Pp) ~ 1e5: float32 ARITHMETIC
// misses the north star's 1e-3 there whatever the kernel family (profiles/r03_fp32_reference_grid.txt), while fp64
// arithmetic on the float32 ARRAYS holds 1e-4 (profiles/r04_fp32_reference_grid.txt: the rounding of the inputs is not
// the problem).  So calls that run a smoother (pkfs, pks) on float32 arrays probe the grid first: a few thousand
// transition matrices spread over the series, ||F_k - I||_max against a threshold that grows with the state dimension
// (the error of the float32 smoother does: measured at d = 2, 3, 6); when an eighth of them or more are that close to the
// identity, the arrays are widened into scratch, the fp64 kernels run, the results are rounded back -- and
// pgps_status reports PGPS_STATUS_F32_PROMOTED.  pgps_set_f32_policy(ctx, 1) keeps float32 arithmetic whatever the
// grid, 2 always widens.  Filter-only calls (pkf) hold 1e-3 natively on every grid measured and are never probed.
// ---------------------------------------------------------------------------------------------
namespace pgps {
// ONE workgroup of 1024 lanes: sixteen lanes share a sampled transition matrix (consecutive lanes read consecutive entries:
// whole 64-byte segments -- one lane per matrix made every load instruction touch 64 cache lines, 17 us of one CU's address
// unit for 1024 samples), kProbeRounds samples per group; the count of dense samples comes out of a workgroup reduction -- no
// inter-workgroup atomics, no counters to reset.  result[1] = the count, then result[0] = the call's sequence number
// (system-scope release): the host spins on that word, no event involved.
constexpr int kProbeGroup = 16, kProbeRounds = 4, kProbeSamples = 1024 / kProbeGroup * kProbeRounds;
static __global__ __launch_bounds__(1024) void k_f32_probe(long N, int d, const float* __restrict__ Fs, float tau, long stride,
                                                             int nsamp, int* result, int seq) {
    const int g = threadIdx.x / kProbeGroup, j = threadIdx.x % kProbeGroup;
    const int dd = d * d;
    int dense = 0;
    for (int r = 0; r < kProbeRounds; ++r) {
        const int s = r * (1024 / kProbeGroup) + g;
        float m = 0.f;
        if (s < nsamp) {
            long k = 1 + (long)s * stride;          // (step 0 spans t0 .. t_0: whatever the grid, it may be long)
            if (k >= N) k = N - 1;
            const float* F = Fs + k * (long)dd;
            for (int e = j; e < dd; e += kProbeGroup) m = fmaxf(m, fabsf(F[e] - ((e / d == e % d) ? 1.f : 0.f)));
        }
        for (int o = kProbeGroup / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, kProbeGroup));
        dense += (j == 0 && s < nsamp && m < tau) ? 1 : 0;
    }
    // (a lane's count is 0..kProbeRounds: sum them over the workgroup)
    int total = 0;
    for (int c = 1; c <= kProbeRounds; ++c) total += __syncthreads_count(dense >= c);
    if (threadIdx.x == 0) {
        __hip_atomic_store(result + 1, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(result, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
}  // namespace pgps

static float f32_dense_threshold(int d) {
    // ||F - I||_max below which the float32 smoother is not trusted.  Measured (max-norm relative error of the smoothed
    // covariance, reference grid): d = 2 / 3: 5.5e-4 / 4.0e-4 at 1e-5; d = 6: 1.1e-4 at 8e-3, 3.7e-3 at 1e-3.  From d = 17
    // (two-rows kernels, 2e-3 on an ordinary grid) every smoother call is promoted.
    if (d <= 3) return 1e-4f;
    if (d == 4) return 5e-4f;
    if (d == 5) return 2e-3f;
    if (d <= 8) return 5e-3f;
    if (d <= 16) return 1e-2f;
    return 3.0e38f;
}

// The probe of a float32 smoother call: ONE small launch on the context's stream, in front of the call's own kernels, whose
// last workgroup writes its verdict and the call's sequence number to pinned host memory.  *fixed: the policy already decides
// (no probe): 0 / 1 = float32 / fp64 arithmetic.
// (Round 4 ran the probe on a stream of its own between two events -- hipEventRecord on the context's stream, a
// hipStreamWaitEvent, a second event the host synchronised on: beside the call's first kernel instead of in front of it, but
// each event record is a barrier packet on the stream that costs the pass ~5 us (the same effect bench.py's per-launch stamps
// showed in round 5), which is where the probe's +3 .. 4.6 % on c3 came from.  One 4 us kernel costs less than its plumbing.)
static int f32_probe_launch(pgps_ctx* ctx, long N, int d, const float* Fs, int* fixed, int* nsamp_out) {
    *fixed = -1;
    if (ctx->f32_policy == 1) { *fixed = 0; return PGPS_OK; }
    if (ctx->f32_policy == 2 || d > 16) { *fixed = 1; return PGPS_OK; }
    if (N < 3) { *fixed = 0; return PGPS_OK; }
    if (!ctx->probe_host) {
        // all or nothing: the context keeps the pinned words only once every step of the setup has succeeded
        int* host = nullptr;
        int* dev = nullptr;
        HIPCHK(ctx, hipHostMalloc((void**)&host, 64, hipHostMallocDefault));
        if (hipHostGetDevicePointer((void**)&dev, host, 0) != hipSuccess) {
            (void)hipHostFree(host);
            ctx->hip_err = "float32 probe: pinned result words could not be set up";
            return PGPS_E_HIP;
        }
        host[0] = 0;
        host[1] = 0;
        ctx->probe_host = host;
        ctx->probe_dev = dev;
        ctx->probe_seq = 0;
    }
    const int nsamp = (int)std::min<long>(pgps::kProbeSamples, N - 1);
    const long stride = std::max<long>(1, (N - 1) / nsamp);
    ctx->probe_seq = (ctx->probe_seq % 0x3fffffff) + 1;         // never 0: the words start at 0
    hipLaunchKernelGGL(pgps::k_f32_probe, dim3(1), dim3(1024), 0, ctx->stream, N, d, Fs, f32_dense_threshold(d), stride, nsamp,
                       ctx->probe_dev, ctx->probe_seq);
    HIPCHK(ctx, hipGetLastError());
    *nsamp_out = nsamp;
    return PGPS_OK;
}
// ... and its answer: the host spins on the pinned sequence word (no HIP call, no event: the probe is the first thing this
// call put on the stream, whatever the call enqueues behind it keeps the GPU busy meanwhile).  Bounded: a stream that never
// reaches the probe (a hung predecessor) ends the call with PGPS_E_HIP after ~20 s instead of hanging the host.
static int f32_probe_result(pgps_ctx* ctx, int nsamp, int* dense) {
    volatile int* w = ctx->probe_host;
    const auto t0 = std::chrono::steady_clock::now();
    long spins = 0;
    while (__atomic_load_n(&w[0], __ATOMIC_ACQUIRE) != ctx->probe_seq) {
        if ((++spins & 0xfff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) {
            ctx->hip_err = "float32 probe: no verdict from the device within 20 s";
            return PGPS_E_HIP;
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    *dense = (long)w[1] * 8 >= nsamp;
    return PGPS_OK;
}

// the plain sequence: probe, wait, decide
int pgps::f32_wants_promotion(pgps_ctx* ctx, long N, int d, const float* Fs, int* wide) {
    int nsamp = 0;
    TRY(f32_probe_launch(ctx, N, d, Fs, wide, &nsamp));
    if (*wide >= 0) return PGPS_OK;                 // the policy decided
    TRY(f32_probe_result(ctx, nsamp, wide));
    ctx->f32_last_promoted = *wide;
    return PGPS_OK;
}

static int f32_run_wide(pgps_ctx* ctx, int d, const ScanArgs<float>& a, Mode mode);

// A float32 smoother call (pkfs or pks).  Waiting for the probe before anything else is enqueued leaves the GPU idle for the
// host's launch latency behind every call (3.4 % of BASELINE's c3 pass, measured); enqueuing the float32 pass first and
// asking afterwards wastes that pass when the grid turns out dense.  The context remembers which way its last probed call
// went and orders the next one accordingly -- float32 pass first after a float32 call (the wait then hides behind the
// call's own kernels: no idle time, and the float32 pass is simply overwritten by the fp64 one if the grid has become
// dense), probe first after a promoted call.  The RESULT never depends on the memory: only what is enqueued when.
static int f32_smoother_call(pgps_ctx* ctx, int d, const ScanArgs<float>& a, Mode mode) {
    int fixed = -1, nsamp = 0, dense = 0;
    int rc_ = f32_probe_launch(ctx, a.N, d, a.Fs, &fixed, &nsamp);
    if (rc_) return rc_;
    if (fixed == 0) return dispatch_scan<float>(ctx, d, a, mode);
    if (fixed == 1) return f32_run_wide(ctx, d, a, mode);
    if (ctx->f32_last_promoted) {
        if ((rc_ = f32_probe_result(ctx, nsamp, &dense))) return rc_;
        ctx->f32_last_promoted = dense;
        return dense ? f32_run_wide(ctx, d, a, mode) : dispatch_scan<float>(ctx, d, a, mode);
    }
    if ((rc_ = dispatch_scan<float>(ctx, d, a, mode))) {
        (void)f32_probe_result(ctx, nsamp, &dense);      // (the probe reads the caller's Fs: it has run before the error is returned)
        return rc_;
    }
    if ((rc_ = f32_probe_result(ctx, nsamp, &dense))) return rc_;
    ctx->f32_last_promoted = dense;
    return dense ? f32_run_wide(ctx, d, a, mode) : PGPS_OK;
}

// the float32 call `a` (whole series: pkfs or pks) in fp64 arithmetic
static int f32_run_wide(pgps_ctx* ctx, int d, const ScanArgs<float>& a, Mode mode) {
    const size_t n = (size_t)a.N, dd = (size_t)d * d;
    const size_t sizes[9] = {dd, (size_t)d, n * dd, n * dd, n, n * d, n * dd, n * d, n * dd};
    double* w[9];
    for (int i = 0; i < 9; ++i) {
        int rc_ = ensure(ctx, ctx->wide[i], sizes[i] * sizeof(double));
        if (rc_) return rc_;
        w[i] = (double*)ctx->wide[i].p;
    }
    // one conversion launch in, one out; the stand-alone smoother reads the filtered moments, the filter writes them
    WideConv conv(ctx);
    const void* in[7] = {a.P0, a.H, a.Fs, a.Qs, a.ys, a.fms, a.fPs};
    for (int i = 0; i < (mode == MODE_PKS ? 7 : 5); ++i) conv.add(in[i], w[i], sizes[i]);
    conv.widen();
    ScanArgs<double> b{};
    b.N = a.N; b.seg_first = 1; b.seg_last = 1;
    b.P0 = a.P0 ? w[0] : nullptr; b.H = a.H ? w[1] : nullptr; b.R = (double)a.R;
    b.Fs = w[2]; b.Qs = w[3]; b.ys = a.ys ? w[4] : nullptr;
    b.fms = w[5]; b.fPs = w[6]; b.sms = w[7]; b.sPs = w[8]; b.ll = a.ll;
    int rc_ = dispatch_scan<double>(ctx, d, b, mode);
    if (rc_) return rc_;
    float* const out[4] = {a.fms, a.fPs, a.sms, a.sPs};
    for (int i = (mode == MODE_PKS ? 2 : 0); i < 4; ++i) conv.add(w[5 + i], out[i], sizes[5 + i]);
    conv.narrow();
    return conv.finish();
}

// ---------------------------------------------------------------------------------------------
// device-pointer entry points
// ---------------------------------------------------------------------------------------------
template <typename T>
int pgps::pkf_dev(pgps_ctx* ctx, long N, int d, const T* P0, const T* Fs, const T* Qs, const T* H, T R,
                   const T* ys, T* fms, T* fPs, double* ll) {
    RoctxRange range_("parallel_filter");
    if (!ctx || N < 1 || !P0 || !Fs || !Qs || !H || !ys || !fms || !fPs) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    if (!aligned16(Fs) || !aligned16(Qs) || !aligned16(fms) || !aligned16(fPs)) return PGPS_E_INVALID;
    ScanArgs<T> a{};
    a.N = N; a.seg_first = 1; a.seg_last = 1;
    a.P0 = P0; a.H = H; a.R = R; a.Fs = Fs; a.Qs = Qs; a.ys = ys;
    a.fms = fms; a.fPs = fPs; a.ll = ll;
    return dispatch_scan<T>(ctx, d, a, MODE_PKF);
}

template <typename T>
static int pks_dev(pgps_ctx* ctx, long N, int d, const T* Fs, const T* Qs, const T* fms, const T* fPs,
                   T* sms, T* sPs) {
    RoctxRange range_("parallel_smoother");
    if (!ctx || N < 1 || !Fs || !Qs || !fms || !fPs || !sms || !sPs) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    if (!aligned16(Fs) || !aligned16(Qs) || !aligned16(fms) || !aligned16(fPs) || !aligned16(sms) ||
        !aligned16(sPs))
        return PGPS_E_INVALID;
    ScanArgs<T> a{};
    a.N = N; a.seg_first = 1; a.seg_last = 1;
    a.Fs = Fs; a.Qs = Qs;
    a.fms = const_cast<T*>(fms); a.fPs = const_cast<T*>(fPs); a.sms = sms; a.sPs = sPs;
    if constexpr (sizeof(T) == 4) return f32_smoother_call(ctx, d, a, MODE_PKS);
    else return dispatch_scan<T>(ctx, d, a, MODE_PKS);
}

template <typename T>
int pgps::pkfs_dev(pgps_ctx* ctx, long N, int d, const T* P0, const T* Fs, const T* Qs, const T* H, T R,
                    const T* ys, T* fms, T* fPs, T* sms, T* sPs, double* ll) {
    RoctxRange range_("parallel_filter");
    if (!ctx || N < 1 || !P0 || !Fs || !Qs || !H || !ys || !fms || !fPs || !sms || !sPs) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    if (!aligned16(Fs) || !aligned16(Qs) || !aligned16(fms) || !aligned16(fPs) || !aligned16(sms) ||
        !aligned16(sPs))
        return PGPS_E_INVALID;
    ScanArgs<T> a{};
    a.N = N; a.seg_first = 1; a.seg_last = 1;
    a.P0 = P0; a.H = H; a.R = R; a.Fs = Fs; a.Qs = Qs; a.ys = ys;
    a.fms = fms; a.fPs = fPs; a.sms = sms; a.sPs = sPs; a.ll = ll;
    if constexpr (sizeof(T) == 4) return f32_smoother_call(ctx, d, a, MODE_PKFS);
    else return dispatch_scan<T>(ctx, d, a, MODE_PKFS);
}

template <typename T>
int pgps::disc_dev(pgps_ctx* ctx, long N, int d, const T* F, const T* Pinf, const T* ts, T t0, T* Fs, T* Qs) {
    RoctxRange range_("make_model");
    if (!ctx || N < 1 || !F || !Pinf || !ts || !Fs || !Qs) return PGPS_E_INVALID;
    if constexpr (sizeof(T) == 8) {
        const bool rc_ok = d >= rc::kDimMin && d <= rc::kDimMax;
        if (rc_ok && (ctx->family == 3 || ((ctx->family == 0 || ctx->family == 4) && d > PGPS_MAX_DIM_LANE)))
            return launch_disc_rc(ctx, N, d, F, Pinf, ts, t0, Fs, Qs);
    } else {
        if ((((ctx->family == 0 || ctx->family == 4) && d > PGPS_MAX_DIM_LANE) || ctx->family == 3) && d >= rc::kDimMin &&
            d <= rc::kDimMax) {
            // fp32 at 7 <= d <= 16 (or with the row-cooperative family forced): the arithmetic is fp64 in every
            // discretisation kernel anyway; widen the inputs,
            // run the row-cooperative kernel, narrow the results
            const size_t n = (size_t)N, dd = (size_t)d * d;
            int rc_ = ensure(ctx, ctx->lti[7], (2 * dd + n + 2 * n * dd) * sizeof(double));
            if (rc_) return rc_;
            double* base = (double*)ctx->lti[7].p;
            double *F64 = base, *P64 = F64 + dd, *t64 = P64 + dd, *Fs64 = t64 + n, *Qs64 = Fs64 + n * dd;
            WideConv conv(ctx);
            conv.add(F, F64, dd);
            conv.add(Pinf, P64, dd);
            conv.add(ts, t64, n);
            conv.widen();
            rc_ = launch_disc_rc(ctx, N, d, F64, P64, t64, (double)t0, Fs64, Qs64);
            if (rc_) return rc_;
            conv.add(Fs64, Fs, n * dd);
            conv.add(Qs64, Qs, n * dd);
            conv.narrow();
            return conv.finish(false);          // (not a promotion: this arithmetic is fp64 in every family)
        }
    }
    if (ctx->family == 3) return PGPS_E_UNSUPPORTED_DIM;
    if (ctx->family == 2 || (ctx->family == 0 && d > PGPS_MAX_DIM_LANE)) return launch_disc_wc<T>(ctx, N, d, F, Pinf, ts, t0, Fs, Qs);
    return for_dim<1, 6>(d, [&](auto D) { return launch_disc<T, D()>(ctx, N, F, Pinf, ts, t0, Fs, Qs); });
}
// (the model-level calls of the other units run the array path in fp64)
template int pgps::pkf_dev<double>(pgps_ctx*, long, int, const double*, const double*, const double*, const double*, double,
                                   const double*, double*, double*, double*);
template int pgps::pkfs_dev<double>(pgps_ctx*, long, int, const double*, const double*, const double*, const double*, double,
                                    const double*, double*, double*, double*, double*, double*);
template int pgps::disc_dev<double>(pgps_ctx*, long, int, const double*, const double*, const double*, double, double*, double*);

// ---------------------------------------------------------------------------------------------
// host-pointer entry points (stage -> run -> copy back: stage_in / stage_out, pgps_host.h)
// ---------------------------------------------------------------------------------------------
template <typename T>
static int pkf_host(pgps_ctx* ctx, long N, int d, const T* P0, const T* Fs, const T* Qs, const T* H, T R,
                    const T* ys, T* fms, T* fPs, double* ll) {
    if (!ctx || N < 1 || !P0 || !Fs || !Qs || !H || !ys || !fms || !fPs) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)N, dd = (size_t)d * d;
    T *dP0, *dFs, *dQs, *dH, *dys, *dfms, *dfPs;
    double* dll;
    TRY(stage_in(ctx, ctx->st[0], P0, dd, &dP0));
    TRY(stage_in(ctx, ctx->st[1], Fs, n * dd, &dFs));
    TRY(stage_in(ctx, ctx->st[2], Qs, n * dd, &dQs));
    TRY(stage_in(ctx, ctx->st[3], H, (size_t)d, &dH));
    TRY(stage_in(ctx, ctx->st[4], ys, n, &dys));
    TRY(stage_in<T>(ctx, ctx->st[5], nullptr, n * d, &dfms));
    TRY(stage_in<T>(ctx, ctx->st[6], nullptr, n * dd, &dfPs));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 2, &dll));
    TRY(pkf_dev<T>(ctx, N, d, dP0, dFs, dQs, dH, R, dys, dfms, dfPs, ll ? dll : nullptr));
    TRY(stage_out(ctx, fms, dfms, n * d));
    TRY(stage_out(ctx, fPs, dfPs, n * dd));
    TRY(stage_out(ctx, ll, dll, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ll && !std::isfinite(*ll)) return PGPS_E_NUMERIC;
    return PGPS_OK;
}

template <typename T>
static int pks_host(pgps_ctx* ctx, long N, int d, const T* Fs, const T* Qs, const T* fms, const T* fPs, T* sms,
                    T* sPs) {
    if (!ctx || N < 1 || !Fs || !Qs || !fms || !fPs || !sms || !sPs) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)N, dd = (size_t)d * d;
    T *dFs, *dQs, *dfms, *dfPs, *dsms, *dsPs;
    TRY(stage_in(ctx, ctx->st[1], Fs, n * dd, &dFs));
    TRY(stage_in(ctx, ctx->st[2], Qs, n * dd, &dQs));
    TRY(stage_in(ctx, ctx->st[5], fms, n * d, &dfms));
    TRY(stage_in(ctx, ctx->st[6], fPs, n * dd, &dfPs));
    TRY(stage_in<T>(ctx, ctx->st[7], nullptr, n * d, &dsms));
    TRY(stage_in<T>(ctx, ctx->st[8], nullptr, n * dd, &dsPs));
    TRY(pks_dev<T>(ctx, N, d, dFs, dQs, dfms, dfPs, dsms, dsPs));
    TRY(stage_out(ctx, sms, dsms, n * d));
    TRY(stage_out(ctx, sPs, dsPs, n * dd));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGPS_OK;
}

template <typename T>
static int pkfs_host(pgps_ctx* ctx, long N, int d, const T* P0, const T* Fs, const T* Qs, const T* H, T R,
                     const T* ys, T* fms, T* fPs, T* sms, T* sPs, double* ll) {
    if (!ctx || N < 1 || !P0 || !Fs || !Qs || !H || !ys || !sms || !sPs) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)N, dd = (size_t)d * d;
    T *dP0, *dFs, *dQs, *dH, *dys, *dfms, *dfPs, *dsms, *dsPs;
    double* dll;
    TRY(stage_in(ctx, ctx->st[0], P0, dd, &dP0));
    TRY(stage_in(ctx, ctx->st[1], Fs, n * dd, &dFs));
    TRY(stage_in(ctx, ctx->st[2], Qs, n * dd, &dQs));
    TRY(stage_in(ctx, ctx->st[3], H, (size_t)d, &dH));
    TRY(stage_in(ctx, ctx->st[4], ys, n, &dys));
    TRY(stage_in<T>(ctx, ctx->st[5], nullptr, n * d, &dfms));
    TRY(stage_in<T>(ctx, ctx->st[6], nullptr, n * dd, &dfPs));
    TRY(stage_in<T>(ctx, ctx->st[7], nullptr, n * d, &dsms));
    TRY(stage_in<T>(ctx, ctx->st[8], nullptr, n * dd, &dsPs));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 2, &dll));
    TRY(pkfs_dev<T>(ctx, N, d, dP0, dFs, dQs, dH, R, dys, dfms, dfPs, dsms, dsPs, dll));
    TRY(stage_out(ctx, fms, dfms, n * d));
    TRY(stage_out(ctx, fPs, dfPs, n * dd));
    TRY(stage_out(ctx, sms, dsms, n * d));
    TRY(stage_out(ctx, sPs, dsPs, n * dd));
    double llh = 0.0;
    TRY(stage_out(ctx, &llh, dll, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ll) *ll = llh;
    if (!std::isfinite(llh)) return PGPS_E_NUMERIC;
    return PGPS_OK;
}

template <typename T>
static int disc_host(pgps_ctx* ctx, long N, int d, const T* F, const T* Pinf, const T* ts, T t0, T* Fs, T* Qs) {
    if (!ctx || N < 1 || !F || !Pinf || !ts || !Fs || !Qs) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)N, dd = (size_t)d * d;
    T *dF, *dP, *dts, *dFs, *dQs;
    TRY(stage_in(ctx, ctx->st[0], F, dd, &dF));
    TRY(stage_in(ctx, ctx->st[3], Pinf, dd, &dP));
    TRY(stage_in(ctx, ctx->st[4], ts, n, &dts));
    TRY(stage_in<T>(ctx, ctx->st[1], nullptr, n * dd, &dFs));
    TRY(stage_in<T>(ctx, ctx->st[2], nullptr, n * dd, &dQs));
    TRY(disc_dev<T>(ctx, N, d, dF, dP, dts, t0, dFs, dQs));
    TRY(stage_out(ctx, Fs, dFs, n * dd));
    TRY(stage_out(ctx, Qs, dQs, n * dd));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGPS_OK;
}

// ---------------------------------------------------------------------------------------------
// extern "C" surface
// ---------------------------------------------------------------------------------------------
#define PGPS_DEFINE(SUF, T)                                                                                          \
    extern "C" int pgps_discretise_##SUF(pgps_ctx* c, long N, int d, const T* F, const T* P, const T* ts, T t0,     \
                                         T* Fs, T* Qs) {                                                            \
        return disc_host<T>(c, N, d, F, P, ts, t0, Fs, Qs);                                                         \
    }                                                                                                                \
    extern "C" int pgps_discretise_dev_##SUF(pgps_ctx* c, long N, int d, const T* F, const T* P, const T* ts, T t0, \
                                             T* Fs, T* Qs) {                                                        \
        if (d < 1 || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;                                               \
        return disc_dev<T>(c, N, d, F, P, ts, t0, Fs, Qs);                                                          \
    }                                                                                                                \
    extern "C" int pgps_pkf_##SUF(pgps_ctx* c, long N, int d, const T* P0, const T* Fs, const T* Qs, const T* H,    \
                                  T R, const T* ys, T* fms, T* fPs, double* ll) {                                   \
        return pkf_host<T>(c, N, d, P0, Fs, Qs, H, R, ys, fms, fPs, ll);                                            \
    }                                                                                                                \
    extern "C" int pgps_pkf_dev_##SUF(pgps_ctx* c, long N, int d, const T* P0, const T* Fs, const T* Qs,            \
                                      const T* H, T R, const T* ys, T* fms, T* fPs, double* ll) {                   \
        return pkf_dev<T>(c, N, d, P0, Fs, Qs, H, R, ys, fms, fPs, ll);                                             \
    }                                                                                                                \
    extern "C" int pgps_pks_##SUF(pgps_ctx* c, long N, int d, const T* Fs, const T* Qs, const T* fms,               \
                                  const T* fPs, T* sms, T* sPs) {                                                   \
        return pks_host<T>(c, N, d, Fs, Qs, fms, fPs, sms, sPs);                                                    \
    }                                                                                                                \
    extern "C" int pgps_pks_dev_##SUF(pgps_ctx* c, long N, int d, const T* Fs, const T* Qs, const T* fms,           \
                                      const T* fPs, T* sms, T* sPs) {                                               \
        return pks_dev<T>(c, N, d, Fs, Qs, fms, fPs, sms, sPs);                                                     \
    }                                                                                                                \
    extern "C" int pgps_pkfs_##SUF(pgps_ctx* c, long N, int d, const T* P0, const T* Fs, const T* Qs, const T* H,   \
                                   T R, const T* ys, T* fms, T* fPs, T* sms, T* sPs, double* ll) {                  \
        return pkfs_host<T>(c, N, d, P0, Fs, Qs, H, R, ys, fms, fPs, sms, sPs, ll);                                 \
    }                                                                                                                \
    extern "C" int pgps_pkfs_dev_##SUF(pgps_ctx* c, long N, int d, const T* P0, const T* Fs, const T* Qs,           \
                                       const T* H, T R, const T* ys, T* fms, T* fPs, T* sms, T* sPs, double* ll) {  \
        return pkfs_dev<T>(c, N, d, P0, Fs, Qs, H, R, ys, fms, fPs, sms, sPs, ll);                                  \
    }

PGPS_DEFINE(f64, double)
PGPS_DEFINE(f32, float)

// ---------------------------------------------------------------------------------------------
// segment (multi-GPU) entry points
// ---------------------------------------------------------------------------------------------
extern "C" int pgps_seg_record_len(int d, int* rec_filter, int* rec_smoother) {
    if (d < 1 || !rec_filter || !rec_smoother) return PGPS_E_INVALID;
    *rec_filter = seg_rec_f_len(d);
    *rec_smoother = seg_rec_s_len(d);
    return PGPS_OK;
}

template <typename T>
static int seg_common(pgps_ctx* ctx, long N, int d, int rank, int nranks, ScanArgs<T>& a) {
    if (!ctx || N < 1 || rank < 0 || nranks < 1 || rank >= nranks) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    a.N = N;
    a.rank = rank;
    a.nranks = nranks;
    return PGPS_OK;
}

// Phase `phase` (2, 3) may only follow phase - 1 of the same pass with nothing else on the context in between: the
// scratch it reads (chain totals, their scans, stored smoothing elements) is whatever the last call left in `ws`.
static bool seg_follows(const pgps_ctx* ctx, int phase, long N, int d, int rank, int nranks) {
    const auto& t = ctx->seg_tag;
    return t.phase == phase - 1 && t.N == N && t.d == d && t.rank == rank && t.nranks == nranks && t.chunk == ctx->chunk && t.block == ctx->block &&
           t.family == ctx->family && t.stage_g == ctx->stage_g && t.dma == ctx->dma && t.rc_scan == ctx->rc_scan && t.epoch == ctx->ws_epoch;
}
static void seg_mark(pgps_ctx* ctx, int phase, long N, int d, int rank, int nranks) {
    ctx->seg_tag.phase = phase; ctx->seg_tag.N = N; ctx->seg_tag.d = d; ctx->seg_tag.rank = rank;
    ctx->seg_tag.nranks = nranks; ctx->seg_tag.chunk = ctx->chunk; ctx->seg_tag.block = ctx->block; ctx->seg_tag.family = ctx->family;
    ctx->seg_tag.stage_g = ctx->stage_g; ctx->seg_tag.dma = ctx->dma; ctx->seg_tag.rc_scan = ctx->rc_scan; ctx->seg_tag.epoch = ctx->ws_epoch;
}

template <typename T>
static int seg_reduce(pgps_ctx* ctx, long N, int d, int rank, int nranks, const T* P0, const T* Fs, const T* Qs,
                      const T* H, T R, const T* ys, T* rec_f) {
    ScanArgs<T> a{};
    TRY(seg_common<T>(ctx, N, d, rank, nranks, a));
    if (!P0 || !Fs || !Qs || !H || !ys || !rec_f || !aligned16(Fs) || !aligned16(Qs)) return PGPS_E_INVALID;
    a.P0 = P0; a.H = H; a.R = R; a.Fs = Fs; a.Qs = Qs; a.ys = ys; a.rec_f = rec_f;
    ctx->seg_tag.phase = 0;
    TRY(dispatch_scan<T>(ctx, d, a, MODE_SEG_REDUCE));
    seg_mark(ctx, 1, N, d, rank, nranks);
    return PGPS_OK;
}

template <typename T>
static int seg_filter(pgps_ctx* ctx, long N, int d, int rank, int nranks, const T* P0, const T* Fs, const T* Qs,
                      const T* H, T R, const T* ys, const T* gathered_f, T* fms, T* fPs, T* rec_s) {
    ScanArgs<T> a{};
    TRY(seg_common<T>(ctx, N, d, rank, nranks, a));
    if (!P0 || !Fs || !Qs || !H || !ys || !gathered_f || !fms || !fPs || !rec_s) return PGPS_E_INVALID;
    if (!aligned16(Fs) || !aligned16(Qs) || !aligned16(fms) || !aligned16(fPs) || !aligned16(rec_s))
        return PGPS_E_INVALID;
    a.P0 = P0; a.H = H; a.R = R; a.Fs = Fs; a.Qs = Qs; a.ys = ys;
    a.gathered_f = gathered_f; a.fms = fms; a.fPs = fPs; a.rec_s = rec_s;
    if (!seg_follows(ctx, 2, N, d, rank, nranks)) return PGPS_E_INVALID;
    ctx->seg_tag.phase = 0;
    TRY(dispatch_scan<T>(ctx, d, a, MODE_SEG_FILTER));
    seg_mark(ctx, 2, N, d, rank, nranks);
    return PGPS_OK;
}

template <typename T>
static int seg_smoother(pgps_ctx* ctx, long N, int d, int rank, int nranks, const T* Fs, const T* Qs, const T* fms,
                        const T* fPs, const T* gathered_s, T* sms, T* sPs, double* ll) {
    ScanArgs<T> a{};
    TRY(seg_common<T>(ctx, N, d, rank, nranks, a));
    if (!Fs || !Qs || !fms || !fPs || !gathered_s || !sms || !sPs) return PGPS_E_INVALID;
    if (!aligned16(Fs) || !aligned16(Qs) || !aligned16(fms) || !aligned16(fPs) || !aligned16(sms) ||
        !aligned16(sPs) || !aligned16(gathered_s))
        return PGPS_E_INVALID;
    a.Fs = Fs; a.Qs = Qs; a.fms = const_cast<T*>(fms); a.fPs = const_cast<T*>(fPs);
    a.gathered_s = gathered_s; a.sms = sms; a.sPs = sPs; a.ll = ll;
    if (!seg_follows(ctx, 3, N, d, rank, nranks)) return PGPS_E_INVALID;
    ctx->seg_tag.phase = 0;
    return dispatch_scan<T>(ctx, d, a, MODE_SEG_SMOOTHER);
}

#define PGPS_DEFINE_SEG(SUF, T)                                                                                      \
    extern "C" int pgps_seg_filter_reduce_dev_##SUF(pgps_ctx* c, long N, int d, int rank, int nranks, const T* P0,   \
                                                    const T* Fs, const T* Qs, const T* H, T R, const T* ys,         \
                                                    T* rec_f) {                                                     \
        return seg_reduce<T>(c, N, d, rank, nranks, P0, Fs, Qs, H, R, ys, rec_f);                                   \
    }                                                                                                                \
    extern "C" int pgps_seg_filter_apply_dev_##SUF(pgps_ctx* c, long N, int d, int rank, int nranks, const T* P0,    \
                                                   const T* Fs, const T* Qs, const T* H, T R, const T* ys,          \
                                                   const T* gathered_f, T* fms, T* fPs, T* rec_s) {                 \
        return seg_filter<T>(c, N, d, rank, nranks, P0, Fs, Qs, H, R, ys, gathered_f, fms, fPs, rec_s);             \
    }                                                                                                                \
    extern "C" int pgps_seg_smoother_apply_dev_##SUF(pgps_ctx* c, long N, int d, int rank, int nranks, const T* Fs,  \
                                                     const T* Qs, const T* fms, const T* fPs, const T* gathered_s,  \
                                                     T* sms, T* sPs, double* ll) {                                  \
        return seg_smoother<T>(c, N, d, rank, nranks, Fs, Qs, fms, fPs, gathered_s, sms, sPs, ll);                  \
    }

PGPS_DEFINE_SEG(f64, double)
PGPS_DEFINE_SEG(f32, float)

// One call per pass: reduce -> all-gather -> filter -> all-gather -> smoother, all enqueued on the context's stream
// through the context's own RCCL communicator -- no host round trip, no framework in between.
template <typename T>
static int pkfs_seg_run(pgps_ctx* ctx, long N, int d, const T* P0, const T* Fs, const T* Qs, const T* H, T R, const T* ys,
                        T* fms, T* fPs, T* sms, T* sPs, double* ll) {
    RoctxRange range_("parallel_filter");
    const int rank = ctx->comm_rank, nranks = ctx->comm_nranks;
    const size_t rf = ((size_t)seg_rec_f_len(d) * sizeof(T) + 15) / 16 * 16, rs = ((size_t)seg_rec_s_len(d) * sizeof(T) + 15) / 16 * 16;
    TRY(ensure(ctx, ctx->comm_buf, (rf + rs) * (size_t)(nranks + 1)));
    char* base = (char*)ctx->comm_buf.p;
    T* rec_f = (T*)base;
    T* rec_s = (T*)(base + rf);
    T* gat_f = (T*)(base + rf + rs);
    T* gat_s = (T*)(base + rf + rs + rf * (size_t)nranks);
    // records travel at their natural length (the ranks' slots in gathered_* are seg_rec_*_len(d) apart)
    TRY(seg_reduce<T>(ctx, N, d, rank, nranks, P0, Fs, Qs, H, R, ys, rec_f));
    TRY(comm_allgather(ctx, rec_f, gat_f, (size_t)seg_rec_f_len(d) * sizeof(T)));
    TRY(seg_filter<T>(ctx, N, d, rank, nranks, P0, Fs, Qs, H, R, ys, gat_f, fms, fPs, rec_s));
    TRY(comm_allgather(ctx, rec_s, gat_s, (size_t)seg_rec_s_len(d) * sizeof(T)));
    return seg_smoother<T>(ctx, N, d, rank, nranks, Fs, Qs, fms, fPs, gat_s, sms, sPs, ll);
}

template <typename T>
static int pkfs_seg_dev(pgps_ctx* ctx, long N, int d, const T* P0, const T* Fs, const T* Qs, const T* H, T R, const T* ys,
                        T* fms, T* fPs, T* sms, T* sPs, double* ll) {
    if (!ctx || N < 1 || !P0 || !Fs || !Qs || !H || !ys || !fms || !fPs || !sms || !sPs) return PGPS_E_INVALID;
    if (!ctx->comm) return PGPS_E_INVALID;                      // pgps_comm_init first (also for one rank)
    if (d < 1 || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    return pkfs_seg_run<T>(ctx, N, d, P0, Fs, Qs, H, R, ys, fms, fPs, sms, sPs, ll);
}

extern "C" int pgps_pkfs_seg_dev_f64(pgps_ctx* c, long N, int d, const double* P0, const double* Fs, const double* Qs,
                                     const double* H, double R, const double* ys, double* fms, double* fPs, double* sms,
                                     double* sPs, double* ll) {
    return pkfs_seg_dev<double>(c, N, d, P0, Fs, Qs, H, R, ys, fms, fPs, sms, sPs, ll);
}
extern "C" int pgps_pkfs_seg_dev_f32(pgps_ctx* c, long N, int d, const float* P0, const float* Fs, const float* Qs,
                                     const float* H, float R, const float* ys, float* fms, float* fPs, float* sms, float* sPs,
                                     double* ll) {
    return pkfs_seg_dev<float>(c, N, d, P0, Fs, Qs, H, R, ys, fms, fPs, sms, sPs, ll);
}
