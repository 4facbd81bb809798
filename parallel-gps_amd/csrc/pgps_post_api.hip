// pgps_post_api.hip -- what the C ABI (include/pgps.h) offers of the posterior beyond its marginals: joint draws by
// backward sampling, the joint covariance between selected steps, both on arrays and at model level, and the moments of a
// mixture of batched predictions.  The scan kernels are the sampler's and the covariance's (dtype, d) units.
#include "pgps_host.h"

using namespace pgps;

// ---------------------------------------------------------------------------------------------
// joint posterior draws: backward sampling (pgps_sample.hip.h)
// ---------------------------------------------------------------------------------------------
template <typename T>
static int sample_dispatch(pgps_ctx* ctx, int d, const SampleArgs<T>& a) {
    return for_dim<1, 6>(d, [&](auto D) { return launch_sample<T, D()>(ctx, a); });
}

// the float32 call `a` in fp64 arithmetic: widened inputs (and z), the fp64 draws where the library draws, rounded output
static int sample_run_wide(pgps_ctx* ctx, int d, const SampleArgs<float>& a) {
    const size_t n = (size_t)a.N, dd = (size_t)d * d, S = (size_t)a.S;
    const size_t nz = a.z ? S * n * d : 0, nout = S * (size_t)a.out_rows * (a.proj ? 1 : d);
    TRY(ensure(ctx, ctx->wide[2], n * dd * sizeof(double)));
    TRY(ensure(ctx, ctx->wide[3], n * dd * sizeof(double)));
    TRY(ensure(ctx, ctx->wide[5], n * d * sizeof(double)));
    TRY(ensure(ctx, ctx->wide[6], n * dd * sizeof(double)));
    TRY(ensure(ctx, ctx->smp_wide, (nz + nout + 32) * sizeof(double)));
    double* zw = (double*)ctx->smp_wide.p;
    double* ow = zw + (nz + 31) / 32 * 32;
    WideConv conv(ctx);
    conv.add(a.Fs, ctx->wide[2].p, n * dd);
    conv.add(a.Qs, ctx->wide[3].p, n * dd);
    conv.add(a.fms, ctx->wide[5].p, n * d);
    conv.add(a.fPs, ctx->wide[6].p, n * dd);
    conv.add(a.z, zw, nz);
    conv.widen();
    SampleArgs<double> b{};
    b.N = a.N; b.S = a.S; b.s0 = a.s0; b.seed = a.seed;
    b.Fs = (const double*)ctx->wide[2].p; b.Qs = (const double*)ctx->wide[3].p;
    b.fms = (const double*)ctx->wide[5].p; b.fPs = (const double*)ctx->wide[6].p;
    b.z = a.z ? zw : nullptr;
    b.proj = a.proj;
    for (int i = 0; i < PGPS_MAX_DIM_LANE; ++i) b.h[i] = (double)a.h[i];
    b.out = ow; b.out_rows = a.out_rows; b.qslot = a.qslot;
    TRY(sample_dispatch<double>(ctx, d, b));
    conv.narrow_one(ow, a.out, nout);
    return conv.finish();
}

// float32: the policy of pgps_pks_f32 -- the dense-grid probe decides between the float32 kernels and the fp64 ones
static int sample_f32_call(pgps_ctx* ctx, int d, const SampleArgs<float>& a) {
    int wide = 0;
    TRY(f32_wants_promotion(ctx, a.N, d, a.Fs, &wide));
    return wide ? sample_run_wide(ctx, d, a) : sample_dispatch<float>(ctx, d, a);
}

template <typename T>
static int pks_sample_dev(pgps_ctx* ctx, long N, int d, const T* Fs, const T* Qs, const T* fms, const T* fPs, int S, long s0,
                          unsigned long long seed, const T* z, const T* H, T* out) {
    RoctxRange range_("parallel_sampler");
    if (!ctx || N < 1 || S < 1 || s0 < 0 || s0 + S > 0xffffffffL || !Fs || !Qs || !fms || !fPs || !out) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM_LANE) return PGPS_E_UNSUPPORTED_DIM;
    if (!aligned16(Fs) || !aligned16(Qs) || !aligned16(fms) || !aligned16(fPs)) return PGPS_E_INVALID;
    SampleArgs<T> a{};
    a.N = N; a.Fs = Fs; a.Qs = Qs; a.fms = fms; a.fPs = fPs;
    a.S = S; a.s0 = s0; a.seed = seed; a.z = z;
    a.proj = H ? 1 : 0;
    for (int i = 0; i < d && H; ++i) a.h[i] = H[i];
    a.out = out; a.out_rows = N; a.qslot = nullptr;
    if constexpr (sizeof(T) == 4) return sample_f32_call(ctx, d, a);
    else return sample_dispatch<T>(ctx, d, a);
}

template <typename T>
static int pks_sample_host(pgps_ctx* ctx, long N, int d, const T* Fs, const T* Qs, const T* fms, const T* fPs, int S, long s0,
                           unsigned long long seed, const T* z, const T* H, T* out) {
    if (!ctx || N < 1 || S < 1 || !Fs || !Qs || !fms || !fPs || !out) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM_LANE) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)N, dd = (size_t)d * d, nout = (size_t)S * n * (H ? 1 : d);
    T *dFs, *dQs, *dfms, *dfPs, *dz = nullptr, *dout;
    TRY(stage_in(ctx, ctx->st[1], Fs, n * dd, &dFs));
    TRY(stage_in(ctx, ctx->st[2], Qs, n * dd, &dQs));
    TRY(stage_in(ctx, ctx->st[5], fms, n * d, &dfms));
    TRY(stage_in(ctx, ctx->st[6], fPs, n * dd, &dfPs));
    if (z) TRY(stage_in(ctx, ctx->st[7], z, (size_t)S * n * d, &dz));
    TRY(stage_in<T>(ctx, ctx->st[8], nullptr, nout, &dout));
    TRY(pks_sample_dev<T>(ctx, N, d, dFs, dQs, dfms, dfPs, S, s0, seed, dz, H, dout));
    TRY(stage_out(ctx, out, dout, nout));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGPS_OK;
}

template <typename T>
static int sample_normals_dev(pgps_ctx* ctx, long N, int d, int S, long s0, unsigned long long seed, T* z) {
    if (!ctx || N < 1 || d < 1 || S < 1 || s0 < 0 || s0 + S > 0xffffffffL || !z) return PGPS_E_INVALID;
    return launch_sample_normals<T>(ctx, N, d, S, s0, seed, z);
}

#define PGPS_DEFINE_SAMPLE(SUF, T)                                                                                         \
    extern "C" int pgps_pks_sample_##SUF(pgps_ctx* c, long N, int d, const T* Fs, const T* Qs, const T* fms, const T* fPs, \
                                         int S, long s0, unsigned long long seed, const T* z, const T* H, T* out) {        \
        return pks_sample_host<T>(c, N, d, Fs, Qs, fms, fPs, S, s0, seed, z, H, out);                                     \
    }                                                                                                                      \
    extern "C" int pgps_pks_sample_dev_##SUF(pgps_ctx* c, long N, int d, const T* Fs, const T* Qs, const T* fms,          \
                                             const T* fPs, int S, long s0, unsigned long long seed, const T* z,            \
                                             const T* H, T* out) {                                                         \
        return pks_sample_dev<T>(c, N, d, Fs, Qs, fms, fPs, S, s0, seed, z, H, out);                                      \
    }                                                                                                                      \
    extern "C" int pgps_sample_normals_dev_##SUF(pgps_ctx* c, long N, int d, int S, long s0, unsigned long long seed,     \
                                                 T* z) {                                                                   \
        return sample_normals_dev<T>(c, N, d, S, s0, seed, z);                                                            \
    }

PGPS_DEFINE_SAMPLE(f64, double)
PGPS_DEFINE_SAMPLE(f32, float)

// the model-level sampler: merge (k_merge_sorted: its qslot is the output column), discretisation, filter over the N + K
// steps with the query rows missing, backward sampling projected through H at the query rows only
static int lti_sample_dev(pgps_ctx* ctx, long N, long K, int d, const double* F, const double* Pinf, const double* H, double R,
                          const double* ts, const double* ys, double t0, const double* tq, int S, long s0,
                          unsigned long long seed, double* out, double* ll) {
    if (!ctx || N < 1 || K < 1 || S < 1 || s0 < 0 || s0 + S > 0xffffffffL || !F || !Pinf || !H || !ts || !ys || !tq || !out)
        return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM_LANE) return PGPS_E_UNSUPPORTED_DIM;
    if (N + K > 0x7fffffffL) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t m = (size_t)(N + K);
    Merged<double> mg;
    LtiFront f;
    TRY(merged_front<double>(ctx, ctx->lti + 1, N, K, ts, ys, tq, &mg));
    TRY(lti_filter_front(ctx, m, d, F, Pinf, H, R, mg.ts, mg.ys, t0, false, ll, &f));
    SampleArgs<double> a{};
    a.N = (long)m; a.Fs = f.Fs; a.Qs = f.Qs; a.fms = f.fms; a.fPs = f.fPs;
    a.S = S; a.s0 = s0; a.seed = seed; a.z = nullptr;
    a.proj = 1;
    for (int i = 0; i < d; ++i) a.h[i] = H[i];
    a.out = out; a.out_rows = K; a.qslot = mg.qslot;
    return sample_dispatch<double>(ctx, d, a);
}

static int lti_sample_host(pgps_ctx* ctx, long N, long K, int d, const double* F, const double* Pinf, const double* H, double R,
                           const double* ts, const double* ys, double t0, const double* tq, int S, long s0,
                           unsigned long long seed, double* out, double* ll) {
    if (!ctx || N < 1 || K < 1 || S < 1 || !ts || !ys || !tq || !out) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nout = (size_t)S * (size_t)K;
    {
        SmallStage st(ctx, 2 * SmallStage::up((size_t)N * 8) + SmallStage::up((size_t)K * 8), SmallStage::up(nout * 8) + 16);
        if (st.ok) {
            double llh = 0.0;
            double* dts_ = st.in(ts, (size_t)N);
            double* dys_ = st.in(ys, (size_t)N);
            double* dtq_ = st.in(tq, (size_t)K);
            double* dll_ = st.out(&llh, 1);
            double* dout_ = st.out(out, nout);
            TRY(st.send());
            TRY(lti_sample_dev(ctx, N, K, d, F, Pinf, H, R, dts_, dys_, t0, dtq_, S, s0, seed, dout_, dll_));
            TRY(st.finish());
            if (ll) *ll = llh;
            return std::isfinite(llh) ? PGPS_OK : PGPS_E_NUMERIC;
        }
    }
    double *dts, *dys, *dtq, *dout, *dll;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    TRY(stage_in(ctx, ctx->st[3], tq, (size_t)K, &dtq));
    TRY(stage_in<double>(ctx, ctx->st[8], nullptr, nout, &dout));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 2, &dll));
    TRY(lti_sample_dev(ctx, N, K, d, F, Pinf, H, R, dts, dys, t0, dtq, S, s0, seed, dout, dll));
    TRY(stage_out(ctx, out, dout, nout));
    double llh = 0.0;
    TRY(stage_out(ctx, &llh, dll, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ll) *ll = llh;
    return std::isfinite(llh) ? PGPS_OK : PGPS_E_NUMERIC;
}

extern "C" int pgps_lti_sample_f64(pgps_ctx* c, long N, long K, int d, const double* F, const double* Pinf, const double* H,
                                   double R, const double* ts, const double* ys, double t0, const double* tq, int S, long s0,
                                   unsigned long long seed, double* out, double* ll) {
    if (!F || !Pinf || !H) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM_LANE) return PGPS_E_UNSUPPORTED_DIM;
    return lti_sample_host(c, N, K, d, F, Pinf, H, R, ts, ys, t0, tq, S, s0, seed, out, ll);
}
extern "C" int pgps_lti_sample_dev_f64(pgps_ctx* c, long N, long K, int d, const double* F, const double* Pinf,
                                       const double* H, double R, const double* ts, const double* ys, double t0,
                                       const double* tq, int S, long s0, unsigned long long seed, double* out, double* ll) {
    return lti_sample_dev(c, N, K, d, F, Pinf, H, R, ts, ys, t0, tq, S, s0, seed, out, ll);
}

// ---------------------------------------------------------------------------------------------
// joint posterior covariance between selected steps (pgps_cov.hip.h)
// ---------------------------------------------------------------------------------------------
namespace pgps {
// bad <- 1 unless 0 <= sel[0] < sel[1] < .. < sel[n-1] < N
static __global__ void k_cov_check(long N, long n, const long* sel, int* bad) {
    for (long a = (long)blockIdx.x * blockDim.x + threadIdx.x; a < n; a += (long)gridDim.x * blockDim.x) {
        const long k = sel[a];
        if (k < 0 || k >= N || (a > 0 && sel[a - 1] >= k)) *bad = 1;
    }
}
// slot[sel[a]] = a (slot filled with -1 before; sel checked before)
static __global__ void k_cov_slots(long n, const long* sel, int* slot) {
    for (long a = (long)blockIdx.x * blockDim.x + threadIdx.x; a < n; a += (long)gridDim.x * blockDim.x) slot[sel[a]] = (int)a;
}
// the selected steps' smoothed covariances, compact: sPsel[slot[k]] = sPs[k]; with sms: mean[slot[k]] = h . sms[k]
template <typename T>
static __global__ void k_cov_gather(long N, int d, long n, const int* slot, const T* sPs, T* sPsel, const T* sms, const T* h,
                                    T* mean) {
    const int dd = d * d;
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < N; k += (long)gridDim.x * blockDim.x) {
        const int a = slot[k];
        if (a < 0 || a >= n) continue;
        for (int i = 0; i < dd; ++i) sPsel[(long)a * dd + i] = sPs[k * dd + i];
        if (sms) {
            T acc = T(0);
            for (int i = 0; i < d; ++i) acc += h[i] * sms[k * d + i];
            mean[a] = acc;
        }
    }
}
}  // namespace pgps

static dim3 cov_grid(long n) { return dim3((unsigned)std::max<long>(1, std::min<long>(4096, (n + 255) / 256))); }

// bytes of the (n, n) or (n, n, d, d) output, 0 when no allocation could hold it
static size_t cov_out_count(long n, int d, bool proj) {
    const double cnt = (double)n * (double)n * (proj ? 1.0 : (double)d * d);
    return cnt > 0x1p44 ? 0 : (size_t)n * (size_t)n * (proj ? 1 : (size_t)d * d);
}

// (n,) selection [device] -> ctx->cov[1] = (N,) slots; PGPS_E_INVALID unless strictly increasing inside [0, N)
static int cov_slots(pgps_ctx* ctx, long N, long n, const long* sel, int** slot) {
    int* bad;
    TRY(stage_in<int>(ctx, ctx->cov[5], nullptr, 4, &bad));
    TRY(stage_in<int>(ctx, ctx->cov[1], nullptr, (size_t)N, slot));
    HIPCHK(ctx, hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(pgps::k_cov_check, cov_grid(n), dim3(256), 0, ctx->stream, N, n, sel, bad);
    int bad_h = 0;
    HIPCHK(ctx, hipMemcpyAsync(&bad_h, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bad_h) return PGPS_E_INVALID;
    HIPCHK(ctx, hipMemsetAsync(*slot, 0xff, (size_t)N * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(pgps::k_cov_slots, cov_grid(n), dim3(256), 0, ctx->stream, n, sel, *slot);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

template <typename T>
static int cov_gains_run(pgps_ctx* ctx, long N, int d, const T* Fs, const T* Qs, const T* fPs, long n, const int* slot, T* B) {
    CovArgs<T> g{};
    g.N = N; g.Fs = Fs; g.Qs = Qs; g.fPs = fPs; g.slot = slot; g.n = n; g.B = B;
    return for_dim<1, 6>(d, [&](auto D) { return launch_cov_gains<T, D()>(ctx, g); });
}
template <typename T>
static int cov_fill_run(pgps_ctx* ctx, long n, int d, const T* B, const T* sPsel, const T* H, T* out) {
    CovFillArgs<T> f{};
    f.n = n; f.B = B; f.sP = sPsel; f.proj = H ? 1 : 0; f.out = out;
    for (int i = 0; i < d && H; ++i) f.h[i] = H[i];
    return for_dim<1, 6>(d, [&](auto D) { return launch_cov_fill<T, D()>(ctx, f); });
}

// everything on the device but H: the selected sPs (and, with sms, the projected means) are gathered, then the two passes
template <typename T>
static int cov_core(pgps_ctx* ctx, long N, int d, const T* Fs, const T* Qs, const T* fPs, const T* sPs, long n, const int* slot,
                    const T* H, T* out, const T* sms = nullptr, const T* h_dev = nullptr, T* mean = nullptr) {
    const size_t dd = (size_t)d * d;
    T *B, *sPsel;
    TRY(stage_in<T>(ctx, ctx->cov[2], nullptr, (size_t)std::max<long>(1, n - 1) * dd, &B));
    TRY(stage_in<T>(ctx, ctx->cov[3], nullptr, (size_t)n * dd, &sPsel));
    hipLaunchKernelGGL(pgps::k_cov_gather<T>, cov_grid(N), dim3(256), 0, ctx->stream, N, d, n, slot, sPs, sPsel, sms, h_dev, mean);
    HIPCHK(ctx, hipGetLastError());
    if (n > 1) TRY(cov_gains_run<T>(ctx, N, d, Fs, Qs, fPs, n, slot, B));
    return cov_fill_run<T>(ctx, n, d, B, sPsel, H, out);
}

// the float32 call in fp64 arithmetic: widened inputs, rounded output
static int cov_run_wide(pgps_ctx* ctx, long N, int d, const float* Fs, const float* Qs, const float* fPs, const float* sPs,
                        long n, const int* slot, const float* H, float* out, size_t nout) {
    const size_t cnt = (size_t)N * d * d;
    const int idx[4] = {2, 3, 6, 8};
    const float* src[4] = {Fs, Qs, fPs, sPs};
    WideConv conv(ctx);
    for (int i = 0; i < 4; ++i) {
        TRY(ensure(ctx, ctx->wide[idx[i]], cnt * sizeof(double)));
        conv.add(src[i], ctx->wide[idx[i]].p, cnt);
    }
    TRY(ensure(ctx, ctx->cov_wide, nout * sizeof(double)));
    conv.widen();
    double Hw[PGPS_MAX_DIM_LANE];
    for (int i = 0; i < d && H; ++i) Hw[i] = (double)H[i];
    double* ow = (double*)ctx->cov_wide.p;
    TRY(cov_core<double>(ctx, N, d, (const double*)ctx->wide[2].p, (const double*)ctx->wide[3].p, (const double*)ctx->wide[6].p,
                         (const double*)ctx->wide[8].p, n, slot, H ? Hw : nullptr, ow));
    conv.narrow_one(ow, out, nout);
    return conv.finish();
}

template <typename T>
static int pks_cov_dev(pgps_ctx* ctx, long N, int d, const T* Fs, const T* Qs, const T* fPs, const T* sPs, long n,
                       const long* sel, const T* H, T* out) {
    RoctxRange range_("parallel_covariance");
    if (!ctx || N < 1 || N > 0x7fffffffL || n < 1 || n > N || !Fs || !Qs || !fPs || !sPs || !sel || !out) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM_LANE) return PGPS_E_UNSUPPORTED_DIM;
    if (!aligned16(Fs) || !aligned16(Qs) || !aligned16(fPs) || !aligned16(sPs) || !aligned16(out) || (((uintptr_t)sel) & 7u))
        return PGPS_E_INVALID;
    const size_t nout = cov_out_count(n, d, H != nullptr);
    if (!nout) return PGPS_E_NOMEM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int* slot;
    TRY(cov_slots(ctx, N, n, sel, &slot));
    if constexpr (sizeof(T) == 4) {
        // the policy of pgps_pks_f32: the dense-grid probe decides between the float32 kernels and the fp64 ones
        int wide = 0;
        TRY(f32_wants_promotion(ctx, N, d, Fs, &wide));
        if (wide) return cov_run_wide(ctx, N, d, Fs, Qs, fPs, sPs, n, slot, H, out, nout);
    }
    return cov_core<T>(ctx, N, d, Fs, Qs, fPs, sPs, n, slot, H, out);
}

template <typename T>
static int pks_cov_host(pgps_ctx* ctx, long N, int d, const T* Fs, const T* Qs, const T* fPs, const T* sPs, long n,
                        const long* sel, const T* H, T* out) {
    if (!ctx || N < 1 || n < 1 || n > N || !Fs || !Qs || !fPs || !sPs || !sel || !out) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM_LANE) return PGPS_E_UNSUPPORTED_DIM;
    const size_t nout = cov_out_count(n, d, H != nullptr);
    if (!nout) return PGPS_E_NOMEM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t cnt = (size_t)N * d * d;
    T *dFs, *dQs, *dfPs, *dsPs, *dout;
    long* dsel;
    TRY(stage_in<T>(ctx, ctx->st[8], nullptr, nout, &dout));        // the large one first: nothing is copied if it cannot be had
    TRY(stage_in(ctx, ctx->st[1], Fs, cnt, &dFs));
    TRY(stage_in(ctx, ctx->st[2], Qs, cnt, &dQs));
    TRY(stage_in(ctx, ctx->st[6], fPs, cnt, &dfPs));
    TRY(stage_in(ctx, ctx->st[7], sPs, cnt, &dsPs));
    TRY(stage_in(ctx, ctx->st[3], sel, (size_t)n, &dsel));
    TRY(pks_cov_dev<T>(ctx, N, d, dFs, dQs, dfPs, dsPs, n, dsel, H, dout));
    TRY(stage_out(ctx, out, dout, nout));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGPS_OK;
}

template <typename T>
static int pks_cov_gains_dev(pgps_ctx* ctx, long N, int d, const T* Fs, const T* Qs, const T* fPs, long n, const long* sel,
                             T* B) {
    if (!ctx || N < 1 || N > 0x7fffffffL || n < 2 || n > N || !Fs || !Qs || !fPs || !sel || !B) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM_LANE) return PGPS_E_UNSUPPORTED_DIM;
    if (!aligned16(Fs) || !aligned16(Qs) || !aligned16(fPs) || !aligned16(B) || (((uintptr_t)sel) & 7u)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int* slot;
    TRY(cov_slots(ctx, N, n, sel, &slot));
    return cov_gains_run<T>(ctx, N, d, Fs, Qs, fPs, n, slot, B);
}

template <typename T>
static int cov_fill_dev(pgps_ctx* ctx, long n, int d, const T* B, const T* sPsel, const T* H, T* out) {
    if (!ctx || n < 1 || (n > 1 && !B) || !sPsel || !out) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM_LANE) return PGPS_E_UNSUPPORTED_DIM;
    if (!aligned16(B) || !aligned16(sPsel) || !aligned16(out)) return PGPS_E_INVALID;
    if (!cov_out_count(n, d, H != nullptr)) return PGPS_E_NOMEM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return cov_fill_run<T>(ctx, n, d, B, sPsel, H, out);
}

#define PGPS_DEFINE_COV(SUF, T)                                                                                             \
    extern "C" int pgps_pks_cov_##SUF(pgps_ctx* c, long N, int d, const T* Fs, const T* Qs, const T* fPs, const T* sPs,    \
                                      long n, const long* sel, const T* H, T* out) {                                       \
        return pks_cov_host<T>(c, N, d, Fs, Qs, fPs, sPs, n, sel, H, out);                                                 \
    }                                                                                                                       \
    extern "C" int pgps_pks_cov_dev_##SUF(pgps_ctx* c, long N, int d, const T* Fs, const T* Qs, const T* fPs,              \
                                          const T* sPs, long n, const long* sel, const T* H, T* out) {                     \
        return pks_cov_dev<T>(c, N, d, Fs, Qs, fPs, sPs, n, sel, H, out);                                                  \
    }                                                                                                                       \
    extern "C" int pgps_pks_cov_gains_dev_##SUF(pgps_ctx* c, long N, int d, const T* Fs, const T* Qs, const T* fPs,        \
                                                long n, const long* sel, T* B) {                                           \
        return pks_cov_gains_dev<T>(c, N, d, Fs, Qs, fPs, n, sel, B);                                                      \
    }                                                                                                                       \
    extern "C" int pgps_cov_fill_dev_##SUF(pgps_ctx* c, long n, int d, const T* B, const T* sPsel, const T* H, T* out) {   \
        return cov_fill_dev<T>(c, n, d, B, sPsel, H, out);                                                                 \
    }

PGPS_DEFINE_COV(f64, double)
PGPS_DEFINE_COV(f32, float)

// the model-level joint predictive: merge (k_merge_sorted: its qslot is the position of a query row in the selection),
// discretisation, filter + smoother over the N + K steps with the query rows missing, then the two passes between the
// query rows
static int lti_predict_cov_dev(pgps_ctx* ctx, long N, long K, int d, const double* F, const double* Pinf, const double* H,
                               double R, const double* ts, const double* ys, double t0, const double* tq, double* mean,
                               double* cov, double* ll) {
    if (!ctx || N < 1 || K < 1 || !F || !Pinf || !H || !ts || !ys || !tq || !mean || !cov) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM_LANE) return PGPS_E_UNSUPPORTED_DIM;
    if (N + K > 0x7fffffffL || !aligned16(cov)) return PGPS_E_INVALID;
    if (!cov_out_count(K, d, true)) return PGPS_E_NOMEM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t m = (size_t)(N + K);
    Merged<double> mg;
    LtiFront f;
    TRY(merged_front<double>(ctx, ctx->lti + 1, N, K, ts, ys, tq, &mg));
    TRY(lti_filter_front(ctx, m, d, F, Pinf, H, R, mg.ts, mg.ys, t0, true, ll, &f));
    return cov_core<double>(ctx, (long)m, d, f.Fs, f.Qs, f.fPs, f.sPs, K, mg.qslot, H, cov, f.sms, f.model + 2 * (size_t)d * d, mean);
}

static int lti_predict_cov_host(pgps_ctx* ctx, long N, long K, int d, const double* F, const double* Pinf, const double* H,
                                double R, const double* ts, const double* ys, double t0, const double* tq, double* mean,
                                double* cov, double* ll) {
    if (!ctx || N < 1 || K < 1 || !ts || !ys || !tq || !mean || !cov) return PGPS_E_INVALID;
    const size_t nout = cov_out_count(K, d, true);
    if (!nout) return PGPS_E_NOMEM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double *dts, *dys, *dtq, *dmean, *dcov, *dll;
    TRY(stage_in<double>(ctx, ctx->st[8], nullptr, nout, &dcov));
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    TRY(stage_in(ctx, ctx->st[3], tq, (size_t)K, &dtq));
    TRY(stage_in<double>(ctx, ctx->st[7], nullptr, (size_t)K, &dmean));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 2, &dll));
    TRY(lti_predict_cov_dev(ctx, N, K, d, F, Pinf, H, R, dts, dys, t0, dtq, dmean, dcov, dll));
    TRY(stage_out(ctx, mean, dmean, (size_t)K));
    TRY(stage_out(ctx, cov, dcov, nout));
    double llh = 0.0;
    TRY(stage_out(ctx, &llh, dll, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ll) *ll = llh;
    return std::isfinite(llh) ? PGPS_OK : PGPS_E_NUMERIC;
}

extern "C" int pgps_lti_predict_cov_f64(pgps_ctx* c, long N, long K, int d, const double* F, const double* Pinf,
                                        const double* H, double R, const double* ts, const double* ys, double t0,
                                        const double* tq, double* mean, double* cov, double* ll) {
    if (!F || !Pinf || !H) return PGPS_E_INVALID;
    if (d < 1 || d > PGPS_MAX_DIM_LANE) return PGPS_E_UNSUPPORTED_DIM;
    return lti_predict_cov_host(c, N, K, d, F, Pinf, H, R, ts, ys, t0, tq, mean, cov, ll);
}
extern "C" int pgps_lti_predict_cov_dev_f64(pgps_ctx* c, long N, long K, int d, const double* F, const double* Pinf,
                                            const double* H, double R, const double* ts, const double* ys, double t0,
                                            const double* tq, double* mean, double* cov, double* ll) {
    return lti_predict_cov_dev(c, N, K, d, F, Pinf, H, R, ts, ys, t0, tq, mean, cov, ll);
}
// Moments of the mixture sum_b w_b N(mean_b, var_b) per query column: mix = sum_b w_b mean_b, then
// var = sum_b w_b (var_b + (mean_b - mix)^2) -- two passes over the B rows, every term of the variance non-negative.  Lane x =
// query column (a wave reads 64 consecutive columns of a row: coalesced), the kMixRows lanes of a column take the rows
// b = y, y + kMixRows, ... and their partial sums are added in the order y = 0, 1, ...: the same bits on every run.
constexpr int kMixCols = 64, kMixRows = 8;
__global__ __launch_bounds__(kMixCols * kMixRows) void k_mix_moments(int B, long K, const double* __restrict__ mean,
                                                                     const double* __restrict__ var,
                                                                     const double* __restrict__ w, double* __restrict__ mean_out,
                                                                     double* __restrict__ var_out) {
    __shared__ double part[kMixRows][kMixCols];
    __shared__ double mix[kMixCols];
    const int x = threadIdx.x, y = threadIdx.y;
    const long k = (long)blockIdx.x * kMixCols + x;
    const bool in = k < K;
    const double equal = 1.0 / (double)B;
    double acc = 0.0;
    if (in)
        for (int b = y; b < B; b += kMixRows) acc += (w ? w[b] : equal) * mean[(size_t)b * K + k];
    part[y][x] = acc;
    __syncthreads();
    if (y == 0) {
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < kMixRows; ++r) t += part[r][x];
        mix[x] = t;
        if (in) mean_out[k] = t;
    }
    __syncthreads();
    const double mu = mix[x];
    acc = 0.0;
    if (in)
        for (int b = y; b < B; b += kMixRows) {
            const double dlt = mean[(size_t)b * K + k] - mu;
            acc += (w ? w[b] : equal) * (var[(size_t)b * K + k] + dlt * dlt);
        }
    part[y][x] = acc;
    __syncthreads();
    if (y == 0 && in) {
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < kMixRows; ++r) t += part[r][x];
        var_out[k] = t;
    }
}

int pgps::mix_moments_dev(pgps_ctx* ctx, int B, long K, const double* mean, const double* var, const double* w,
                           double* mean_out, double* var_out) {
    if (!ctx || B < 1 || K < 1 || !mean || !var || !mean_out || !var_out) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const dim3 grid((unsigned)((K + kMixCols - 1) / kMixCols)), block(kMixCols, kMixRows);
    k_mix_moments<<<grid, block, 0, ctx->stream>>>(B, K, mean, var, w, mean_out, var_out);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}
extern "C" int pgps_mix_moments_dev_f64(pgps_ctx* ctx, int B, long K, const double* mean, const double* var, const double* w,
                                        double* mean_out, double* var_out) {
    return mix_moments_dev(ctx, B, K, mean, var, w, mean_out, var_out);
}
