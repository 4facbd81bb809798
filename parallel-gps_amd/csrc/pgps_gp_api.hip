// pgps_gp_api.hip -- the fused Matern entry points of the C ABI (include/pgps.h, d <= 3: the discretisation happens inside
// the scan kernels): filter / smoother / log-likelihood, predict_f with the merge of training and query times (the merge
// kernel lives here), the batched log-likelihood and predict_f, and the gradient entry points.
#include "pgps_host.h"
#include "pgps_merge.hip.h"

using namespace pgps;

// ---------------------------------------------------------------------------------------------
// fused-discretisation ("gp") entry points
// ---------------------------------------------------------------------------------------------
template <typename T>
int pgps::gp_dev(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                  const double* H, double R, const T* ts, double t0, const T* ys, T* fms, T* fPs, T* sms, T* sPs,
                  double* ll) {
    RoctxRange range_("parallel_filter");
    if (!ctx || N < 1 || !N1 || !Pinf || !H || !ts || !ys) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    if ((fms == nullptr) != (fPs == nullptr) || (sms == nullptr) != (sPs == nullptr)) return PGPS_E_INVALID;
    if (!fms && !sms && !ll) return PGPS_E_INVALID;
    if ((fms && (!aligned16(fms) || !aligned16(fPs))) || (sms && (!aligned16(sms) || !aligned16(sPs))))
        return PGPS_E_INVALID;
    GpArgs<T> g{};
    g.s.N = N;
    g.s.R = (T)R;
    g.s.ys = ys;
    g.s.fms = fms; g.s.fPs = fPs; g.s.sms = sms; g.s.sPs = sPs; g.s.ll = ll;
    g.m.lam = lam;
    for (int i = 0; i < 9; ++i) { g.m.N1[i] = 0; g.m.N2[i] = 0; g.m.Pinf[i] = 0; }
    for (int i = 0; i < d * d; ++i) { g.m.N1[i] = N1[i]; g.m.N2[i] = N2 ? N2[i] : 0.0; g.m.Pinf[i] = Pinf[i]; }
    for (int i = 0; i < 3; ++i) g.m.H[i] = i < d ? (T)H[i] : T(0);
    g.m.ts = ts;
    g.m.t_prev = (T)t0;
    if constexpr (sizeof(T) == 8) {
        if (resident_fits(ctx, N, d, false) && aligned16(ts) && aligned16(ys)) {
            ResArgs<double> ra{};
            ra.s = g.s;
            ra.m = g.m;
            return launch_resident<double, 2>(ctx, ra, true, sms != nullptr);
        }
    }
    if (sms && !fms) return PGPS_E_INVALID;             // three launches: the smoother reads the filtered moments back
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp<T, D()>(ctx, g, fms != nullptr, sms != nullptr); });
}
template int pgps::gp_dev<double>(pgps_ctx*, long, int, double, const double*, const double*, const double*, const double*, double,
                                  const double*, double, const double*, double*, double*, double*, double*, double*);

// ll and the model's adjoints on the fused path: out = [ll | Abar (d d) | Ubar (d) | Hbar (d) | Rbar] on the device
int pgps::gp_adj_dev(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                      const double* H, double R, const double* ts, double t0, const double* ys, double* out) {
    RoctxRange range_("parallel_filter");
    if (!ctx || N < 1 || !N1 || !Pinf || !H || !ts || !ys || !out) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    GpArgs<double> g{};
    g.s.N = N;
    g.s.R = R;
    g.s.ys = ys;
    g.m.lam = lam;
    for (int i = 0; i < 9; ++i) { g.m.N1[i] = 0; g.m.N2[i] = 0; g.m.Pinf[i] = 0; }
    for (int i = 0; i < d * d; ++i) { g.m.N1[i] = N1[i]; g.m.N2[i] = N2 ? N2[i] : 0.0; g.m.Pinf[i] = Pinf[i]; }
    for (int i = 0; i < 3; ++i) g.m.H[i] = i < d ? H[i] : 0.0;
    g.m.ts = ts;
    g.m.t_prev = t0;
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_adj<double, D()>(ctx, g, out); });
}

extern "C" int pgps_gp_ll_grad_adj_dev_f64(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2,
                                           const double* Pinf, const double* H, double R, const double* ts, double t0,
                                           const double* ys, double* out) {
    return gp_adj_dev(ctx, N, d, lam, N1, N2, Pinf, H, R, ts, t0, ys, out);
}

template <typename T>
static int gp_host(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                   const double* H, double R, const T* ts, double t0, const T* ys, T* fms, T* fPs, T* sms, T* sPs,
                   double* ll) {
    if (!ctx || N < 1 || !ts || !ys) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)N, dd = (size_t)d * d;
    const bool wf = fms || fPs || sms || sPs, wsm = sms || sPs;
    if (!wf) {                  // log-likelihood only (a model's first objective): the small-call road
        SmallStage st(ctx, 2 * SmallStage::up(n * sizeof(T)), 16);
        if (st.ok) {
            double llh = 0.0;
            T* dys_ = st.in(ys, n);
            T* dts_ = st.in(ts, n);
            double* dll_ = st.out(&llh, 1);
            TRY(st.send());
            TRY(gp_dev<T>(ctx, N, d, lam, N1, N2, Pinf, H, R, dts_, t0, dys_, nullptr, nullptr, nullptr, nullptr, dll_));
            TRY(st.finish());
            if (ll) *ll = llh;
            return std::isfinite(llh) ? PGPS_OK : PGPS_E_NUMERIC;
        }
    }
    T *dts, *dys, *dfms = nullptr, *dfPs = nullptr, *dsms = nullptr, *dsPs = nullptr;
    double* dll;
    TRY(stage_in(ctx, ctx->st[4], ys, n, &dys));
    TRY(stage_in(ctx, ctx->st[10], ts, n, &dts));
    if (wf) {
        TRY(stage_in<T>(ctx, ctx->st[5], nullptr, n * d, &dfms));
        TRY(stage_in<T>(ctx, ctx->st[6], nullptr, n * dd, &dfPs));
    }
    if (wsm) {
        TRY(stage_in<T>(ctx, ctx->st[7], nullptr, n * d, &dsms));
        TRY(stage_in<T>(ctx, ctx->st[8], nullptr, n * dd, &dsPs));
    }
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 2, &dll));
    TRY(gp_dev<T>(ctx, N, d, lam, N1, N2, Pinf, H, R, dts, t0, dys, dfms, dfPs, dsms, dsPs, dll));
    if (fms) TRY(stage_out(ctx, fms, dfms, n * d));
    if (fPs) TRY(stage_out(ctx, fPs, dfPs, n * dd));
    if (sms) TRY(stage_out(ctx, sms, dsms, n * d));
    if (sPs) TRY(stage_out(ctx, sPs, dsPs, n * dd));
    double llh = 0.0;
    TRY(stage_out(ctx, &llh, dll, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ll) *ll = llh;
    if (!std::isfinite(llh)) return PGPS_E_NUMERIC;
    return PGPS_OK;
}

#define PGPS_DEFINE_GP(SUF, T)                                                                                       \
    extern "C" int pgps_gp_dev_##SUF(pgps_ctx* c, long N, int d, double lam, const double* N1, const double* N2,     \
                                     const double* Pinf, const double* H, double R, const T* ts, double t0,         \
                                     const T* ys, T* fms, T* fPs, T* sms, T* sPs, double* ll) {                     \
        return gp_dev<T>(c, N, d, lam, N1, N2, Pinf, H, R, ts, t0, ys, fms, fPs, sms, sPs, ll);                     \
    }                                                                                                                \
    extern "C" int pgps_gp_##SUF(pgps_ctx* c, long N, int d, double lam, const double* N1, const double* N2,         \
                                 const double* Pinf, const double* H, double R, const T* ts, double t0, const T* ys, \
                                 T* fms, T* fPs, T* sms, T* sPs, double* ll) {                                      \
        return gp_host<T>(c, N, d, lam, N1, N2, Pinf, H, R, ts, t0, ys, fms, fPs, sms, sPs, ll);                    \
    }

PGPS_DEFINE_GP(f64, double)
PGPS_DEFINE_GP(f32, float)

// ---------------------------------------------------------------------------------------------
// predict_f on the device: merge of the sorted training / query times, NaN marking of the query rows,
// fused filter + smoother, projection through H at the query rows only (pssgp/model.py:15-55,92-111)
// ---------------------------------------------------------------------------------------------
namespace pgps {

// the merge itself: pgps_merge.hip.h (merge_sorted_body), here on ONE series -- tile = blockIdx.x, a query row's slot is
// its index in tq
template <typename T, bool HET = false>
__global__ __launch_bounds__(kBlock) void k_merge_sorted(long N, long K, const T* ts, const T* ys, const T* tq, T* ts_m,
                                                          T* ys_m, int* qslot, const T* rs = nullptr, T* rs_m = nullptr) {
    __shared__ MergeLds<T, HET> sh;
    merge_sorted_body<T, HET>(sh, (long)blockIdx.x, N, K, ts, ys, tq, ts_m, ys_m, qslot, 0L, rs, rs_m);
}

template <typename T>
int launch_merge(pgps_ctx* ctx, long N, long K, const T* ts, const T* ys, const T* tq, T* ts_m, T* ys_m, int* qslot) {
    RoctxRange range_("merge_sorted");
    const long M = N + K;
    const dim3 grid((unsigned)((M + kMergeTile - 1) / kMergeTile)), block(kBlock);
    k_merge_sorted<T><<<grid, block, 0, ctx->stream>>>(N, K, ts, ys, tq, ts_m, ys_m, qslot);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}
template int launch_merge<double>(pgps_ctx*, long, long, const double*, const double*, const double*, double*, double*, int*);
template int launch_merge<float>(pgps_ctx*, long, long, const float*, const float*, const float*, float*, float*, int*);

// the same merge with rs woven next to ys (rs_m 16-byte aligned, as the other outputs are)
int launch_merge_het(pgps_ctx* ctx, long N, long K, const double* ts, const double* ys, const double* rs, const double* tq,
                     double* ts_m, double* ys_m, double* rs_m, int* qslot) {
    RoctxRange range_("merge_sorted");
    const long M = N + K;
    const dim3 grid((unsigned)((M + kMergeTile - 1) / kMergeTile)), block(kBlock);
    k_merge_sorted<double, true><<<grid, block, 0, ctx->stream>>>(N, K, ts, ys, tq, ts_m, ys_m, qslot, rs, rs_m);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

}  // namespace pgps

template <typename T>
static int gp_predict_dev(pgps_ctx* ctx, long N, long K, int d, double lam, const double* N1, const double* N2,
                          const double* Pinf, const double* H, double R, const T* ts, const T* ys, double t0,
                          const T* tq, T* mean, T* var, double* ll) {
    if (!ctx || N < 1 || K < 1 || !N1 || !Pinf || !H || !ts || !ys || !tq || !mean || !var) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    if (N + K > 0x7fffffffL) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t m = (size_t)(N + K), dd = (size_t)d * d;
    Merged<T> mg;
    T *fms, *fPs;
    double* dll;
    TRY(merged_front<T>(ctx, ctx->st, N, K, ts, ys, tq, &mg));
    TRY(stage_in<T>(ctx, ctx->st[5], nullptr, m * d, &fms));
    TRY(stage_in<T>(ctx, ctx->st[6], nullptr, m * dd, &fPs));
    TRY(stage_in<double>(ctx, ctx->st[11], nullptr, 2, &dll));
    GpArgs<T> g{};
    g.s.N = (long)m;
    g.s.R = (T)R;
    g.s.ys = mg.ys;
    g.s.fms = fms; g.s.fPs = fPs; g.s.sms = nullptr; g.s.sPs = nullptr;
    g.s.ll = ll ? ll : dll;
    g.m.lam = lam;
    for (int i = 0; i < 9; ++i) { g.m.N1[i] = 0; g.m.N2[i] = 0; g.m.Pinf[i] = 0; }
    for (int i = 0; i < d * d; ++i) { g.m.N1[i] = N1[i]; g.m.N2[i] = N2 ? N2[i] : 0.0; g.m.Pinf[i] = Pinf[i]; }
    for (int i = 0; i < 3; ++i) g.m.H[i] = i < d ? (T)H[i] : T(0);
    g.m.ts = mg.ts;
    g.m.t_prev = (T)t0;
    g.qslot = mg.qslot;
    g.pmean = mean;
    g.pvar = var;
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp<T, D()>(ctx, g, 1, 1); });
}

template <typename T>
static int gp_predict_host(pgps_ctx* ctx, long N, long K, int d, double lam, const double* N1, const double* N2,
                           const double* Pinf, const double* H, double R, const T* ts, const T* ys, double t0,
                           const T* tq, T* mean, T* var, double* ll) {
    if (!ctx || N < 1 || K < 1 || !ts || !ys || !tq || !mean || !var) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    {
        SmallStage st(ctx, 2 * SmallStage::up((size_t)N * sizeof(T)) + SmallStage::up((size_t)K * sizeof(T)),
                      2 * SmallStage::up((size_t)K * sizeof(T)) + 16);
        if (st.ok) {
            double llh = 0.0;
            T* dts = st.in(ts, (size_t)N);
            T* dys = st.in(ys, (size_t)N);
            T* dtq = st.in(tq, (size_t)K);
            double* dll = st.out(&llh, 1);
            T* dmean = st.out(mean, (size_t)K);
            T* dvar = st.out(var, (size_t)K);
            TRY(st.send());
            TRY(gp_predict_dev<T>(ctx, N, K, d, lam, N1, N2, Pinf, H, R, dts, dys, t0, dtq, dmean, dvar, dll));
            TRY(st.finish());
            if (ll) *ll = llh;
            return std::isfinite(llh) ? PGPS_OK : PGPS_E_NUMERIC;
        }
    }
    T *dts, *dys, *dtq, *dmean, *dvar;
    double* dll;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    TRY(stage_in(ctx, ctx->st[3], tq, (size_t)K, &dtq));
    TRY(stage_in<T>(ctx, ctx->st[7], nullptr, (size_t)K, &dmean));
    TRY(stage_in<T>(ctx, ctx->st[8], nullptr, (size_t)K, &dvar));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 2, &dll));
    TRY(gp_predict_dev<T>(ctx, N, K, d, lam, N1, N2, Pinf, H, R, dts, dys, t0, dtq, dmean, dvar, dll));
    TRY(stage_out(ctx, mean, dmean, (size_t)K));
    TRY(stage_out(ctx, var, dvar, (size_t)K));
    double llh = 0.0;
    TRY(stage_out(ctx, &llh, dll, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ll) *ll = llh;
    if (!std::isfinite(llh)) return PGPS_E_NUMERIC;
    return PGPS_OK;
}

#define PGPS_DEFINE_PREDICT(SUF, T)                                                                                  \
    extern "C" int pgps_gp_predict_dev_##SUF(pgps_ctx* c, long N, long K, int d, double lam, const double* N1,       \
                                             const double* N2, const double* Pinf, const double* H, double R,       \
                                             const T* ts, const T* ys, double t0, const T* tq, T* mean, T* var,     \
                                             double* ll) {                                                          \
        return gp_predict_dev<T>(c, N, K, d, lam, N1, N2, Pinf, H, R, ts, ys, t0, tq, mean, var, ll);                \
    }                                                                                                                \
    extern "C" int pgps_gp_predict_##SUF(pgps_ctx* c, long N, long K, int d, double lam, const double* N1,           \
                                         const double* N2, const double* Pinf, const double* H, double R,           \
                                         const T* ts, const T* ys, double t0, const T* tq, T* mean, T* var,         \
                                         double* ll) {                                                              \
        return gp_predict_host<T>(c, N, K, d, lam, N1, N2, Pinf, H, R, ts, ys, t0, tq, mean, var, ll);               \
    }

PGPS_DEFINE_PREDICT(f64, double)
PGPS_DEFINE_PREDICT(f32, float)
// ---------------------------------------------------------------------------------------------
// batched log-likelihood: B hyper-parameter settings over one series
// ---------------------------------------------------------------------------------------------
// models: B blocks [lam | N1 (d*d) | N2 (d*d) | Pinf (d*d) | H (d) | R] from the caller, re-packed to the fixed device
// stride (kGpModelStride); lam <= 0 or R <= 0 in any row: PGPS_E_INVALID
static int gp_pack_models(int B, int d, const double* models_host, std::vector<double>& packed) {
    packed.assign((size_t)B * kGpModelStride, 0.0);
    const int in_stride = 1 + 3 * d * d + d + 1;
    for (int m = 0; m < B; ++m) {
        const double* p = models_host + (size_t)m * in_stride;
        double* q = packed.data() + (size_t)m * kGpModelStride;
        q[0] = p[0];
        for (int i = 0; i < d * d; ++i) { q[1 + i] = p[1 + i]; q[10 + i] = p[1 + d * d + i]; q[19 + i] = p[1 + 2 * d * d + i]; }
        for (int i = 0; i < d; ++i) q[28 + i] = p[1 + 3 * d * d + i];
        q[31] = p[1 + 3 * d * d + d];
        if (!(q[0] > 0.0) || !(q[31] > 0.0)) return PGPS_E_INVALID;
    }
    return PGPS_OK;
}

template <typename T>
static int gp_ll_batch_dev(pgps_ctx* ctx, int B, long N, int d, const double* models_host, const T* ts, double t0,
                           const T* ys, double* ll) {
    if (!ctx || B < 1 || B > 65535 || N < 1 || !models_host || !ts || !ys || !ll) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<double> packed;
    TRY(gp_pack_models(B, d, models_host, packed));
    double* dmodels;
    TRY(stage_in<double>(ctx, ctx->st[0], nullptr, packed.size(), &dmodels));
    // the packed vector dies with this frame: synchronous copy (pageable memory, so hipMemcpyAsync would
    // stage it anyway)
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(dmodels, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice));
    GpBatchArgs<T> b{};
    b.N = N;
    b.ts = ts;
    b.ys = ys;
    b.t_prev = (T)t0;
    b.models = dmodels;
    b.ll = ll;
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_batch<T, D()>(ctx, B, b); });
}

template <typename T>
static int gp_ll_batch_host(pgps_ctx* ctx, int B, long N, int d, const double* models, const T* ts, double t0,
                            const T* ys, double* ll) {
    if (!ctx || B < 1 || N < 1 || !ts || !ys || !ll) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    T *dts, *dys;
    double* dll;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)B, &dll));
    TRY(gp_ll_batch_dev<T>(ctx, B, N, d, models, dts, t0, dys, dll));
    TRY(stage_out(ctx, ll, dll, (size_t)B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGPS_OK;
}

#define PGPS_DEFINE_LL_BATCH(SUF, T)                                                                                \
    extern "C" int pgps_gp_ll_batch_dev_##SUF(pgps_ctx* c, int B, long N, int d, const double* models, const T* ts, \
                                              double t0, const T* ys, double* ll) {                                \
        return gp_ll_batch_dev<T>(c, B, N, d, models, ts, t0, ys, ll);                                              \
    }                                                                                                               \
    extern "C" int pgps_gp_ll_batch_##SUF(pgps_ctx* c, int B, long N, int d, const double* models, const T* ts,     \
                                          double t0, const T* ys, double* ll) {                                    \
        return gp_ll_batch_host<T>(c, B, N, d, models, ts, t0, ys, ll);                                             \
    }

PGPS_DEFINE_LL_BATCH(f64, double)
PGPS_DEFINE_LL_BATCH(f32, float)

// ---------------------------------------------------------------------------------------------
// batched predict_f: B hyper-parameter settings over one series and one query grid (fused path, d <= 3)
// ---------------------------------------------------------------------------------------------
// the B models over an ALREADY MERGED series of m steps (ts_m, ys_m, qslot on the device); mean, var (B, K), ll (B) device
template <typename T>
int pgps::gp_predict_batch_merged(pgps_ctx* ctx, int B, size_t m, long K, int d, const double* models_host, const T* ts_m,
                                   const T* ys_m, double t0, const int* qslot, T* mean, T* var, double* ll) {
    std::vector<double> packed;
    TRY(gp_pack_models(B, d, models_host, packed));
    double* dmodels;
    TRY(stage_in<double>(ctx, ctx->st[5], nullptr, packed.size(), &dmodels));
    // the packed vector dies with this frame: synchronous copy, as in gp_ll_batch_dev
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(dmodels, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice));
    GpBatchArgs<T> b{};
    b.N = (long)m;
    b.ts = ts_m;
    b.ys = ys_m;
    b.t_prev = (T)t0;
    b.models = dmodels;
    b.ll = ll;
    b.qslot = qslot;
    b.pmean = mean;
    b.pvar = var;
    b.K = K;
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_predict_batch<T, D()>(ctx, B, b); });     // (the callers have refused d > 3)
}
template int pgps::gp_predict_batch_merged<double>(pgps_ctx*, int, size_t, long, int, const double*, const double*, const double*,
                                                   double, const int*, double*, double*, double*);

template <typename T>
static int gp_predict_batch_dev(pgps_ctx* ctx, int B, long N, long K, int d, const double* models_host, const T* ts,
                                const T* ys, double t0, const T* tq, T* mean, T* var, double* ll) {
    if (!ctx || B < 1 || N < 1 || K < 1 || !models_host || !ts || !ys || !tq || !mean || !var) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    if (N + K > 0x7fffffffL) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t m = (size_t)(N + K);
    Merged<T> mg;
    double* dll = ll;
    TRY(merged_front<T>(ctx, ctx->st, N, K, ts, ys, tq, &mg));             // ONE merge, shared by all models
    if (!dll) TRY(stage_in<double>(ctx, ctx->st[11], nullptr, (size_t)B, &dll));
    return gp_predict_batch_merged<T>(ctx, B, m, K, d, models_host, mg.ts, mg.ys, t0, mg.qslot, mean, var, dll);
}

template <typename T>
static int gp_predict_batch_host(pgps_ctx* ctx, int B, long N, long K, int d, const double* models, const T* ts, const T* ys,
                                 double t0, const T* tq, T* mean, T* var, double* ll) {
    if (!ctx || B < 1 || N < 1 || K < 1 || !models || !ts || !ys || !tq || !mean || !var) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t bk = (size_t)B * (size_t)K;
    T *dts, *dys, *dtq, *dmean, *dvar;
    double* dll;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    TRY(stage_in(ctx, ctx->st[3], tq, (size_t)K, &dtq));
    TRY(stage_in<T>(ctx, ctx->st[7], nullptr, bk, &dmean));
    TRY(stage_in<T>(ctx, ctx->st[8], nullptr, bk, &dvar));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)B, &dll));
    TRY(gp_predict_batch_dev<T>(ctx, B, N, K, d, models, dts, dys, t0, dtq, dmean, dvar, dll));
    return copy_out_batch(ctx, B, {mean, dmean, bk * sizeof(T)}, {var, dvar, bk * sizeof(T)}, dll, ll);
}

#define PGPS_DEFINE_PREDICT_BATCH(SUF, T)                                                                             \
    extern "C" int pgps_gp_predict_batch_dev_##SUF(pgps_ctx* c, int B, long N, long K, int d, const double* models,   \
                                                   const T* ts, const T* ys, double t0, const T* tq, T* mean, T* var, \
                                                   double* ll) {                                                      \
        return gp_predict_batch_dev<T>(c, B, N, K, d, models, ts, ys, t0, tq, mean, var, ll);                         \
    }                                                                                                                 \
    extern "C" int pgps_gp_predict_batch_##SUF(pgps_ctx* c, int B, long N, long K, int d, const double* models,       \
                                               const T* ts, const T* ys, double t0, const T* tq, T* mean, T* var,     \
                                               double* ll) {                                                          \
        return gp_predict_batch_host<T>(c, B, N, K, d, models, ts, ys, t0, tq, mean, var, ll);                        \
    }

PGPS_DEFINE_PREDICT_BATCH(f64, double)
PGPS_DEFINE_PREDICT_BATCH(f32, float)
// ---------------------------------------------------------------------------------------------
// batched log-likelihood and adjoints: B hyper-parameter settings over one series (fused path, d <= 3, fp64)
// ---------------------------------------------------------------------------------------------
// out (B, 1 + d d + 2 d + 1) on the device: row b = [ll | Abar | Ubar | Hbar | Rbar] of model b, as gp_adj_dev defines it
int pgps::gp_adj_batch_dev(pgps_ctx* ctx, int B, long N, int d, const double* models_host, const double* ts, double t0,
                           const double* ys, double* out) {
    if (!ctx || B < 1 || N < 1 || !models_host || !ts || !ys || !out) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<double> packed;
    TRY(gp_pack_models(B, d, models_host, packed));
    double* dmodels;
    TRY(stage_in<double>(ctx, ctx->st[0], nullptr, packed.size(), &dmodels));
    // the packed vector dies with this frame: synchronous copy, as in gp_ll_batch_dev
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(dmodels, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice));
    GpBatchArgs<double> b{};
    b.N = N;
    b.ts = ts;
    b.ys = ys;
    b.t_prev = t0;
    b.models = dmodels;
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_adj_batch<double, D()>(ctx, B, b, out); });
}

// rows on the host: PGPS_E_NUMERIC when a row's log-likelihood is not finite
int pgps::adj_batch_result(int B, int nout, const double* rows) {
    for (int m = 0; m < B; ++m)
        if (!std::isfinite(rows[(size_t)m * nout])) return PGPS_E_NUMERIC;
    return PGPS_OK;
}

extern "C" int pgps_gp_ll_grad_adj_batch_dev_f64(pgps_ctx* ctx, int B, long N, int d, const double* models, const double* ts,
                                                 double t0, const double* ys, double* out) {
    return gp_adj_batch_dev(ctx, B, N, d, models, ts, t0, ys, out);
}

extern "C" int pgps_gp_ll_grad_adj_batch_f64(pgps_ctx* ctx, int B, long N, int d, const double* models, const double* ts,
                                             double t0, const double* ys, double* out) {
    if (!ctx || B < 1 || N < 1 || !models || !ts || !ys || !out) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int nout = 1 + d * d + 2 * d + 1;
    double *dts, *dys, *dout;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)B * nout, &dout));
    TRY(gp_adj_batch_dev(ctx, B, N, d, models, dts, t0, dys, dout));
    TRY(stage_out(ctx, out, dout, (size_t)B * nout));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return adj_batch_result(B, nout, out);
}
// ---------------------------------------------------------------------------------------------
// log-likelihood and its gradient (fused path, forward-mode duals through the scan)
// ---------------------------------------------------------------------------------------------
extern "C" int pgps_gp_ll_grad_dev_f64(pgps_ctx* ctx, long N, int d, int np, const double* model, const double* ts,
                                       double t0, const double* ys, double* out) {
    if (!ctx || N < 1 || !model || !ts || !ys || !out) return PGPS_E_INVALID;
    return launch_grad(ctx, N, d, np, model, ts, t0, ys, out);
}

static int gradb_dispatch(pgps_ctx* ctx, long N, int d, int nblk, const int* bsize, int np, const double* model,
                          const double* ts, double t0, const double* ys, double* out) {
    if (!ctx || N < 1 || !bsize || !model || !ts || !ys || !out) return PGPS_E_INVALID;
    if (nblk < 1 || nblk > 4 || np < 1 || np > 16) return PGPS_E_INVALID;
    int sum = 0;
    for (int b = 0; b < nblk; ++b) { if (bsize[b] < 1) return PGPS_E_INVALID; sum += bsize[b]; }
    if (sum != d) return PGPS_E_INVALID;
    RoctxRange range_("parallel_filter");
    return for_dim<2, 6>(d, [&](auto D) { return launch_gradb<D()>(ctx, N, nblk, bsize, np, model, ts, t0, ys, out); });
}

extern "C" int pgps_gp_ll_grad_blocks_dev_f64(pgps_ctx* ctx, long N, int d, int nblk, const int* bsize, int np,
                                              const double* model, const double* ts, double t0, const double* ys,
                                              double* out) {
    return gradb_dispatch(ctx, N, d, nblk, bsize, np, model, ts, t0, ys, out);
}

extern "C" int pgps_gp_ll_grad_blocks_f64(pgps_ctx* ctx, long N, int d, int nblk, const int* bsize, int np,
                                          const double* model, const double* ts, double t0, const double* ys, double* out) {
    if (!ctx || N < 1 || !model || !ts || !ys || !out || np < 1 || np > 16) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double *dts, *dys, *dout;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)(1 + 3 * np), &dout));
    TRY(gradb_dispatch(ctx, N, d, nblk, bsize, np, model, dts, t0, dys, dout));
    TRY(stage_out(ctx, out, dout, (size_t)(1 + np)));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (!std::isfinite(out[0])) return PGPS_E_NUMERIC;
    return PGPS_OK;
}

extern "C" int pgps_gp_ll_grad_f64(pgps_ctx* ctx, long N, int d, int np, const double* model, const double* ts,
                                   double t0, const double* ys, double* out) {
    if (!ctx || N < 1 || !model || !ts || !ys || !out) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double *dts, *dys, *dout;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 16, &dout));
    TRY(launch_grad(ctx, N, d, np, model, dts, t0, dys, dout));
    TRY(stage_out(ctx, out, dout, (size_t)(1 + np)));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (!std::isfinite(out[0])) return PGPS_E_NUMERIC;
    return PGPS_OK;
}
