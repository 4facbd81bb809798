// pgps_series.hip -- the pgps_series handle of the C ABI (include/pgps.h): a series (and its merged query grid) kept on the
// device across calls, and every pgps_series_* entry point.  The work itself is the other host units' (pgps_host.h).
#include <new>

#include "pgps_host.h"
#include "pgps_gradlti.h"

using namespace pgps;

// ---------------------------------------------------------------------------------------------
// A series kept on the device across calls (round 3).  The reference's drivers evaluate the SAME (ts, ys) thousands of
// times with changing hyper-parameters (L-BFGS: pssgp/experiments/sunspot/map.py:74-82; HMC: experiments/common.py:95-133;
// the speed mesh calls predict_f on fixed grids: toy_models/speed_and_stability.py:73-87): with the host entry points every
// call copied ts and ys to the device again, merged the query grid again and waited for three or four staged copies.
// A pgps_series holds ts, ys (and, once set, the query grid MERGED with them: times, observations with NaN at the query
// rows, query slots) on the device, so that a call sends the model's few scalars and brings back the log-likelihood
// (+ gradient, or the K means and variances) through a pinned buffer: one short launch set and one copy per call.
// fp64, the fused (Matern-family, d <= 3) entry points.
// ---------------------------------------------------------------------------------------------
struct pgps_series {
    pgps_ctx* ctx = nullptr;
    long N = 0, K = 0;
    double t0 = 0.0;
    double *ts = nullptr, *ys = nullptr, *tq = nullptr;
    double *ts_m = nullptr, *ys_m = nullptr, *fms = nullptr, *fPs = nullptr, *pm = nullptr, *pv = nullptr, *res = nullptr;
    int* qslot = nullptr;
    double* host = nullptr;             // pinned: 2 K + 32 doubles
    double* hdev = nullptr;             // the same buffer as the device sees it: the last kernel of a call writes its results
                                        // straight into it (a D2H copy is a blit kernel of its own: ~5 us each, three per
                                        // predict_f; PGPS_SERIES_ZERO_COPY=0 in the environment brings the copies back)
    bool zero_copy = true;
    size_t host_cap = 0;
};

static void series_free_queries(pgps_series* s) {
    for (void* p : {(void*)s->tq, (void*)s->ts_m, (void*)s->ys_m, (void*)s->fms, (void*)s->fPs, (void*)s->pm, (void*)s->pv, (void*)s->qslot})
        if (p) (void)hipFree(p);
    s->tq = s->ts_m = s->ys_m = s->fms = s->fPs = s->pm = s->pv = nullptr;
    s->qslot = nullptr;
    s->K = 0;
}
static int series_host(pgps_series* s, size_t doubles) {
    if (s->host_cap >= doubles) return PGPS_OK;
    if (s->host) (void)hipHostFree(s->host);
    s->host = nullptr; s->host_cap = 0; s->hdev = nullptr;
    if (hipHostMalloc((void**)&s->host, doubles * sizeof(double), hipHostMallocDefault) != hipSuccess) {
        s->host = nullptr;
        (void)hipGetLastError();                    // reported here: the next call's launch check must not find it
        return PGPS_E_NOMEM;
    }
    s->host_cap = doubles;
    const char* env = std::getenv("PGPS_SERIES_ZERO_COPY");
    s->zero_copy = !(env && env[0] == '0');
    s->hdev = nullptr;
    if (s->zero_copy && hipHostGetDevicePointer((void**)&s->hdev, s->host, 0) != hipSuccess) { s->hdev = nullptr; s->zero_copy = false; }
    return PGPS_OK;
}

extern "C" int pgps_series_destroy(pgps_series* s) {
    if (!s) return PGPS_OK;
    if (s->ctx) { (void)hipSetDevice(s->ctx->device); (void)hipStreamSynchronize(s->ctx->stream); }
    series_free_queries(s);
    if (s->ts) (void)hipFree(s->ts);
    if (s->ys) (void)hipFree(s->ys);
    if (s->res) (void)hipFree(s->res);
    if (s->host) (void)hipHostFree(s->host);
    delete s;
    return PGPS_OK;
}

extern "C" int pgps_series_create_f64(pgps_ctx* ctx, long N, const double* ts, const double* ys, double t0, pgps_series** out) {
    if (!ctx || N < 1 || !ts || !ys || !out) return PGPS_E_INVALID;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pgps_series* s = new (std::nothrow) pgps_series();
    if (!s) return PGPS_E_NOMEM;
    s->ctx = ctx; s->N = N; s->t0 = t0;
    const size_t nb = (size_t)N * sizeof(double);
    if (hipMalloc((void**)&s->ts, nb) != hipSuccess || hipMalloc((void**)&s->ys, nb) != hipSuccess ||
        hipMalloc((void**)&s->res, 64 * sizeof(double)) != hipSuccess || series_host(s, 64) != PGPS_OK) {
        pgps_series_destroy(s);
        return PGPS_E_NOMEM;
    }
    if (hipMemcpyAsync(s->ts, ts, nb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(s->ys, ys, nb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
        pgps_series_destroy(s);
        return PGPS_E_HIP;
    }
    *out = s;
    return PGPS_OK;
}

// the query grid of predict_f: merged with the training series on the device ONCE (pssgp/model.py:15-55 tie rule)
extern "C" int pgps_series_set_queries_f64(pgps_series* s, long K, const double* tq) {
    if (!s || K < 0 || (K > 0 && !tq)) return PGPS_E_INVALID;
    pgps_ctx* ctx = s->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    series_free_queries(s);
    if (K == 0) return PGPS_OK;
    if (s->N + K > 0x7fffffffL) return PGPS_E_INVALID;
    const size_t m = (size_t)(s->N + K);
    if (hipMalloc((void**)&s->tq, (size_t)K * 8) != hipSuccess || hipMalloc((void**)&s->ts_m, m * 8) != hipSuccess ||
        hipMalloc((void**)&s->ys_m, m * 8) != hipSuccess || hipMalloc((void**)&s->qslot, m * 4) != hipSuccess ||
        hipMalloc((void**)&s->fms, m * 3 * 8) != hipSuccess || hipMalloc((void**)&s->fPs, m * 9 * 8) != hipSuccess ||
        hipMalloc((void**)&s->pm, (size_t)K * 8) != hipSuccess || hipMalloc((void**)&s->pv, (size_t)K * 8) != hipSuccess ||
        series_host(s, 2 * (size_t)K + 64) != PGPS_OK) {
        series_free_queries(s);
        return PGPS_E_NOMEM;
    }
    s->K = K;
    HIPCHK(ctx, hipMemcpyAsync(s->tq, tq, (size_t)K * 8, hipMemcpyHostToDevice, ctx->stream));
    TRY(pgps::launch_merge<double>(ctx, s->N, K, s->ts, s->ys, s->tq, s->ts_m, s->ys_m, s->qslot));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGPS_OK;
}

extern "C" int pgps_series_info(pgps_series* s, long* N, long* K) {
    if (!s || !N || !K) return PGPS_E_INVALID;
    *N = s->N; *K = s->K;
    return PGPS_OK;
}

// log-likelihood of the fused model on the resident series; ll on the host when the call returns
extern "C" int pgps_series_gp_ll_f64(pgps_series* s, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                                     const double* H, double R, double* ll) {
    if (!s || !ll) return PGPS_E_INVALID;
    pgps_ctx* ctx = s->ctx;
    double* const res = s->zero_copy ? s->hdev : s->res;
    TRY(gp_dev<double>(ctx, s->N, d, lam, N1, N2, Pinf, H, R, s->ts, s->t0, s->ys, nullptr, nullptr, nullptr, nullptr, res));
    if (!s->zero_copy) HIPCHK(ctx, hipMemcpyAsync(s->host, s->res, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *ll = s->host[0];
    return std::isfinite(*ll) ? PGPS_OK : PGPS_E_NUMERIC;
}

// log-likelihood and its gradient (forward-mode duals, pgps_gp_ll_grad_*): out = [ll, d ll / d theta_1 .. np] on the host
extern "C" int pgps_series_gp_ll_grad_f64(pgps_series* s, int d, int np, const double* model, double* out) {
    if (!s || !model || !out || np < 1 || np > 16) return PGPS_E_INVALID;
    pgps_ctx* ctx = s->ctx;
    TRY(launch_grad(ctx, s->N, d, np, model, s->ts, s->t0, s->ys, s->zero_copy ? s->hdev : s->res));
    if (!s->zero_copy) HIPCHK(ctx, hipMemcpyAsync(s->host, s->res, (size_t)(1 + np) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i <= np; ++i) out[i] = s->host[i];
    return std::isfinite(out[0]) ? PGPS_OK : PGPS_E_NUMERIC;
}

// log-likelihood and the model's adjoints (the adjoint pass, pgps_gpadj.hip.h): out = 1 + d d + 2 d + 1 doubles on the host
extern "C" int pgps_series_gp_ll_grad_adj_f64(pgps_series* s, int d, double lam, const double* N1, const double* N2,
                                              const double* Pinf, const double* H, double R, double* out) {
    if (!s || !out) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    pgps_ctx* ctx = s->ctx;
    const int n = 1 + d * d + 2 * d + 1;
    double* const res = s->zero_copy ? s->hdev : s->res;
    TRY(gp_adj_dev(ctx, s->N, d, lam, N1, N2, Pinf, H, R, s->ts, s->t0, s->ys, res));
    if (!s->zero_copy) HIPCHK(ctx, hipMemcpyAsync(s->host, s->res, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; ++i) out[i] = s->host[i];
    return std::isfinite(out[0]) ? PGPS_OK : PGPS_E_NUMERIC;
}

// Where the B result rows of a batched gradient call on the resident series go: a small result straight into the pinned
// buffer (grown if need be), as the single call's; else a staging buffer of the context
static int series_rows_begin(pgps_series* s, size_t n, double** dout) {
    pgps_ctx* ctx = s->ctx;
    *dout = nullptr;
    if (s->zero_copy && n * sizeof(double) <= ((size_t)8 << 20)) {
        if (n > s->host_cap) {
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // (the buffer is replaced: nothing may still write it)
            if (series_host(s, n + 64) != PGPS_OK && series_host(s, 2 * (size_t)s->K + 64) != PGPS_OK) return PGPS_E_NOMEM;
        }
        if (s->zero_copy && n <= s->host_cap) *dout = s->hdev;
    }
    if (!*dout) TRY(stage_in<double>(ctx, ctx->st[9], nullptr, n, dout));
    return PGPS_OK;
}
static int series_rows_end(pgps_series* s, int B, int nout, const double* dout, double* out) {
    pgps_ctx* ctx = s->ctx;
    const size_t n = (size_t)B * nout;
    if (dout != s->hdev) {
        TRY(stage_out(ctx, out, dout, n));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    } else {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(out, s->host, n * sizeof(double));
    }
    return adj_batch_result(B, nout, out);
}

// the same for B models (pgps_gp_ll_grad_adj_batch_f64) on the resident series: out (B, 1 + d d + 2 d + 1) on the host
extern "C" int pgps_series_gp_ll_grad_adj_batch_f64(pgps_series* s, int B, int d, const double* models, double* out) {
    if (!s || B < 1 || !models || !out) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    pgps_ctx* ctx = s->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int nout = 1 + d * d + 2 * d + 1;
    double* dout;
    TRY(series_rows_begin(s, (size_t)B * nout, &dout));
    TRY(gp_adj_batch_dev(ctx, B, s->N, d, models, s->ts, s->t0, s->ys, dout));
    return series_rows_end(s, B, nout, dout, out);
}
// ... and for B general LTI models [F | Pinf | H | R] of one state dimension 2 .. 16 (pgps_lti_ll_grad_batch_f64)
extern "C" int pgps_series_lti_ll_grad_batch_f64(pgps_series* s, int B, int d, const double* models, double* out) {
    if (!s || B < 1 || !models || !out) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > rc::kDimMax) return PGPS_E_UNSUPPORTED_DIM;
    pgps_ctx* ctx = s->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int nout = 1 + grad_lti_nstat(d);
    double* dout;
    TRY(series_rows_begin(s, (size_t)B * nout, &dout));
    TRY(lti_grad_batch_dev(ctx, B, s->N, d, models, s->ts, s->ys, s->t0, dout));
    return series_rows_end(s, B, nout, dout, out);
}

// predict_f at the query grid set by pgps_series_set_queries_f64: K means and variances (and the log-likelihood of the
// training series: the query rows are missing observations and contribute nothing) on the host when the call returns
extern "C" int pgps_series_gp_predict_f64(pgps_series* s, int d, double lam, const double* N1, const double* N2,
                                          const double* Pinf, const double* H, double R, double* mean, double* var, double* ll) {
    if (!s || s->K < 1 || !mean || !var || !N1 || !Pinf || !H) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    pgps_ctx* ctx = s->ctx;
    RoctxRange range_("parallel_filter");
    GpArgs<double> g{};
    g.s.N = s->N + s->K;
    g.s.R = R;
    g.s.ys = s->ys_m;
    g.s.fms = s->fms; g.s.fPs = s->fPs; g.s.sms = nullptr; g.s.sPs = nullptr;
    const size_t K = (size_t)s->K;
    g.s.ll = s->zero_copy ? s->hdev + 2 * K : s->res;
    g.m.lam = lam;
    for (int i = 0; i < 9; ++i) { g.m.N1[i] = 0; g.m.N2[i] = 0; g.m.Pinf[i] = 0; }
    for (int i = 0; i < d * d; ++i) { g.m.N1[i] = N1[i]; g.m.N2[i] = N2 ? N2[i] : 0.0; g.m.Pinf[i] = Pinf[i]; }
    for (int i = 0; i < 3; ++i) g.m.H[i] = i < d ? H[i] : 0.0;
    g.m.ts = s->ts_m;
    g.m.t_prev = s->t0;
    g.qslot = s->qslot;
    g.pmean = s->zero_copy ? s->hdev : s->pm;
    g.pvar = s->zero_copy ? s->hdev + K : s->pv;
    TRY((for_dim<1, 3>(d, [&](auto D) { return launch_gp<double, D()>(ctx, g, 1, 1); })));
    if (!s->zero_copy) {
        HIPCHK(ctx, hipMemcpyAsync(s->host, s->pm, K * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(s->host + K, s->pv, K * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(s->host + 2 * K, s->res, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(mean, s->host, K * 8);
    std::memcpy(var, s->host + K, K * 8);
    if (ll) *ll = s->host[2 * K];
    return std::isfinite(s->host[2 * K]) ? PGPS_OK : PGPS_E_NUMERIC;
}
// the same three calls for ANY kernel's LTI model (F, Pinf, H from the host; fp64, 2 <= d <= 32): pgps_lti_ll_* /
// pgps_lti_predict_* / pgps_lti_ll_batch_* on the resident series and its merged query grid
extern "C" int pgps_series_lti_ll_f64(pgps_series* s, int d, const double* F, const double* Pinf, const double* H, double R,
                                      double* ll) {
    if (!s || !ll || !F || !Pinf || !H) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    pgps_ctx* ctx = s->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double* const res = s->zero_copy ? s->hdev : s->res;
    TRY(lti_core(ctx, (size_t)s->N, d, F, Pinf, H, R, s->ts, s->ys, s->t0, nullptr, nullptr, nullptr, res));
    if (!s->zero_copy) HIPCHK(ctx, hipMemcpyAsync(s->host, s->res, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *ll = s->host[0];
    return std::isfinite(*ll) ? PGPS_OK : PGPS_E_NUMERIC;
}

extern "C" int pgps_series_lti_predict_f64(pgps_series* s, int d, const double* F, const double* Pinf, const double* H, double R,
                                           double* mean, double* var, double* ll) {
    if (!s || s->K < 1 || !mean || !var || !F || !Pinf || !H) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    pgps_ctx* ctx = s->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t K = (size_t)s->K;
    double* const dm = s->zero_copy ? s->hdev : s->pm;
    double* const dv = s->zero_copy ? s->hdev + K : s->pv;
    double* const dl = s->zero_copy ? s->hdev + 2 * K : s->res;
    TRY(lti_core(ctx, (size_t)(s->N + s->K), d, F, Pinf, H, R, s->ts_m, s->ys_m, s->t0, s->qslot, dm, dv, dl));
    if (!s->zero_copy) {
        HIPCHK(ctx, hipMemcpyAsync(s->host, s->pm, K * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(s->host + K, s->pv, K * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(s->host + 2 * K, s->res, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(mean, s->host, K * 8);
    std::memcpy(var, s->host + K, K * 8);
    if (ll) *ll = s->host[2 * K];
    return std::isfinite(s->host[2 * K]) ? PGPS_OK : PGPS_E_NUMERIC;
}

extern "C" int pgps_series_lti_ll_batch_f64(pgps_series* s, int B, int d, const double* models, double* ll) {
    if (!s || B < 1 || !models || !ll) return PGPS_E_INVALID;
    pgps_ctx* ctx = s->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double* dll;
    if (s->zero_copy && (size_t)B <= s->host_cap) dll = s->hdev;
    else TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)B, &dll));
    TRY(lti_ll_batch_dev(ctx, B, s->N, d, models, s->ts, s->ys, s->t0, dll));
    if (dll != s->hdev) {
        TRY(stage_out(ctx, ll, dll, (size_t)B));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return PGPS_OK;
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(ll, s->host, (size_t)B * sizeof(double));
    return PGPS_OK;
}
extern "C" int pgps_series_lti_ll_grad_f64(pgps_series* s, int d, const double* F, const double* Pinf, const double* H, double R,
                                           double* out) {
    if (!s || !out || !F || !Pinf || !H) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    pgps_ctx* ctx = s->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nout = 1 + (size_t)grad_lti_nstat(d);
    TRY(series_host(s, std::max<size_t>(nout, s->host_cap)));
    double* dout;
    if (s->zero_copy) dout = s->hdev;
    else TRY(stage_in<double>(ctx, ctx->st[9], nullptr, nout, &dout));
    TRY(lti_grad_dev(ctx, s->N, d, F, Pinf, H, R, s->ts, s->ys, s->t0, dout));
    if (!s->zero_copy) HIPCHK(ctx, hipMemcpyAsync(s->host, dout, nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(out, s->host, nout * sizeof(double));
    return std::isfinite(out[0]) ? PGPS_OK : PGPS_E_NUMERIC;
}
// Results of a batch on a resident series.  Small unreduced results are written by the kernels straight into the series'
// pinned host buffer, as the single predict's are (no copy-back blit: at N = 2^17, K = 2^15, B = 8 the bounce through
// copy_out made the batch slower than eight single calls); larger ones and the mixture go through copy_out.
constexpr size_t kBatchZeroCopyMax = (size_t)8 << 20;
struct SeriesBatchOut {
    double *dmean = nullptr, *dvar = nullptr, *dll = nullptr, *dmix = nullptr, *dw = nullptr;
    bool zero = false;
};
static int series_batch_begin(pgps_series* s, int B, const double* w, SeriesBatchOut& o) {
    pgps_ctx* ctx = s->ctx;
    const size_t K = (size_t)s->K, bk = (size_t)B * K;
    if (!w && s->zero_copy && (2 * bk + (size_t)B) * sizeof(double) <= kBatchZeroCopyMax) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));         // (the buffer may be replaced: nothing may still write it)
        if (series_host(s, 2 * bk + (size_t)B + 64) == PGPS_OK && s->zero_copy) {
            o.zero = true;
            o.dmean = s->hdev; o.dvar = s->hdev + bk; o.dll = s->hdev + 2 * bk;
            return PGPS_OK;
        }
        // the pinned buffer could not be had at this size: the staged path below needs none of it.  The series keeps a
        // buffer for its single calls (2 K + 64 doubles), or says so
        if (!s->host && series_host(s, 2 * (size_t)s->K + 64) != PGPS_OK) return PGPS_E_NOMEM;
    }
    TRY(stage_in<double>(ctx, ctx->st[7], nullptr, bk, &o.dmean));
    TRY(stage_in<double>(ctx, ctx->st[8], nullptr, bk, &o.dvar));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)B, &o.dll));
    if (w) {
        TRY(stage_in<double>(ctx, ctx->st[3], nullptr, 2 * K, &o.dmix));
        TRY(stage_in<double>(ctx, ctx->st[4], w, (size_t)B, &o.dw));
    }
    return PGPS_OK;
}
static int series_batch_end(pgps_series* s, int B, const double* w, const SeriesBatchOut& o, double* mean, double* var,
                            double* ll) {
    pgps_ctx* ctx = s->ctx;
    const size_t K = (size_t)s->K, bk = (size_t)B * K;
    if (o.zero) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(mean, s->host, bk * sizeof(double));
        std::memcpy(var, s->host + bk, bk * sizeof(double));
        return batch_ll_result(B, s->host + 2 * bk, ll);
    }
    if (w) TRY(mix_moments_dev(ctx, B, s->K, o.dmean, o.dvar, o.dw, o.dmix, o.dmix + K));
    const size_t nout = (w ? K : bk) * sizeof(double);
    return copy_out_batch(ctx, B, {mean, w ? o.dmix : o.dmean, nout}, {var, w ? o.dmix + K : o.dvar, nout}, o.dll, ll);
}

// the batch on the resident series and its merged query grid.  w == NULL: mean, var (B, K) on the host; else w = B mixture
// weights (host, used as given) and mean, var (K): the (B, K) results stay on the device, k_mix_moments reduces them there
extern "C" int pgps_series_gp_predict_batch_f64(pgps_series* s, int B, int d, const double* models, const double* w,
                                                double* mean, double* var, double* ll) {
    if (!s || B < 1 || s->K < 1 || !models || !mean || !var) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    pgps_ctx* ctx = s->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SeriesBatchOut o;
    TRY(series_batch_begin(s, B, w, o));
    TRY(gp_predict_batch_merged<double>(ctx, B, (size_t)(s->N + s->K), s->K, d, models, s->ts_m, s->ys_m, s->t0, s->qslot, o.dmean,
                                        o.dvar, o.dll));
    return series_batch_end(s, B, w, o, mean, var, ll);
}
extern "C" int pgps_series_lti_predict_batch_f64(pgps_series* s, int B, int d, const double* models, const double* w,
                                                 double* mean, double* var, double* ll) {
    if (!s || B < 1 || s->K < 1 || !models || !mean || !var) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > rc::kDimMax) return PGPS_E_UNSUPPORTED_DIM;
    pgps_ctx* ctx = s->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SeriesBatchOut o;
    TRY(series_batch_begin(s, B, w, o));
    TRY(lti_predict_batch_merged(ctx, B, (size_t)(s->N + s->K), s->K, d, models, s->ts_m, s->ys_m, s->t0, s->qslot, o.dmean, o.dvar,
                                 o.dll));
    return series_batch_end(s, B, w, o, mean, var, ll);
}
