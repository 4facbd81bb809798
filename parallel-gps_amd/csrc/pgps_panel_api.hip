// pgps_panel_api.hip -- the panel entry points of the C ABI (include/pgps.h: pgps_gp_panel_ll_*, pgps_gp_panel_ll_grad_*,
// pgps_gp_panel_predict_*, pgps_gp_panel_loo_*; DESIGN.md sections 4aa, 4ac): S independent series cut out of concatenated arrays by `offs`, each on its
// own clock.  Argument checks, the one scan of `rs` the host forms make, staging through the context's buffers (rs travels
// behind ys in the same buffer), dispatch to launch_gp_panel<d> (pgps_panel_inst.hip).
#include "pgps_host.h"

using namespace pgps;

// everything a call can be refused for before anything is staged
int pgps::panel_check(pgps_ctx* ctx, long S, const long* offs, const long* qoffs, bool predict, int d, int nmodels,
                       const double* models, const double* ts, const double* ys, bool het) {
    if (!ctx || S < 1 || !offs || !models || !ts || !ys) return PGPS_E_INVALID;
    if (predict && !qoffs) return PGPS_E_INVALID;
    if (nmodels != 1 && (long)nmodels != S) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    if (offs[0] != 0 || (predict && qoffs[0] != 0)) return PGPS_E_INVALID;
    for (long s = 0; s < S; ++s) {
        const long n = offs[s + 1] - offs[s], k = predict ? qoffs[s + 1] - qoffs[s] : 0;
        if (n < 1 || k < 0 || n > PGPS_PANEL_MAX_STEPS || n + k > PGPS_PANEL_MAX_STEPS) return PGPS_E_INVALID;
    }
    if (predict && (qoffs[S] < 1 || qoffs[S] > 0x7fffffffL)) return PGPS_E_INVALID;     // (qslot holds global positions as ints)
    const int in_stride = 1 + 3 * d * d + d + 1;
    for (int b = 0; b < nmodels; ++b) {
        const double lam = models[(size_t)b * in_stride], R = models[(size_t)b * in_stride + in_stride - 1];
        if (!(lam > 0.0) || !std::isfinite(R) || !(R >= 0.0)) return PGPS_E_INVALID;
        if (!het && !(R > 0.0)) return PGPS_E_INVALID;
    }
    return PGPS_OK;
}

// the caller's rows [lam | N1 (d d) | N2 (d d) | Pinf (d d) | H (d) | R] re-packed to the fixed device stride (kGpModelStride), as
// gp_pack_models of pgps_gp_api.hip does for the batched calls (panel_check has validated them)
void pgps::panel_pack_models(int nmodels, int d, const double* models, std::vector<double>& packed) {
    packed.assign((size_t)nmodels * kGpModelStride, 0.0);
    const int dd = d * d, in_stride = 1 + 3 * dd + d + 1;
    for (int m = 0; m < nmodels; ++m) {
        const double* p = models + (size_t)m * in_stride;
        double* q = packed.data() + (size_t)m * kGpModelStride;
        q[0] = p[0];
        for (int i = 0; i < dd; ++i) { q[1 + i] = p[1 + i]; q[10 + i] = p[1 + dd + i]; q[19 + i] = p[1 + 2 * dd + i]; }
        for (int i = 0; i < d; ++i) q[28 + i] = p[1 + 3 * dd + i];
        q[31] = p[in_stride - 1];
    }
}

// the host forms' one pass over rs, series by series with the R of its row (the rule of pgps_gp_ll_het_f64: finite, >= 0 and
// R + rs[k] > 0 at the observed rows; rows where ys is NaN are not looked at)
static bool panel_noise_valid(long S, const long* offs, int d, int nmodels, const double* models, const double* ys,
                              const double* rs) {
    const int in_stride = 1 + 3 * d * d + d + 1;
    for (long s = 0; s < S; ++s) {
        const double R = models[(size_t)(nmodels == 1 ? 0 : s) * in_stride + in_stride - 1];
        for (long k = offs[s]; k < offs[s + 1]; ++k) {
            if (std::isnan(ys[k])) continue;
            const double v = rs[k];
            if (!std::isfinite(v) || v < 0.0 || !(R + v > 0.0)) return false;
        }
    }
    return true;
}

static int panel_dev(pgps_ctx* ctx, int d, const PanelCall& c, PanelWhat what) {
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_panel<D()>(ctx, c, what); });
}

// ts, ys and rs of a host call on the device: [ys (N) | rs (N)] share ONE staging buffer
static int panel_stage_series(pgps_ctx* ctx, long N, const double* ts, const double* ys, const double* rs, PanelCall* c) {
    double *dts, *dys;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in<double>(ctx, ctx->st[4], nullptr, (rs ? 2 : 1) * (size_t)N, &dys));
    HIPCHK(ctx, hipMemcpyAsync(dys, ys, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (rs) HIPCHK(ctx, hipMemcpyAsync(dys + N, rs, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    c->ts = dts; c->ys = dys; c->rs = rs ? dys + N : nullptr;
    return PGPS_OK;
}

// PGPS_E_NUMERIC unless the first entry of every row is finite
static int panel_rows_finite(long S, int stride, const double* rows) {
    for (long s = 0; s < S; ++s)
        if (!std::isfinite(rows[(size_t)s * stride])) return PGPS_E_NUMERIC;
    return PGPS_OK;
}

extern "C" int pgps_gp_panel_ll_dev_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models,
                                        const double* ts, const double* ys, const double* rs, double* ll) {
    TRY(panel_check(ctx, S, offs, nullptr, false, d, nmodels, models, ts, ys, rs != nullptr));
    if (!ll) return PGPS_E_INVALID;
    std::vector<double> packed;
    panel_pack_models(nmodels, d, models, packed);
    PanelCall c{};
    c.S = S; c.offs = offs; c.nmodels = nmodels; c.models = packed.data(); c.ts = ts; c.ys = ys; c.rs = rs; c.ll = ll;
    return panel_dev(ctx, d, c, PANEL_LL);
}

extern "C" int pgps_gp_panel_ll_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models,
                                    const double* ts, const double* ys, const double* rs, double* ll) {
    TRY(panel_check(ctx, S, offs, nullptr, false, d, nmodels, models, ts, ys, rs != nullptr));
    if (!ll) return PGPS_E_INVALID;
    if (rs && !panel_noise_valid(S, offs, d, nmodels, models, ys, rs)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<double> packed;
    panel_pack_models(nmodels, d, models, packed);
    PanelCall c{};
    c.S = S; c.offs = offs; c.nmodels = nmodels; c.models = packed.data();
    TRY(panel_stage_series(ctx, offs[S], ts, ys, rs, &c));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)S, &c.ll));
    TRY(panel_dev(ctx, d, c, PANEL_LL));
    TRY(stage_out(ctx, ll, c.ll, (size_t)S));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return panel_rows_finite(S, 1, ll);
}

extern "C" int pgps_gp_panel_ll_grad_dev_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models,
                                             const double* ts, const double* ys, const double* rs, double* out) {
    TRY(panel_check(ctx, S, offs, nullptr, false, d, nmodels, models, ts, ys, rs != nullptr));
    if (!out) return PGPS_E_INVALID;
    std::vector<double> packed;
    panel_pack_models(nmodels, d, models, packed);
    PanelCall c{};
    c.S = S; c.offs = offs; c.nmodels = nmodels; c.models = packed.data(); c.ts = ts; c.ys = ys; c.rs = rs; c.out = out;
    return panel_dev(ctx, d, c, PANEL_GRAD);
}

extern "C" int pgps_gp_panel_ll_grad_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models,
                                         const double* ts, const double* ys, const double* rs, double* out) {
    TRY(panel_check(ctx, S, offs, nullptr, false, d, nmodels, models, ts, ys, rs != nullptr));
    if (!out) return PGPS_E_INVALID;
    if (rs && !panel_noise_valid(S, offs, d, nmodels, models, ys, rs)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int nout = 1 + d * d + 2 * d + 1;
    std::vector<double> packed;
    panel_pack_models(nmodels, d, models, packed);
    PanelCall c{};
    c.S = S; c.offs = offs; c.nmodels = nmodels; c.models = packed.data();
    TRY(panel_stage_series(ctx, offs[S], ts, ys, rs, &c));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)S * nout, &c.out));
    TRY(panel_dev(ctx, d, c, PANEL_GRAD));
    TRY(stage_out(ctx, out, c.out, (size_t)S * nout));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return panel_rows_finite(S, nout, out);
}

// ll may be null: the log-likelihoods then go to a buffer of the context
static int panel_predict_dev(pgps_ctx* ctx, int d, PanelCall c) {
    if (!c.ll) TRY(stage_in<double>(ctx, ctx->st[11], nullptr, (size_t)c.S, &c.ll));
    return panel_dev(ctx, d, c, PANEL_PREDICT);
}

extern "C" int pgps_gp_panel_predict_dev_f64(pgps_ctx* ctx, long S, const long* offs, const long* qoffs, int d, int nmodels,
                                             const double* models, const double* ts, const double* ys, const double* rs,
                                             const double* tq, double* mean, double* var, double* ll) {
    TRY(panel_check(ctx, S, offs, qoffs, true, d, nmodels, models, ts, ys, rs != nullptr));
    if (!tq || !mean || !var) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<double> packed;
    panel_pack_models(nmodels, d, models, packed);
    PanelCall c{};
    c.S = S; c.offs = offs; c.qoffs = qoffs; c.nmodels = nmodels; c.models = packed.data();
    c.ts = ts; c.ys = ys; c.rs = rs; c.tq = tq; c.mean = mean; c.var = var; c.ll = ll;
    return panel_predict_dev(ctx, d, c);
}

extern "C" int pgps_gp_panel_predict_f64(pgps_ctx* ctx, long S, const long* offs, const long* qoffs, int d, int nmodels,
                                         const double* models, const double* ts, const double* ys, const double* rs,
                                         const double* tq, double* mean, double* var, double* ll) {
    TRY(panel_check(ctx, S, offs, qoffs, true, d, nmodels, models, ts, ys, rs != nullptr));
    if (!tq || !mean || !var) return PGPS_E_INVALID;
    if (rs && !panel_noise_valid(S, offs, d, nmodels, models, ys, rs)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t K = (size_t)qoffs[S];
    std::vector<double> packed;
    panel_pack_models(nmodels, d, models, packed);
    PanelCall c{};
    c.S = S; c.offs = offs; c.qoffs = qoffs; c.nmodels = nmodels; c.models = packed.data();
    TRY(panel_stage_series(ctx, offs[S], ts, ys, rs, &c));
    double* dtq;
    TRY(stage_in(ctx, ctx->st[3], tq, K, &dtq));
    c.tq = dtq;
    TRY(stage_in<double>(ctx, ctx->st[7], nullptr, K, &c.mean));
    TRY(stage_in<double>(ctx, ctx->st[8], nullptr, K, &c.var));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)S, &c.ll));
    TRY(panel_predict_dev(ctx, d, c));
    std::vector<double> llh((size_t)S);
    TRY(stage_out(ctx, mean, c.mean, K));
    TRY(stage_out(ctx, var, c.var, K));
    TRY(stage_out(ctx, llh.data(), c.ll, (size_t)S));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ll) memcpy(ll, llh.data(), (size_t)S * sizeof(double));
    return panel_rows_finite(S, 1, llh.data());
}

// ---- predictive checks of every series ----------------------------------------------------------------
extern "C" int pgps_gp_panel_loo_dev_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models,
                                         const double* ts, const double* ys, const double* rs, double* osa_mean, double* osa_var,
                                         double* loo_mean, double* loo_var, double* sums) {
    TRY(panel_check(ctx, S, offs, nullptr, false, d, nmodels, models, ts, ys, rs != nullptr));
    if (!sums) return PGPS_E_INVALID;
    std::vector<double> packed;
    panel_pack_models(nmodels, d, models, packed);
    PanelCall c{};
    c.S = S; c.offs = offs; c.nmodels = nmodels; c.models = packed.data(); c.ts = ts; c.ys = ys; c.rs = rs;
    c.osa_mean = osa_mean; c.osa_var = osa_var; c.loo_mean = loo_mean; c.loo_var = loo_var; c.sums = sums;
    return panel_dev(ctx, d, c, PANEL_LOO);
}

extern "C" int pgps_gp_panel_loo_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models,
                                     const double* ts, const double* ys, const double* rs, double* osa_mean, double* osa_var,
                                     double* loo_mean, double* loo_var, double* sums) {
    TRY(panel_check(ctx, S, offs, nullptr, false, d, nmodels, models, ts, ys, rs != nullptr));
    if (!sums) return PGPS_E_INVALID;
    if (rs && !panel_noise_valid(S, offs, d, nmodels, models, ys, rs)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)offs[S];
    std::vector<double> packed;
    panel_pack_models(nmodels, d, models, packed);
    PanelCall c{};
    c.S = S; c.offs = offs; c.nmodels = nmodels; c.models = packed.data();
    TRY(panel_stage_series(ctx, offs[S], ts, ys, rs, &c));
    // the arrays asked for leave through ONE staging buffer (none: the sums alone come back)
    double* host[4] = {osa_mean, osa_var, loo_mean, loo_var};
    double* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t wanted = 0;
    for (double* h : host) wanted += h ? 1 : 0;
    double* dout = nullptr;
    if (wanted) TRY(stage_in<double>(ctx, ctx->st[7], nullptr, wanted * N, &dout));
    for (size_t i = 0, j = 0; i < 4; ++i)
        if (host[i]) dev[i] = dout + (j++) * N;
    c.osa_mean = dev[0]; c.osa_var = dev[1]; c.loo_mean = dev[2]; c.loo_var = dev[3];
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 2 * (size_t)S, &c.sums));
    TRY(panel_dev(ctx, d, c, PANEL_LOO));
    for (int i = 0; i < 4; ++i) TRY(stage_out(ctx, host[i], dev[i], N));
    TRY(stage_out(ctx, sums, c.sums, 2 * (size_t)S));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (long s = 0; s < 2 * S; ++s)
        if (!std::isfinite(sums[s])) return PGPS_E_NUMERIC;
    return PGPS_OK;
}
