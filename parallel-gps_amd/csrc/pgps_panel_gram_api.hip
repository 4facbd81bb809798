// pgps_panel_gram_api.hip -- the panel's mean-function entry points of the C ABI (include/pgps.h: pgps_gp_panel_gram_*,
// pgps_gp_panel_residual_dev_f64): the whitened Gram matrix of C = 1 + p columns of every series, and
// the residual series at given trend coefficients.  Argument checks (those of pgps_gp_panel_ll_* and C in 1 .. kPanelGramMax),
// the host form's passes over V (all-or-none rows) and rs, staging through the context's buffers, dispatch to
// launch_gp_panel_gram<d> (pgps_panel_gram_inst.hip).
#include "pgps_host.h"

using namespace pgps;

int pgps::panel_gram_check(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models, int C, const double* ts,
                           const double* V, bool het, const double* out) {
    TRY(panel_check(ctx, S, offs, nullptr, false, d, nmodels, models, ts, V, het));
    if (C < 1 || C > kPanelGramMax || !out) return PGPS_E_INVALID;
    return PGPS_OK;
}

// the host form's one pass over V and rs: a row is observed in all columns or in none (the rule of pgps_gp_*_multi_f64), and
// at the observed rows rs is finite, >= 0 and R + rs[k] > 0 (the rule of pgps_gp_panel_ll_f64)
bool pgps::panel_gram_rows_valid(long S, const long* offs, int d, int nmodels, const double* models, int C, const double* V,
                                 const double* rs) {
    const int in_stride = 1 + 3 * d * d + d + 1;
    for (long s = 0; s < S; ++s) {
        const double R = models[(size_t)(nmodels == 1 ? 0 : s) * in_stride + in_stride - 1];
        for (long k = offs[s]; k < offs[s + 1]; ++k) {
            const double* r = V + (size_t)k * C;
            int nan = 0;
            for (int j = 0; j < C; ++j) nan += std::isnan(r[j]) ? 1 : 0;
            if (nan != 0 && nan != C) return false;
            if (nan || !rs) continue;
            const double v = rs[k];
            if (!std::isfinite(v) || v < 0.0 || !(R + v > 0.0)) return false;
        }
    }
    return true;
}

static int gram_dev(pgps_ctx* ctx, int d, const PanelGramCall& c) {
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_panel_gram<D()>(ctx, c); });
}

extern "C" int pgps_gp_panel_gram_dev_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models, int C,
                                          const double* ts, const double* V, const double* rs, double* out) {
    TRY(panel_gram_check(ctx, S, offs, d, nmodels, models, C, ts, V, rs != nullptr, out));
    std::vector<double> packed;
    panel_pack_models(nmodels, d, models, packed);
    PanelGramCall c{};
    c.S = S; c.offs = offs; c.nmodels = nmodels; c.models = packed.data(); c.C = C; c.ts = ts; c.V = V; c.rs = rs; c.out = out;
    return gram_dev(ctx, d, c);
}

extern "C" int pgps_gp_panel_gram_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models, int C,
                                      const double* ts, const double* V, const double* rs, double* out) {
    TRY(panel_gram_check(ctx, S, offs, d, nmodels, models, C, ts, V, rs != nullptr, out));
    if (!panel_gram_rows_valid(S, offs, d, nmodels, models, C, V, rs)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)offs[S], rec = (size_t)C * C + 2;
    std::vector<double> packed;
    panel_pack_models(nmodels, d, models, packed);
    PanelGramCall c{};
    c.S = S; c.offs = offs; c.nmodels = nmodels; c.models = packed.data(); c.C = C;
    // [V (N, C) | rs (N)] share ONE staging buffer
    double *dts, *dV;
    TRY(stage_in(ctx, ctx->st[10], ts, N, &dts));
    TRY(stage_in<double>(ctx, ctx->st[4], nullptr, N * C + (rs ? N : 0), &dV));
    HIPCHK(ctx, hipMemcpyAsync(dV, V, N * C * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (rs) HIPCHK(ctx, hipMemcpyAsync(dV + N * C, rs, N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    c.ts = dts; c.V = dV; c.rs = rs ? dV + N * C : nullptr;
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)S * rec, &c.out));
    TRY(gram_dev(ctx, d, c));
    // the records come back through a vector of the call: an error leaves the caller's output untouched
    std::vector<double> outh((size_t)S * rec);
    TRY(stage_out(ctx, outh.data(), c.out, (size_t)S * rec));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out, outh.data(), outh.size() * sizeof(double));
    for (long s = 0; s < S; ++s)
        if (!std::isfinite(outh[(size_t)s * rec + rec - 2])) return PGPS_E_NUMERIC;         // (logdet)
    return PGPS_OK;
}

extern "C" int pgps_gp_panel_residual_dev_f64(pgps_ctx* ctx, long S, const long* offs, int C, const double* V, const double* betas,
                                              double* ys_out) {
    if (!ctx || S < 1 || !offs || !V || !ys_out) return PGPS_E_INVALID;
    if (C < 1 || C > kPanelGramMax || (C > 1 && !betas)) return PGPS_E_INVALID;
    if (offs[0] != 0) return PGPS_E_INVALID;
    for (long s = 0; s < S; ++s) {
        const long n = offs[s + 1] - offs[s];
        if (n < 1 || n > PGPS_PANEL_MAX_STEPS) return PGPS_E_INVALID;
    }
    return launch_panel_residual(ctx, S, offs, C, V, betas, ys_out);
}
