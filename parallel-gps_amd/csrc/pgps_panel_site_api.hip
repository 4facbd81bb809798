// pgps_panel_site_api.hip -- the Laplace entry points of a panel (include/pgps.h: pgps_gp_panel_laplace_*,
// pgps_gp_panel_laplace_grad_*): argument checks, staging of the host forms through the context's
// buffers, dispatch to launch_gp_panel_laplace<d> / launch_gp_panel_laplace_grad<d> (pgps_panel_site_inst.hip).
#include "pgps_host.h"
#include "pgps_lik.h"
#include "pgps_newton.h"
#include "pgps_panel_site.h"
#include "pgps_panel_site_lay.h"

using namespace pgps;

// everything a call can be refused for before anything is staged
static int site_check(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models, int lik, int npars,
                      const double* pars, const double* ts, const double* ys) {
    if (!ctx || S < 1 || !offs || !models || !pars || !ts || !ys) return PGPS_E_INVALID;
    if (nmodels != 1 && (long)nmodels != S) return PGPS_E_INVALID;
    if (npars != 1 && (long)npars != S) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    if (offs[0] != 0) return PGPS_E_INVALID;
    for (long s = 0; s < S; ++s) {
        const long n = offs[s + 1] - offs[s];
        if (n < 1 || n > PGPS_PANEL_MAX_STEPS) return PGPS_E_INVALID;
    }
    const int in_stride = 1 + 3 * d * d + d + 1;
    for (int b = 0; b < nmodels; ++b)
        if (!(models[(size_t)b * in_stride] > 0.0)) return PGPS_E_INVALID;          // lam (R, the last column, is ignored)
    if (!lik_known(lik)) return PGPS_E_INVALID;
    if (lik != PGPS_LIK_BERNOULLI_LOGIT)
        for (int i = 0; i < npars; ++i)
            if (!(pars[i] > 0.0) || !std::isfinite(pars[i])) return PGPS_E_INVALID;
    return PGPS_OK;
}

// the caller's rows [lam | N1 | N2 | Pinf | H | R] at the fixed device stride, R = 0: the sites carry all the noise
static void site_pack_models(int nmodels, int d, const double* models, std::vector<double>& packed) {
    packed.assign((size_t)nmodels * kGpModelStride, 0.0);
    const int dd = d * d, in_stride = 1 + 3 * dd + d + 1;
    for (int m = 0; m < nmodels; ++m) {
        const double* p = models + (size_t)m * in_stride;
        double* q = packed.data() + (size_t)m * kGpModelStride;
        q[0] = p[0];
        for (int i = 0; i < dd; ++i) { q[1 + i] = p[1 + i]; q[10 + i] = p[1 + dd + i]; q[19 + i] = p[1 + 2 * dd + i]; }
        for (int i = 0; i < d; ++i) q[28 + i] = p[1 + 3 * dd + i];
    }
}

static PanelSiteCall site_call(long S, const long* offs, int nmodels, const std::vector<double>& packed, int lik, int npars,
                               const double* pars, const double* ts, const double* ys) {
    PanelSiteCall c{};
    c.S = S; c.offs = offs; c.nmodels = nmodels; c.models = packed.data(); c.lik = lik; c.npars = npars; c.pars = pars;
    c.ts = ts; c.ys = ys;
    return c;
}

static int site_fit_dev(pgps_ctx* ctx, int d, const PanelSiteCall& c) {
    RoctxRange range_("laplace_panel_search");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_panel_laplace<D()>(ctx, c); });
}
static int site_grad_dev(pgps_ctx* ctx, int d, const PanelSiteCall& c) {
    RoctxRange range_("laplace_panel_grad");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_panel_laplace_grad<D()>(ctx, c); });
}

extern "C" int pgps_gp_panel_laplace_dev_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models,
                                             int lik, int npars, const double* pars, const double* ts, const double* ys,
                                             double tol, int max_iter, double* f, double* v, double* zs, double* ss,
                                             double* info) {
    TRY(site_check(ctx, S, offs, d, nmodels, models, lik, npars, pars, ts, ys));
    if (!f || !v || !zs || !ss || !info) return PGPS_E_INVALID;
    if (!newton_tol_valid(tol) || !newton_max_iter_valid(max_iter)) return PGPS_E_INVALID;
    std::vector<double> packed;
    site_pack_models(nmodels, d, models, packed);
    PanelSiteCall c = site_call(S, offs, nmodels, packed, lik, npars, pars, ts, ys);
    c.tol = tol; c.max_iter = max_iter;
    c.f = f; c.v = v; c.zs = zs; c.ss = ss; c.info = info;
    return site_fit_dev(ctx, d, c);
}

extern "C" int pgps_gp_panel_laplace_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models, int lik,
                                         int npars, const double* pars, const double* ts, const double* ys, double tol,
                                         int max_iter, double* f, double* v, double* zs, double* ss, double* info) {
    TRY(site_check(ctx, S, offs, d, nmodels, models, lik, npars, pars, ts, ys));
    if (!f || !v || !zs || !ss || !info) return PGPS_E_INVALID;
    if (!newton_tol_valid(tol) || !newton_max_iter_valid(max_iter)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)offs[S];
    std::vector<double> packed;
    site_pack_models(nmodels, d, models, packed);
    double *dts, *dys, *drows, *dinfo;
    TRY(stage_in(ctx, ctx->st[10], ts, N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, N, &dys));
    TRY(stage_in<double>(ctx, ctx->st[7], nullptr, 4 * N, &drows));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)S * kSiteInfo, &dinfo));
    PanelSiteCall c = site_call(S, offs, nmodels, packed, lik, npars, pars, dts, dys);
    c.tol = tol; c.max_iter = max_iter;
    c.f = drows; c.v = drows + N; c.zs = drows + 2 * N; c.ss = drows + 3 * N; c.info = dinfo;
    TRY(site_fit_dev(ctx, d, c));
    std::vector<double> rows(4 * N), infoh((size_t)S * kSiteInfo);
    TRY(stage_out(ctx, rows.data(), (const double*)drows, 4 * N));
    TRY(stage_out(ctx, infoh.data(), (const double*)dinfo, infoh.size()));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(f, rows.data(), N * sizeof(double));
    memcpy(v, rows.data() + N, N * sizeof(double));
    memcpy(zs, rows.data() + 2 * N, N * sizeof(double));
    memcpy(ss, rows.data() + 3 * N, N * sizeof(double));
    memcpy(info, infoh.data(), infoh.size() * sizeof(double));
    for (double x : infoh)
        if (!std::isfinite(x)) return PGPS_E_NUMERIC;
    return PGPS_OK;
}

extern "C" int pgps_gp_panel_laplace_grad_dev_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models,
                                                  int lik, int npars, const double* pars, const double* ts, const double* ys,
                                                  const double* f, const double* v, const double* zs, const double* ss,
                                                  double* out) {
    TRY(site_check(ctx, S, offs, d, nmodels, models, lik, npars, pars, ts, ys));
    if (!f || !v || !zs || !ss || !out) return PGPS_E_INVALID;
    std::vector<double> packed;
    site_pack_models(nmodels, d, models, packed);
    PanelSiteCall c = site_call(S, offs, nmodels, packed, lik, npars, pars, ts, ys);
    c.f = const_cast<double*>(f); c.v = const_cast<double*>(v); c.zs = const_cast<double*>(zs); c.ss = const_cast<double*>(ss);
    c.out = out;
    return site_grad_dev(ctx, d, c);
}

extern "C" int pgps_gp_panel_laplace_grad_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models,
                                              int lik, int npars, const double* pars, const double* ts, const double* ys,
                                              const double* f, const double* v, const double* zs, const double* ss, double* out) {
    TRY(site_check(ctx, S, offs, d, nmodels, models, lik, npars, pars, ts, ys));
    if (!f || !v || !zs || !ss || !out) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)offs[S], nout = (size_t)S * (1 + d * d + 2 * d + 1);
    std::vector<double> packed;
    site_pack_models(nmodels, d, models, packed);
    double *dts, *dys, *drows, *dout;
    TRY(stage_in(ctx, ctx->st[10], ts, N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, N, &dys));
    TRY(stage_in<double>(ctx, ctx->st[7], nullptr, 4 * N, &drows));
    const double* in_h[4] = {f, v, zs, ss};
    for (int i = 0; i < 4; ++i)
        HIPCHK(ctx, hipMemcpyAsync(drows + (size_t)i * N, in_h[i], N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, nout, &dout));
    PanelSiteCall c = site_call(S, offs, nmodels, packed, lik, npars, pars, dts, dys);
    c.f = drows; c.v = drows + N; c.zs = drows + 2 * N; c.ss = drows + 3 * N; c.out = dout;
    TRY(site_grad_dev(ctx, d, c));
    std::vector<double> outh(nout);
    TRY(stage_out(ctx, outh.data(), (const double*)dout, nout));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out, outh.data(), nout * sizeof(double));
    const size_t stride = nout / (size_t)S;
    for (long s = 0; s < S; ++s)
        if (!std::isfinite(outh[(size_t)s * stride])) return PGPS_E_NUMERIC;
    return PGPS_OK;
}
