// pgps_check_api.hip -- the predictive-check entry points of the C ABI (include/pgps.h: pgps_gp_loo_f64, pgps_gp_loo_dev_f64;
// DESIGN.md section 4w): argument checks, staging through the context's buffers (the four per-step arrays leave through ONE
// staging buffer; with all four null the call brings back the two sums alone), dispatch to launch_gp_loo<d> (pgps_loo_inst.hip).
#include "pgps_host.h"

using namespace pgps;

static int loo_args(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* Pinf, const double* H, double R,
                    const double* ts, const double* ys, const double* sums) {
    if (!ctx || N < 1 || !N1 || !Pinf || !H || !ts || !ys || !sums) return PGPS_E_INVALID;
    if (!(R > 0.0) || !std::isfinite(R) || !(lam > 0.0)) return PGPS_E_INVALID;     // (leaving out a noise-free observation is undefined)
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    return PGPS_OK;
}

static int gp_loo_dev(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                      const double* H, double R, const double* ts, const double* ys, double t0, GpLooOut<double> o,
                      double* sums) {
    TRY(loo_args(ctx, N, d, lam, N1, Pinf, H, R, ts, ys, sums));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    GpArgs<double> g{};
    g.s.N = N;
    g.s.R = R;
    g.s.ys = ys;
    g.m.lam = lam;
    for (int i = 0; i < d * d; ++i) { g.m.N1[i] = N1[i]; g.m.N2[i] = N2 ? N2[i] : 0.0; g.m.Pinf[i] = Pinf[i]; }
    for (int i = 0; i < d; ++i) g.m.H[i] = H[i];
    g.m.ts = ts;
    g.m.t_prev = t0;
    // the filtered moments the smoother reads back
    TRY(stage_in<double>(ctx, ctx->st[5], nullptr, (size_t)N * d, &g.s.fms));
    TRY(stage_in<double>(ctx, ctx->st[6], nullptr, (size_t)N * d * d, &g.s.fPs));
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_loo<D()>(ctx, g, o, sums); });
}

extern "C" int pgps_gp_loo_dev_f64(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2,
                                   const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                                   double* osa_mean, double* osa_var, double* loo_mean, double* loo_var, double* sums) {
    return gp_loo_dev(ctx, N, d, lam, N1, N2, Pinf, H, R, ts, ys, t0, GpLooOut<double>{osa_mean, osa_var, loo_mean, loo_var, nullptr},
                      sums);
}

extern "C" int pgps_gp_loo_f64(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                               const double* H, double R, const double* ts, const double* ys, double t0, double* osa_mean,
                               double* osa_var, double* loo_mean, double* loo_var, double* sums) {
    TRY(loo_args(ctx, N, d, lam, N1, Pinf, H, R, ts, ys, sums));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double* host[4] = {osa_mean, osa_var, loo_mean, loo_var};
    double* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t wanted = 0;
    for (double* h : host) wanted += h ? 1 : 0;
    double *dts, *dys, *dout = nullptr, *dsums;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    if (wanted) TRY(stage_in<double>(ctx, ctx->st[7], nullptr, wanted * (size_t)N, &dout));
    for (size_t i = 0, j = 0; i < 4; ++i)
        if (host[i]) dev[i] = dout + (j++) * (size_t)N;
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 2, &dsums));
    TRY(gp_loo_dev(ctx, N, d, lam, N1, N2, Pinf, H, R, dts, dys, t0, GpLooOut<double>{dev[0], dev[1], dev[2], dev[3], nullptr}, dsums));
    for (int i = 0; i < 4; ++i) TRY(stage_out(ctx, host[i], dev[i], (size_t)N));
    double h2[2] = {0.0, 0.0};
    TRY(stage_out(ctx, h2, dsums, 2));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    sums[0] = h2[0];
    sums[1] = h2[1];
    return std::isfinite(h2[0]) && std::isfinite(h2[1]) ? PGPS_OK : PGPS_E_NUMERIC;
}
