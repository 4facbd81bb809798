// pgps_site_api.hip -- the Laplace-inference entry points of the C ABI (include/pgps.h: pgps_gp_newton_*, pgps_lik_sites_*;
// DESIGN.md section 4y): argument checks, the one scan of the site variances the host forms make, staging through the context's
// buffers (the host forms exist for the ABI tests: every array travels), dispatch to launch_gp_newton<d> / launch_lik_sites
// (pgps_site_inst.hip).
#include "pgps_host.h"
#include "pgps_lik.h"

using namespace pgps;

static int lik_args(int lik, double par) {
    if (!lik_known(lik)) return PGPS_E_INVALID;
    if (lik != PGPS_LIK_BERNOULLI_LOGIT && (!(par > 0.0) || !std::isfinite(par))) return PGPS_E_INVALID;
    return PGPS_OK;
}

static int newton_args(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* Pinf, const double* H, int lik,
                       double par, const double* ts, const double* ys, const double* zs, const double* ss, const double* f_out,
                       const double* v_out, const double* alpha_out, const double* zs_out, const double* ss_out,
                       const double* sums) {
    if (!ctx || N < 1 || !N1 || !Pinf || !H || !ts || !ys || !zs || !ss) return PGPS_E_INVALID;
    if (!f_out || !v_out || !alpha_out || !zs_out || !ss_out || !sums) return PGPS_E_INVALID;
    if (!(lam > 0.0)) return PGPS_E_INVALID;
    TRY(lik_args(lik, par));
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    return PGPS_OK;
}

static int gp_newton_dev(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                         const double* H, int lik, double par, const double* ts, const double* ys, const double* zs,
                         const double* ss, const double* f_prev, double t0, double* f_out, double* v_out, double* alpha_out,
                         double* zs_out, double* ss_out, double* sums) {
    TRY(newton_args(ctx, N, d, lam, N1, Pinf, H, lik, par, ts, ys, zs, ss, f_out, v_out, alpha_out, zs_out, ss_out, sums));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    GpArgs<double> g{};
    g.s.N = N;
    g.s.R = 0.0;                // (the sites carry all the noise)
    g.s.ys = zs;
    g.m.lam = lam;
    for (int i = 0; i < d * d; ++i) { g.m.N1[i] = N1[i]; g.m.N2[i] = N2 ? N2[i] : 0.0; g.m.Pinf[i] = Pinf[i]; }
    for (int i = 0; i < d; ++i) g.m.H[i] = H[i];
    g.m.ts = ts;
    g.m.t_prev = t0;
    // the filtered moments the smoother reads back
    TRY(stage_in<double>(ctx, ctx->st[5], nullptr, (size_t)N * d, &g.s.fms));
    TRY(stage_in<double>(ctx, ctx->st[6], nullptr, (size_t)N * d * d, &g.s.fPs));
    const GpSiteOut<double> o{lik, par, ys, ss, f_prev, f_out, v_out, alpha_out, zs_out, ss_out, nullptr};
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_newton<D()>(ctx, g, o, sums); });
}

static int lik_sites_args(pgps_ctx* ctx, long N, int lik, double par, const double* ys, const double* f_a, const double* alpha_a,
                          const double* f_b, const double* alpha_b, double step, const double* f_out, const double* alpha_out,
                          const double* zs_out, const double* ss_out, const double* sums) {
    if (!ctx || N < 1 || !ys || !f_a || !alpha_a || !f_out || !alpha_out || !zs_out || !ss_out || !sums) return PGPS_E_INVALID;
    if ((f_b == nullptr) != (alpha_b == nullptr) || !std::isfinite(step)) return PGPS_E_INVALID;
    return lik_args(lik, par);
}

static int lik_sites_dev(pgps_ctx* ctx, long N, int lik, double par, const double* ys, const double* f_a, const double* alpha_a,
                         const double* f_b, const double* alpha_b, double step, double* f_out, double* alpha_out, double* zs_out,
                         double* ss_out, double* sums) {
    TRY(lik_sites_args(ctx, N, lik, par, ys, f_a, alpha_a, f_b, alpha_b, step, f_out, alpha_out, zs_out, ss_out, sums));
    LikSitesArgs a{};
    a.N = N;
    a.lik = lik;
    a.par = par;
    a.ys = ys; a.f_a = f_a; a.alpha_a = alpha_a; a.f_b = f_b; a.alpha_b = alpha_b;
    a.step = step;
    a.f_out = f_out; a.alpha_out = alpha_out; a.zs_out = zs_out; a.ss_out = ss_out;
    return launch_lik_sites(ctx, a, sums);
}

extern "C" int pgps_gp_newton_dev_f64(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2,
                                      const double* Pinf, const double* H, int lik, double par, const double* ts,
                                      const double* ys, const double* zs, const double* ss, const double* f_prev, double t0,
                                      double* f_out, double* v_out, double* alpha_out, double* zs_out, double* ss_out,
                                      double* sums) {
    return gp_newton_dev(ctx, N, d, lam, N1, N2, Pinf, H, lik, par, ts, ys, zs, ss, f_prev, t0, f_out, v_out, alpha_out, zs_out,
                         ss_out, sums);
}

// the host forms' one pass over the sites: zs is NaN exactly where ys is, and ss is finite and > 0 at every observed row
static bool sites_valid(long N, const double* ys, const double* zs, const double* ss) {
    for (long k = 0; k < N; ++k) {
        if (std::isnan(ys[k]) != std::isnan(zs[k])) return false;
        if (std::isnan(ys[k])) continue;
        if (!std::isfinite(ss[k]) || !(ss[k] > 0.0)) return false;
    }
    return true;
}

// `count` arrays of N doubles behind each other in ONE staging buffer; the non-null host arrays are copied in
static int stage_rows(pgps_ctx* ctx, DevBuf& b, long N, int count, const double* const* host, double** dev) {
    double* base;
    TRY(stage_in<double>(ctx, b, nullptr, (size_t)count * (size_t)N, &base));
    for (int i = 0; i < count; ++i) {
        dev[i] = base + (size_t)i * (size_t)N;
        if (host && host[i])
            HIPCHK(ctx, hipMemcpyAsync(dev[i], host[i], (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    return PGPS_OK;
}

static bool all_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

extern "C" int pgps_gp_newton_f64(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                                  const double* H, int lik, double par, const double* ts, const double* ys, const double* zs,
                                  const double* ss, const double* f_prev, double t0, double* f_out, double* v_out,
                                  double* alpha_out, double* zs_out, double* ss_out, double* sums) {
    TRY(newton_args(ctx, N, d, lam, N1, Pinf, H, lik, par, ts, ys, zs, ss, f_out, v_out, alpha_out, zs_out, ss_out, sums));
    if (!sites_valid(N, ys, zs, ss)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double* in_h[5] = {ts, ys, zs, ss, f_prev};
    double *in_d[5], *out_d[5], *dsums;
    TRY(stage_rows(ctx, ctx->st[4], N, 5, in_h, in_d));
    TRY(stage_rows(ctx, ctx->st[7], N, 5, nullptr, out_d));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 6, &dsums));
    TRY(gp_newton_dev(ctx, N, d, lam, N1, N2, Pinf, H, lik, par, in_d[0], in_d[1], in_d[2], in_d[3], f_prev ? in_d[4] : nullptr,
                      t0, out_d[0], out_d[1], out_d[2], out_d[3], out_d[4], dsums));
    double* out_h[5] = {f_out, v_out, alpha_out, zs_out, ss_out};
    for (int i = 0; i < 5; ++i) TRY(stage_out(ctx, out_h[i], out_d[i], (size_t)N));
    double h6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    TRY(stage_out(ctx, h6, dsums, 6));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 6; ++i) sums[i] = h6[i];
    return all_finite(h6, 6) ? PGPS_OK : PGPS_E_NUMERIC;
}

extern "C" int pgps_lik_sites_dev_f64(pgps_ctx* ctx, long N, int lik, double par, const double* ys, const double* f_a,
                                      const double* alpha_a, const double* f_b, const double* alpha_b, double step,
                                      double* f_out, double* alpha_out, double* zs_out, double* ss_out, double* sums) {
    return lik_sites_dev(ctx, N, lik, par, ys, f_a, alpha_a, f_b, alpha_b, step, f_out, alpha_out, zs_out, ss_out, sums);
}

extern "C" int pgps_lik_sites_f64(pgps_ctx* ctx, long N, int lik, double par, const double* ys, const double* f_a,
                                  const double* alpha_a, const double* f_b, const double* alpha_b, double step, double* f_out,
                                  double* alpha_out, double* zs_out, double* ss_out, double* sums) {
    TRY(lik_sites_args(ctx, N, lik, par, ys, f_a, alpha_a, f_b, alpha_b, step, f_out, alpha_out, zs_out, ss_out, sums));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double* in_h[5] = {ys, f_a, alpha_a, f_b, alpha_b};
    double *in_d[5], *out_d[4], *dsums;
    TRY(stage_rows(ctx, ctx->st[4], N, 5, in_h, in_d));
    TRY(stage_rows(ctx, ctx->st[7], N, 4, nullptr, out_d));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 3, &dsums));
    TRY(lik_sites_dev(ctx, N, lik, par, in_d[0], in_d[1], in_d[2], f_b ? in_d[3] : nullptr, f_b ? in_d[4] : nullptr, step,
                      out_d[0], out_d[1], out_d[2], out_d[3], dsums));
    double* out_h[4] = {f_out, alpha_out, zs_out, ss_out};
    for (int i = 0; i < 4; ++i) TRY(stage_out(ctx, out_h[i], out_d[i], (size_t)N));
    double h3[3] = {0.0, 0.0, 0.0};
    TRY(stage_out(ctx, h3, dsums, 3));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 3; ++i) sums[i] = h3[i];
    return all_finite(h3, 3) ? PGPS_OK : PGPS_E_NUMERIC;
}
