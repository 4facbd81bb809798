// pgps_het_api.hip -- the per-observation-noise entry points of the C ABI (include/pgps.h: pgps_gp_ll_het_*,
// pgps_gp_predict_het_*, pgps_gp_ll_grad_adj_het_*): argument checks, the one scan of `rs` the host forms
// make, staging through the context's buffers (rs travels behind ys in the same buffer), the merge of training and query
// times with ys AND rs as its payloads, dispatch to launch_gp_het<d> / launch_gp_adj_het<d> (pgps_het_inst.hip).
#include "pgps_host.h"

using namespace pgps;

static int het_args(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                    const double* H, double R, const double* ts, const double* ys, const double* rs, GpArgs<double>* g) {
    if (!ctx || N < 1 || !N1 || !Pinf || !H || !ts || !ys || !rs) return PGPS_E_INVALID;
    if (!(R >= 0.0) || !std::isfinite(R) || !(lam > 0.0)) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    *g = GpArgs<double>{};
    g->s.N = N;
    g->s.R = R;
    g->s.ys = ys;
    g->m.lam = lam;
    for (int i = 0; i < 9; ++i) { g->m.N1[i] = 0; g->m.N2[i] = 0; g->m.Pinf[i] = 0; }
    for (int i = 0; i < d * d; ++i) { g->m.N1[i] = N1[i]; g->m.N2[i] = N2 ? N2[i] : 0.0; g->m.Pinf[i] = Pinf[i]; }
    for (int i = 0; i < 3; ++i) g->m.H[i] = i < d ? H[i] : 0.0;
    g->m.ts = ts;
    return PGPS_OK;
}

// the host forms' one pass over rs: at every observed row s_k is finite and >= 0 and R + s_k > 0 (rows where ys is NaN are not
// looked at)
static bool het_noise_valid(long N, double R, const double* ys, const double* rs) {
    for (long k = 0; k < N; ++k) {
        if (std::isnan(ys[k])) continue;
        const double s = rs[k];
        if (!std::isfinite(s) || s < 0.0 || !(R + s > 0.0)) return false;
    }
    return true;
}

// ys and rs of a host call into ONE staging buffer: [ys (N) | rs (N)]
static int het_stage_series(pgps_ctx* ctx, long N, const double* ys, const double* rs, double** dys, double** drs) {
    TRY(stage_in<double>(ctx, ctx->st[4], nullptr, 2 * (size_t)N, dys));
    *drs = *dys + N;
    HIPCHK(ctx, hipMemcpyAsync(*dys, ys, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(*drs, rs, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return PGPS_OK;
}

static int gp_ll_het_dev(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                         const double* H, double R, const double* ts, const double* ys, const double* rs, double t0, double* ll) {
    GpArgs<double> g;
    TRY(het_args(ctx, N, d, lam, N1, N2, Pinf, H, R, ts, ys, rs, &g));
    if (!ll) return PGPS_E_INVALID;
    g.m.t_prev = t0;
    g.s.ll = ll;
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_het<D()>(ctx, g, rs); });
}

static int gp_predict_het_dev(pgps_ctx* ctx, long N, long K, int d, double lam, const double* N1, const double* N2,
                              const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                              const double* rs, double t0, const double* tq, double* mean, double* var, double* ll) {
    GpArgs<double> g;
    TRY(het_args(ctx, N, d, lam, N1, N2, Pinf, H, R, ts, ys, rs, &g));
    if (K < 1 || !tq || !mean || !var) return PGPS_E_INVALID;
    if (N + K > 0x7fffffffL) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t m = (size_t)(N + K), dd = (size_t)d * d;
    const size_t mpad = (m + 31) / 32 * 32;         // rs_m starts on a 256-byte boundary behind ys_m (whole 16-byte stores)
    double *ts_m, *ys_m, *fms, *fPs, *dll;
    int* qslot;
    TRY(stage_in<double>(ctx, ctx->st[0], nullptr, m, &ts_m));
    TRY(stage_in<double>(ctx, ctx->st[1], nullptr, 2 * mpad, &ys_m));
    TRY(stage_in<int>(ctx, ctx->st[2], nullptr, m, &qslot));
    double* rs_m = ys_m + mpad;
    TRY(launch_merge_het(ctx, N, K, ts, ys, rs, tq, ts_m, ys_m, rs_m, qslot));      // (equal times: the shorter array's point first)
    TRY(stage_in<double>(ctx, ctx->st[5], nullptr, m * d, &fms));
    TRY(stage_in<double>(ctx, ctx->st[6], nullptr, m * dd, &fPs));
    TRY(stage_in<double>(ctx, ctx->st[11], nullptr, 2, &dll));
    g.s.N = (long)m;
    g.s.ys = ys_m;
    g.s.fms = fms; g.s.fPs = fPs;
    g.s.ll = ll ? ll : dll;
    g.m.ts = ts_m;
    g.m.t_prev = t0;
    g.qslot = qslot;
    g.pmean = mean;
    g.pvar = var;
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_het<D()>(ctx, g, rs_m); });
}

static int gp_adj_het_dev(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                          const double* H, double R, const double* ts, double t0, const double* ys, const double* rs,
                          double* out) {
    GpArgs<double> g;
    TRY(het_args(ctx, N, d, lam, N1, N2, Pinf, H, R, ts, ys, rs, &g));
    if (!out) return PGPS_E_INVALID;
    g.m.t_prev = t0;
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_adj_het<D()>(ctx, g, rs, out); });
}

extern "C" int pgps_gp_ll_het_dev_f64(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2,
                                      const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                      const double* rs, double t0, double* ll) {
    return gp_ll_het_dev(ctx, N, d, lam, N1, N2, Pinf, H, R, ts, ys, rs, t0, ll);
}

extern "C" int pgps_gp_ll_het_f64(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2,
                                  const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                  const double* rs, double t0, double* ll) {
    GpArgs<double> chk;
    TRY(het_args(ctx, N, d, lam, N1, N2, Pinf, H, R, ts, ys, rs, &chk));
    if (!het_noise_valid(N, R, ys, rs)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double *dts, *dys, *drs, *dll;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(het_stage_series(ctx, N, ys, rs, &dys, &drs));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 2, &dll));
    TRY(gp_ll_het_dev(ctx, N, d, lam, N1, N2, Pinf, H, R, dts, dys, drs, t0, dll));
    double llh = 0.0;
    TRY(stage_out(ctx, &llh, dll, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ll) *ll = llh;
    return std::isfinite(llh) ? PGPS_OK : PGPS_E_NUMERIC;
}

extern "C" int pgps_gp_predict_het_dev_f64(pgps_ctx* ctx, long N, long K, int d, double lam, const double* N1, const double* N2,
                                           const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                           const double* rs, double t0, const double* tq, double* mean, double* var,
                                           double* ll) {
    return gp_predict_het_dev(ctx, N, K, d, lam, N1, N2, Pinf, H, R, ts, ys, rs, t0, tq, mean, var, ll);
}

extern "C" int pgps_gp_predict_het_f64(pgps_ctx* ctx, long N, long K, int d, double lam, const double* N1, const double* N2,
                                       const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                       const double* rs, double t0, const double* tq, double* mean, double* var, double* ll) {
    GpArgs<double> chk;
    TRY(het_args(ctx, N, d, lam, N1, N2, Pinf, H, R, ts, ys, rs, &chk));
    if (K < 1 || !tq || !mean || !var) return PGPS_E_INVALID;
    if (N + K > 0x7fffffffL) return PGPS_E_INVALID;
    if (!het_noise_valid(N, R, ys, rs)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double *dts, *dys, *drs, *dtq, *dmean, *dvar, *dll;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(het_stage_series(ctx, N, ys, rs, &dys, &drs));
    TRY(stage_in(ctx, ctx->st[3], tq, (size_t)K, &dtq));
    TRY(stage_in<double>(ctx, ctx->st[7], nullptr, (size_t)K, &dmean));
    TRY(stage_in<double>(ctx, ctx->st[8], nullptr, (size_t)K, &dvar));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 2, &dll));
    TRY(gp_predict_het_dev(ctx, N, K, d, lam, N1, N2, Pinf, H, R, dts, dys, drs, t0, dtq, dmean, dvar, dll));
    TRY(stage_out(ctx, mean, dmean, (size_t)K));
    TRY(stage_out(ctx, var, dvar, (size_t)K));
    double llh = 0.0;
    TRY(stage_out(ctx, &llh, dll, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ll) *ll = llh;
    return std::isfinite(llh) ? PGPS_OK : PGPS_E_NUMERIC;
}

extern "C" int pgps_gp_ll_grad_adj_het_dev_f64(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2,
                                               const double* Pinf, const double* H, double R, const double* ts, double t0,
                                               const double* ys, const double* rs, double* out) {
    return gp_adj_het_dev(ctx, N, d, lam, N1, N2, Pinf, H, R, ts, t0, ys, rs, out);
}

extern "C" int pgps_gp_ll_grad_adj_het_f64(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2,
                                           const double* Pinf, const double* H, double R, const double* ts, double t0,
                                           const double* ys, const double* rs, double* out) {
    GpArgs<double> chk;
    TRY(het_args(ctx, N, d, lam, N1, N2, Pinf, H, R, ts, ys, rs, &chk));
    if (!out) return PGPS_E_INVALID;
    if (!het_noise_valid(N, R, ys, rs)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nout = (size_t)(1 + d * d + 2 * d + 1);
    double *dts, *dys, *drs, *dout;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(het_stage_series(ctx, N, ys, rs, &dys, &drs));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, nout, &dout));
    TRY(gp_adj_het_dev(ctx, N, d, lam, N1, N2, Pinf, H, R, dts, t0, dys, drs, dout));
    TRY(stage_out(ctx, out, dout, nout));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return std::isfinite(out[0]) ? PGPS_OK : PGPS_E_NUMERIC;
}
