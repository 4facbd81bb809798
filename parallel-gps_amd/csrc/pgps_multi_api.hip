// pgps_multi_api.hip -- the multi-column entry points of the C ABI (include/pgps.h: pgps_gp_ll_multi_*,
// pgps_gp_predict_multi_*, pgps_gp_ll_grad_multi_*, pgps_gp_whiten_multi_*, pgps_gp_gram_multi_*): argument checks, the all-or-none check of the host forms, staging
// through the context's buffers, the merge of training and query times with the source ROW of every merged step as its
// payload, dispatch to launch_gp_multi<d> (pgps_multi_inst.hip), launch_gp_multi_grad<d> (pgps_multi_grad_inst.hip) and
// launch_gp_whiten<d> (pgps_whiten_inst.hip).
#include "pgps_host.h"

using namespace pgps;

// rows[i] = i, as doubles: the payload k_merge_sorted weaves (it carries one value per training step; a query step gets NaN),
// so a merged step knows which row of ys (N, M) to read and the (N, M) array itself is never copied
static __global__ void k_multi_rows(long N, double* rows) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) rows[i] = (double)i;
}

static int multi_args(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2, const double* Pinf,
                      const double* H, double R, const double* ts, const double* ys, GpMultiArgs* a) {
    if (!ctx || N < 1 || M < 1 || !N1 || !Pinf || !H || !ts || !ys) return PGPS_E_INVALID;
    if (!(R > 0.0) || !(lam > 0.0)) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    *a = GpMultiArgs{};
    a->N = N;
    a->M = M;
    a->R = R;
    a->ys = ys;
    a->ys_aligned = aligned16(ys) ? 1 : 0;
    a->m.lam = lam;
    for (int i = 0; i < 9; ++i) { a->m.N1[i] = 0; a->m.N2[i] = 0; a->m.Pinf[i] = 0; }
    for (int i = 0; i < d * d; ++i) { a->m.N1[i] = N1[i]; a->m.N2[i] = N2 ? N2[i] : 0.0; a->m.Pinf[i] = Pinf[i]; }
    for (int i = 0; i < 3; ++i) a->m.H[i] = i < d ? H[i] : 0.0;
    a->m.ts = ts;
    return PGPS_OK;
}

static int multi_dispatch(pgps_ctx* ctx, int d, const GpMultiArgs& a, int predict, double* ll) {
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_multi<D()>(ctx, a, predict, ll); });
}

static int gp_ll_multi_dev(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2,
                           const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                           double* ll) {
    GpMultiArgs a;
    TRY(multi_args(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, &a));
    if (!ll) return PGPS_E_INVALID;
    a.m.t_prev = t0;
    return multi_dispatch(ctx, d, a, 0, ll);
}

static int gp_ll_grad_multi_dev(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2,
                                const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                                double* out) {
    GpMultiArgs a;
    TRY(multi_args(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, &a));
    if (!out) return PGPS_E_INVALID;
    a.m.t_prev = t0;
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_multi_grad<D()>(ctx, a, out); });
}

// w (N, M) or gram (M, M), the other null (launch_gp_whiten)
static int gp_whiten_multi_dev(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2,
                               const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                               double* w, double* gram, double* logdet, long* n_obs) {
    GpMultiArgs a;
    TRY(multi_args(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, &a));
    if ((!w && !gram) || !logdet || !n_obs) return PGPS_E_INVALID;
    if (gram && M > kGramMax) return PGPS_E_INVALID;
    a.m.t_prev = t0;
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_whiten<D()>(ctx, a, w, gram, logdet, n_obs); });
}

static int gp_predict_multi_dev(pgps_ctx* ctx, long N, long K, int M, int d, double lam, const double* N1, const double* N2,
                                const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                                const double* tq, double* mean, double* var, double* ll) {
    GpMultiArgs a;
    TRY(multi_args(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, &a));
    if (K < 1 || !tq || !mean || !var) return PGPS_E_INVALID;
    if (N + K > 0x7fffffffL) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double* rows;
    TRY(stage_in<double>(ctx, ctx->st[5], nullptr, (size_t)N, &rows));
    k_multi_rows<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream>>>(N, rows);
    HIPCHK(ctx, hipGetLastError());
    Merged<double> mg;
    TRY(merged_front<double>(ctx, ctx->st, N, K, ts, rows, tq, &mg));        // (equal times: the shorter array's point first)
    a.N = N + K;
    a.m.ts = mg.ts;
    a.m.t_prev = t0;
    a.rows = mg.ys;
    a.qslot = mg.qslot;
    a.pmean = mean;
    a.pvar = var;
    a.mean_aligned = aligned16(mean) ? 1 : 0;
    return multi_dispatch(ctx, d, a, 1, ll);
}

// every row of ys (N, M) observed in all columns or in none?
static bool rows_all_or_none(long N, int M, const double* ys) {
    for (long i = 0; i < N; ++i) {
        const double* r = ys + (size_t)i * M;
        int nan = 0;
        for (int j = 0; j < M; ++j) nan += std::isnan(r[j]) ? 1 : 0;
        if (nan != 0 && nan != M) return false;
    }
    return true;
}

static int ll_multi_result(int M, const double* llh, double* ll) {
    bool finite = true;
    for (int j = 0; j < M; ++j) {
        if (ll) ll[j] = llh[j];
        finite = finite && std::isfinite(llh[j]);
    }
    return finite ? PGPS_OK : PGPS_E_NUMERIC;
}

extern "C" int pgps_gp_ll_multi_dev_f64(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2,
                                        const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                        double t0, double* ll) {
    return gp_ll_multi_dev(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, t0, ll);
}

extern "C" int pgps_gp_ll_multi_f64(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2,
                                    const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                    double t0, double* ll) {
    GpMultiArgs chk;
    TRY(multi_args(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, &chk));
    if (!ll) return PGPS_E_INVALID;
    if (!rows_all_or_none(N, M, ys)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double *dts, *dys, *dll;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N * M, &dys));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)M, &dll));
    TRY(gp_ll_multi_dev(ctx, N, M, d, lam, N1, N2, Pinf, H, R, dts, dys, t0, dll));
    std::vector<double> llh((size_t)M);
    TRY(stage_out(ctx, llh.data(), dll, (size_t)M));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ll_multi_result(M, llh.data(), ll);
}

extern "C" int pgps_gp_predict_multi_dev_f64(pgps_ctx* ctx, long N, long K, int M, int d, double lam, const double* N1,
                                             const double* N2, const double* Pinf, const double* H, double R, const double* ts,
                                             const double* ys, double t0, const double* tq, double* mean, double* var,
                                             double* ll) {
    return gp_predict_multi_dev(ctx, N, K, M, d, lam, N1, N2, Pinf, H, R, ts, ys, t0, tq, mean, var, ll);
}

extern "C" int pgps_gp_predict_multi_f64(pgps_ctx* ctx, long N, long K, int M, int d, double lam, const double* N1,
                                         const double* N2, const double* Pinf, const double* H, double R, const double* ts,
                                         const double* ys, double t0, const double* tq, double* mean, double* var, double* ll) {
    GpMultiArgs chk;
    TRY(multi_args(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, &chk));
    if (K < 1 || !tq || !mean || !var) return PGPS_E_INVALID;
    if (N + K > 0x7fffffffL) return PGPS_E_INVALID;
    if (!rows_all_or_none(N, M, ys)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double *dts, *dys, *dtq, *dmean, *dvar, *dll;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N * M, &dys));
    TRY(stage_in(ctx, ctx->st[3], tq, (size_t)K, &dtq));
    TRY(stage_in<double>(ctx, ctx->st[7], nullptr, (size_t)K * M, &dmean));
    TRY(stage_in<double>(ctx, ctx->st[8], nullptr, (size_t)K, &dvar));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)M, &dll));
    TRY(gp_predict_multi_dev(ctx, N, K, M, d, lam, N1, N2, Pinf, H, R, dts, dys, t0, dtq, dmean, dvar, dll));
    std::vector<double> llh((size_t)M);
    TRY(stage_out(ctx, mean, dmean, (size_t)K * M));
    TRY(stage_out(ctx, var, dvar, (size_t)K));
    TRY(stage_out(ctx, llh.data(), dll, (size_t)M));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ll_multi_result(M, llh.data(), ll);
}

extern "C" int pgps_gp_ll_grad_multi_dev_f64(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2,
                                             const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                             double t0, double* out) {
    return gp_ll_grad_multi_dev(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, t0, out);
}

extern "C" int pgps_gp_ll_grad_multi_f64(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2,
                                         const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                         double t0, double* out) {
    GpMultiArgs chk;
    TRY(multi_args(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, &chk));
    if (!out) return PGPS_E_INVALID;
    if (!rows_all_or_none(N, M, ys)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nout = (size_t)M + (size_t)(d * d + 2 * d + 1);
    double *dts, *dys, *dout;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N * M, &dys));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, nout, &dout));
    TRY(gp_ll_grad_multi_dev(ctx, N, M, d, lam, N1, N2, Pinf, H, R, dts, dys, t0, dout));
    std::vector<double> outh(nout);
    TRY(stage_out(ctx, outh.data(), dout, nout));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < nout; ++i) out[i] = outh[i];
    return ll_multi_result(M, outh.data(), nullptr);
}

// the host form of both: nout doubles of w or gram come back, with logdet and n_obs
static int gp_whiten_multi_host(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2,
                                const double* Pinf, const double* H, double R, const double* ts, const double* ys, double t0,
                                bool want_gram, double* out, double* logdet, long* n_obs) {
    GpMultiArgs chk;
    TRY(multi_args(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, &chk));
    if (!out || !logdet || !n_obs) return PGPS_E_INVALID;
    if (want_gram && M > kGramMax) return PGPS_E_INVALID;
    if (!rows_all_or_none(N, M, ys)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nout = want_gram ? (size_t)M * M : (size_t)N * M;
    double *dts, *dys, *dout, *dsum;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N * M, &dys));
    TRY(stage_in<double>(ctx, ctx->st[7], nullptr, nout, &dout));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 2, &dsum));           // logdet | n_obs (a long: 8 bytes as well)
    static_assert(sizeof(long) == sizeof(double), "n_obs shares the staging buffer of logdet");
    long* dcnt = reinterpret_cast<long*>(dsum + 1);
    TRY(gp_whiten_multi_dev(ctx, N, M, d, lam, N1, N2, Pinf, H, R, dts, dys, t0, want_gram ? nullptr : dout,
                            want_gram ? dout : nullptr, dsum, dcnt));
    TRY(stage_out(ctx, out, dout, nout));
    TRY(stage_out(ctx, logdet, dsum, (size_t)1));
    TRY(stage_out(ctx, n_obs, dcnt, (size_t)1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    bool finite = std::isfinite(*logdet);
    for (size_t i = 0; i < nout && finite; ++i) finite = std::isfinite(out[i]);
    return finite ? PGPS_OK : PGPS_E_NUMERIC;
}

extern "C" int pgps_gp_whiten_multi_dev_f64(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2,
                                            const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                            double t0, double* w, double* logdet, long* n_obs) {
    if (!w) return PGPS_E_INVALID;
    return gp_whiten_multi_dev(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, t0, w, nullptr, logdet, n_obs);
}

extern "C" int pgps_gp_whiten_multi_f64(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2,
                                        const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                        double t0, double* w, double* logdet, long* n_obs) {
    return gp_whiten_multi_host(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, t0, false, w, logdet, n_obs);
}

extern "C" int pgps_gp_gram_multi_dev_f64(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2,
                                          const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                          double t0, double* gram, double* logdet, long* n_obs) {
    if (!gram) return PGPS_E_INVALID;
    return gp_whiten_multi_dev(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, t0, nullptr, gram, logdet, n_obs);
}

extern "C" int pgps_gp_gram_multi_f64(pgps_ctx* ctx, long N, int M, int d, double lam, const double* N1, const double* N2,
                                      const double* Pinf, const double* H, double R, const double* ts, const double* ys,
                                      double t0, double* gram, double* logdet, long* n_obs) {
    return gp_whiten_multi_host(ctx, N, M, d, lam, N1, N2, Pinf, H, R, ts, ys, t0, true, gram, logdet, n_obs);
}
