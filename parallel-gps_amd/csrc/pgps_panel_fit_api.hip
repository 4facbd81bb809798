// pgps_panel_fit_api.hip -- the per-series fit of a panel (include/pgps.h: pgps_gp_panel_fit_*):
// argument checks, the start records, staging of the host form through the context's buffers, dispatch to
// launch_gp_panel_fit<d> (pgps_panel_fit_inst.hip).
#include "pgps_host.h"
#include "pgps_fit.h"
#include "pgps_panel_fit.h"

using namespace pgps;

static bool positive(double v) { return std::isfinite(v) && v > 0.0; }

// everything a call can be refused for before anything is staged
static int fit_check(pgps_ctx* ctx, long S, const long* offs, int d, const double* unit, const double* ts, const double* ys,
                     bool het, const double* theta0, const double* lo, const double* hi, const int* free3, double gtol,
                     int max_iter, const double* thetas, const double* info) {
    if (!ctx || S < 1 || !offs || !ts || !ys || !theta0 || !lo || !hi || !free3 || !thetas || !info) return PGPS_E_INVALID;
    if (d < 1 || d > 3) return PGPS_E_UNSUPPORTED_DIM;
    if (d == 3 && !unit) return PGPS_E_INVALID;
    if (offs[0] != 0) return PGPS_E_INVALID;
    for (long s = 0; s < S; ++s) {
        const long n = offs[s + 1] - offs[s];
        if (n < 1 || n > PGPS_PANEL_MAX_STEPS) return PGPS_E_INVALID;
    }
    if (d == 3 && !(positive(unit[0]))) return PGPS_E_INVALID;         // lam of the unit row
    if (!fit_gtol_valid(gtol) || !fit_max_iter_valid(max_iter)) return PGPS_E_INVALID;
    for (long s = 0; s < S; ++s)
        for (int i = 0; i < kFitP; ++i) {
            const size_t at = (size_t)s * kFitP + i;
            if (free3[i]) {
                if (!positive(theta0[at]) || !positive(lo[at]) || !positive(hi[at]) || !(lo[at] < hi[at])) return PGPS_E_INVALID;
            } else if (i < 2) {
                if (!positive(theta0[at])) return PGPS_E_INVALID;      // a fixed variance or lengthscale is still a model's
            } else {
                if (!std::isfinite(theta0[at]) || theta0[at] < 0.0 || (!het && !(theta0[at] > 0.0))) return PGPS_E_INVALID;
            }
        }
    return PGPS_OK;
}

// the host form's one pass over rs (the rule of pgps_gp_panel_ll_f64 at the observed rows: finite, >= 0, and R + rs[k] > 0 --
// a free noise variance is > 0 everywhere in its box, a fixed one is the series' own)
static bool fit_noise_valid(long S, const long* offs, const double* ys, const double* rs, const double* theta0, bool noise_free) {
    for (long s = 0; s < S; ++s) {
        const double R = theta0[(size_t)s * kFitP + 2];
        for (long k = offs[s]; k < offs[s + 1]; ++k) {
            if (std::isnan(ys[k])) continue;
            const double v = rs[k];
            if (!std::isfinite(v) || v < 0.0 || (!noise_free && !(R + v > 0.0))) return false;
        }
    }
    return true;
}

// the caller's unit row [lam | N1 | N2 | Pinf | H | R] at the fixed device stride (null at d < 3: nothing reads it)
static void fit_pack_unit(int d, const double* unit, std::vector<double>& packed) {
    packed.assign((size_t)kGpModelStride, 0.0);
    packed[0] = 1.0;
    if (!unit) return;
    const int dd = d * d;
    packed[0] = unit[0];
    for (int i = 0; i < dd; ++i) { packed[1 + i] = unit[1 + i]; packed[10 + i] = unit[1 + dd + i]; packed[19 + i] = unit[1 + 2 * dd + i]; }
    for (int i = 0; i < d; ++i) packed[28 + i] = unit[1 + 3 * dd + i];
}

static void fit_records(long S, const double* theta0, const double* lo, const double* hi, const int* free3,
                        std::vector<double>& rec) {
    rec.assign((size_t)S * kFitRecord, 0.0);
    for (long s = 0; s < S; ++s)
        for (int i = 0; i < kFitP; ++i) {
            const size_t at = (size_t)s * kFitP + i;
            double* r = rec.data() + (size_t)s * kFitRecord;
            r[kFitRecTheta0 + i] = theta0[at];
            if (free3[i]) {
                r[kFitRecX0 + i] = std::log(theta0[at]); r[kFitRecXlo + i] = std::log(lo[at]); r[kFitRecXhi + i] = std::log(hi[at]);
                r[kFitRecLo + i] = lo[at]; r[kFitRecHi + i] = hi[at];
            } else {
                r[kFitRecLo + i] = theta0[at]; r[kFitRecHi + i] = theta0[at];
            }
        }
}

static int fit_dev(pgps_ctx* ctx, int d, const PanelFitCall& c) {
    RoctxRange range_("panel_fit");
    return for_dim<1, 3>(d, [&](auto D) { return launch_gp_panel_fit<D()>(ctx, c); });
}

extern "C" int pgps_gp_panel_fit_dev_f64(pgps_ctx* ctx, long S, const long* offs, int d, const double* unit, const double* ts,
                                         const double* ys, const double* rs, const double* theta0, const double* lo,
                                         const double* hi, const int* free3, double gtol, int max_iter, double* thetas,
                                         double* info) {
    TRY(fit_check(ctx, S, offs, d, unit, ts, ys, rs != nullptr, theta0, lo, hi, free3, gtol, max_iter, thetas, info));
    std::vector<double> packed, rec;
    fit_pack_unit(d, unit, packed);
    fit_records(S, theta0, lo, hi, free3, rec);
    PanelFitCall c{};
    c.S = S; c.offs = offs; c.unit = packed.data(); c.records = rec.data(); c.ts = ts; c.ys = ys; c.rs = rs;
    for (int i = 0; i < kFitP; ++i) c.free_[i] = free3[i] ? 1 : 0;
    c.gtol = gtol; c.max_iter = max_iter; c.thetas = thetas; c.info = info;
    return fit_dev(ctx, d, c);
}

extern "C" int pgps_gp_panel_fit_f64(pgps_ctx* ctx, long S, const long* offs, int d, const double* unit, const double* ts,
                                     const double* ys, const double* rs, const double* theta0, const double* lo, const double* hi,
                                     const int* free3, double gtol, int max_iter, double* thetas, double* info) {
    TRY(fit_check(ctx, S, offs, d, unit, ts, ys, rs != nullptr, theta0, lo, hi, free3, gtol, max_iter, thetas, info));
    if (rs && !fit_noise_valid(S, offs, ys, rs, theta0, free3[2] != 0)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)offs[S], nt = (size_t)S * kFitP, ni = (size_t)S * kFitInfo;
    std::vector<double> packed, rec;
    fit_pack_unit(d, unit, packed);
    fit_records(S, theta0, lo, hi, free3, rec);
    PanelFitCall c{};
    c.S = S; c.offs = offs; c.unit = packed.data(); c.records = rec.data();
    for (int i = 0; i < kFitP; ++i) c.free_[i] = free3[i] ? 1 : 0;
    c.gtol = gtol; c.max_iter = max_iter;
    // ts, and [ys | rs] in ONE staging buffer, as the panel's host forms stage them; [thetas | info] leave through one
    double *dts, *dys, *dout;
    TRY(stage_in(ctx, ctx->st[10], ts, N, &dts));
    TRY(stage_in<double>(ctx, ctx->st[4], nullptr, (rs ? 2 : 1) * N, &dys));
    HIPCHK(ctx, hipMemcpyAsync(dys, ys, N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (rs) HIPCHK(ctx, hipMemcpyAsync(dys + N, rs, N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, nt + ni, &dout));
    c.ts = dts; c.ys = dys; c.rs = rs ? dys + N : nullptr;
    c.thetas = dout; c.info = dout + nt;
    TRY(fit_dev(ctx, d, c));
    std::vector<double> outh(nt + ni);
    TRY(stage_out(ctx, outh.data(), (const double*)dout, nt + ni));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(thetas, outh.data(), nt * sizeof(double));
    memcpy(info, outh.data() + nt, ni * sizeof(double));
    for (long s = 0; s < S; ++s)
        if (!std::isfinite(info[(size_t)s * kFitInfo])) return PGPS_E_NUMERIC;
    return PGPS_OK;
}
