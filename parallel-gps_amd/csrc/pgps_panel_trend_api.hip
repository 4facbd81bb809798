// pgps_panel_trend_api.hip -- the panel's GLS solves and the profile gradient of every series in one call (include/pgps.h:
// pgps_gp_panel_trend_solve_*, pgps_gp_panel_profile_grad_*).  Argument checks (those of
// pgps_gp_panel_gram_* for the chained call), the host forms' staging through the context's buffers, and the chain itself:
// the Gram launches, the solve kernel, the residual kernel and the adjoint launches queued back to back behind ONE table copy
// and ONE stream synchronisation (pgps_panel_plan.h).
#include "pgps_host.h"
#include "pgps_panel_plan.h"
#include "pgps_scratch.h"

using namespace pgps;

static int solve_check(pgps_ctx* ctx, long S, int C, const double* records, const double* betas, const double* sol) {
    if (!ctx || S < 1 || C < 1 || C > kPanelGramMax || !records || !sol) return PGPS_E_INVALID;
    if (C > 1 && !betas) return PGPS_E_INVALID;
    return PGPS_OK;
}

extern "C" int pgps_gp_panel_trend_solve_dev_f64(pgps_ctx* ctx, long S, int C, const double* records, double* betas, double* sol) {
    TRY(solve_check(ctx, S, C, records, betas, sol));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return launch_panel_trend_solve(ctx, S, C, records, betas, sol);
}

extern "C" int pgps_gp_panel_trend_solve_f64(pgps_ctx* ctx, long S, int C, const double* records, double* betas, double* sol) {
    TRY(solve_check(ctx, S, C, records, betas, sol));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t p = (size_t)C - 1, rec = (size_t)C * C + 2, nb = (size_t)S * p, ns = (size_t)S * (p * p + 4);
    double *drec, *dres;
    TRY(stage_in(ctx, ctx->st[4], records, (size_t)S * rec, &drec));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, nb + ns, &dres));            // [betas | sol]: ONE copy back
    TRY(launch_panel_trend_solve(ctx, S, C, drec, dres, dres + nb));
    // the results come back through a vector of the call: an error leaves the caller's outputs untouched
    std::vector<double> resh(nb + ns);
    TRY(stage_out(ctx, resh.data(), dres, nb + ns));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (nb) memcpy(betas, resh.data(), nb * sizeof(double));
    memcpy(sol, resh.data() + nb, ns * sizeof(double));
    return PGPS_OK;
}

// ---- the chain --------------------------------------------------------------------------------------------------------------
namespace {
struct ProfileCall {
    long S;
    const long* offs;           // host
    int nmodels;
    const double* models;       // host, (nmodels, kGpModelStride)
    int C;
    const double *ts, *V, *rs;  // device
    double *betas, *sol, *ys_work, *out;
};
}  // namespace

// Both phases are planned first.  ONE table [packed models | Gram records' PanelDesc | adjoint pass's PanelDesc | offs] goes up,
// ctx->ws is sized for the larger phase, and the Gram records get their buffer -- all before the first launch, behind the one
// synchronisation that lets the host vectors die.  From there on nothing is allocated, copied or waited for.
template <int D>
static int profile_chain(pgps_ctx* ctx, const ProfileCall& a) {
    const size_t S = (size_t)a.S, rec = (size_t)a.C * a.C + 2;
    PanelGramCall g{};
    g.S = a.S; g.offs = a.offs; g.nmodels = a.nmodels; g.models = a.models; g.C = a.C; g.ts = a.ts; g.V = a.V; g.rs = a.rs;
    PanelCall c{};
    c.S = a.S; c.offs = a.offs; c.nmodels = a.nmodels; c.models = a.models; c.ts = a.ts; c.ys = a.ys_work; c.rs = a.rs; c.out = a.out;
    PanelGramPlan gplan;
    panel_gram_plan(ctx, g, gplan);
    PanelPlan aplan;
    panel_plan<D>(ctx, c, PANEL_GRAD, aplan);

    const size_t mbytes = align_up((size_t)a.nmodels * kGpModelStride * sizeof(double), 256);
    const size_t dbytes = align_up(S * sizeof(PanelDesc), 256);
    std::vector<char> tables(mbytes + 2 * dbytes + (S + 1) * sizeof(long));
    memcpy(tables.data(), a.models, (size_t)a.nmodels * kGpModelStride * sizeof(double));
    memcpy(tables.data() + mbytes, gplan.desc.data(), S * sizeof(PanelDesc));
    memcpy(tables.data() + mbytes + dbytes, aplan.desc.data(), S * sizeof(PanelDesc));
    memcpy(tables.data() + mbytes + 2 * dbytes, a.offs, (S + 1) * sizeof(long));
    TRY(ensure(ctx, ctx->panel, tables.size()));
    TRY(ensure(ctx, ctx->ws, std::max(gplan.need_w, aplan.need_w)));
    TRY(ensure(ctx, ctx->gadj, aplan.need_g));
    TRY(stage_in<double>(ctx, ctx->st[11], nullptr, S * rec, &g.out));
    HIPCHK(ctx, hipMemcpyAsync(ctx->panel.p, tables.data(), tables.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const char* base = (const char*)ctx->panel.p;
    const double* dmodels = reinterpret_cast<const double*>(base);
    const PanelDesc* gdesc = reinterpret_cast<const PanelDesc*>(base + mbytes);
    const PanelDesc* adesc = reinterpret_cast<const PanelDesc*>(base + mbytes + dbytes);
    const long* doffs = reinterpret_cast<const long*>(base + mbytes + 2 * dbytes);

    TRY(panel_gram_enqueue<D>(ctx, g, gplan, dmodels, gdesc));
    TRY(launch_panel_trend_solve(ctx, a.S, a.C, g.out, a.betas, a.sol));
    TRY(panel_residual_enqueue(ctx, a.S, a.offs, doffs, a.C, a.V, a.betas, a.ys_work));
    return panel_enqueue<D>(ctx, c, PANEL_GRAD, aplan, dmodels, adesc);
}

static int profile_dev(pgps_ctx* ctx, int d, const ProfileCall& a) {
    RoctxRange range_("parallel_filter");
    return for_dim<1, 3>(d, [&](auto D) { return profile_chain<D()>(ctx, a); });
}

static int profile_check(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models, int C, const double* ts,
                         const double* V, bool het, const double* betas, const double* sol, const double* out) {
    TRY(panel_gram_check(ctx, S, offs, d, nmodels, models, C, ts, V, het, out));
    if (!sol || (C > 1 && !betas)) return PGPS_E_INVALID;
    return PGPS_OK;
}

extern "C" int pgps_gp_panel_profile_grad_dev_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models,
                                                  int C, const double* ts, const double* V, const double* rs, double* betas,
                                                  double* sol, double* ys_work, double* out) {
    TRY(profile_check(ctx, S, offs, d, nmodels, models, C, ts, V, rs != nullptr, betas, sol, out));
    if (!ys_work) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<double> packed;
    panel_pack_models(nmodels, d, models, packed);
    const ProfileCall a{S, offs, nmodels, packed.data(), C, ts, V, rs, betas, sol, ys_work, out};
    return profile_dev(ctx, d, a);
}

extern "C" int pgps_gp_panel_profile_grad_f64(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models,
                                              int C, const double* ts, const double* V, const double* rs, double* betas, double* sol,
                                              double* out) {
    TRY(profile_check(ctx, S, offs, d, nmodels, models, C, ts, V, rs != nullptr, betas, sol, out));
    if (!panel_gram_rows_valid(S, offs, d, nmodels, models, C, V, rs)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)offs[S], p = (size_t)C - 1, nout = (size_t)(2 + d * d + 2 * d);
    const size_t nb = (size_t)S * p, ns = (size_t)S * (p * p + 4), no = (size_t)S * nout;
    std::vector<double> packed;
    panel_pack_models(nmodels, d, models, packed);
    // [V (N, C) | rs (N)] share ONE staging buffer, as in pgps_gp_panel_gram_f64; [betas | sol | out] leave through ONE
    double *dts, *dV, *dys, *dres;
    TRY(stage_in(ctx, ctx->st[10], ts, N, &dts));
    TRY(stage_in<double>(ctx, ctx->st[4], nullptr, N * C + (rs ? N : 0), &dV));
    HIPCHK(ctx, hipMemcpyAsync(dV, V, N * C * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (rs) HIPCHK(ctx, hipMemcpyAsync(dV + N * C, rs, N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TRY(stage_in<double>(ctx, ctx->st[7], nullptr, N, &dys));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, nb + ns + no, &dres));
    const ProfileCall a{S, offs, nmodels, packed.data(), C, dts, dV, rs ? dV + N * C : nullptr, dres, dres + nb, dys, dres + nb + ns};
    TRY(profile_dev(ctx, d, a));
    // the results come back through a vector of the call: an error leaves the caller's outputs untouched
    std::vector<double> resh(nb + ns + no);
    TRY(stage_out(ctx, resh.data(), dres, nb + ns + no));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (nb) memcpy(betas, resh.data(), nb * sizeof(double));
    memcpy(sol, resh.data() + nb, ns * sizeof(double));
    memcpy(out, resh.data() + nb + ns, no * sizeof(double));
    // a series that was solved (status 0) must have finite log-likelihoods by both routes
    for (size_t s = 0; s < (size_t)S; ++s) {
        const double* q = sol + s * (p * p + 4);
        if (q[p * p + 3] == 0.0 && !(std::isfinite(q[p * p]) && std::isfinite(out[s * nout]))) return PGPS_E_NUMERIC;
    }
    return PGPS_OK;
}
