// pgps_panel_inst.hip -- one translation unit per state dimension d = 1, 2, 3 (fp64): the panel kernels (pgps_panel.hip.h:
// one workgroup per series, scalar and per-observation noise) and the launch function the C ABI dispatches to
// (pgps_panel_api.hip).  The d = 1 unit also holds the segmented merge, which knows nothing of d.
//
// launch_gp_panel lays a call out.  Series run in GROUPS: a group is one launch's grid.y (at most 65535 series) and holds as
// many consecutive series as fit the context's batch budget (pgps_set_batch_scratch; one series is the least a group can
// hold).  Everything a group needs besides the caller's arrays is carved from the context's scratch and reused by the next
// group on the same stream: the merged slots, the filtered moments (of the merged series; in the predictive checks, PANEL_LOO,
// of every series: no merge, no kept states), the scan records (ctx->ws), the kept states and the gradient partials (ctx->gadj).  A series' record does not depend on the group it lands in except through WHERE its slices
// lie, and no arithmetic does: results do not depend on the grouping.
#include <cstring>
#include <vector>

#include "pgps_merge.hip.h"
#include "pgps_panel.hip.h"
#include "pgps_panel_plan.h"
#include "pgps_scratch.h"

#ifndef PGPS_PANEL_D
#error "compile with -DPGPS_PANEL_D=<1|2|3>"
#endif

namespace pgps {

#if PGPS_PANEL_D == 1
// k_merge_sorted behind a per-series view: grid (tiles of the group's longest merged series, series).  Equal times follow
// merge_sorted_body's rule, decided per series from n >= k; a query row's slot is its GLOBAL position q0 + index, so the
// smoother's projection stores mean / var in place.
template <bool HET>
__global__ __launch_bounds__(kBlock) void k_panel_merge(const PanelArgs p) {
    const PanelDesc r = p.desc[blockIdx.y];
    // A series without queries needs no merge (its view reads the training rows), and the surplus workgroups of a series
    // shorter than the longest have no tile.  r and blockIdx are uniform: the WHOLE workgroup returns, before any barrier
    if (r.k == 0 || (long)blockIdx.x * kMergeTile >= (long)r.m) return;
    __shared__ MergeLds<double, HET> sh;
    merge_sorted_body<double, HET>(sh, (long)blockIdx.x, r.n, r.k, p.ts + r.row0, p.ys + r.row0, p.tq + r.q0, p.ts_m + r.m0,
                                   p.ys_m + r.m0, p.qslot + r.m0, r.q0, HET ? p.rs + r.row0 : nullptr,
                                   HET ? p.rs_m + r.m0 : nullptr);
}

int launch_panel_merge(pgps_ctx* ctx, const PanelArgs& p, unsigned tiles, unsigned series) {
    RoctxRange range_("merge_sorted");
    const dim3 grid(tiles, series), block(kBlock);
    if (p.rs) k_panel_merge<true><<<grid, block, 0, ctx->stream>>>(p);
    else k_panel_merge<false><<<grid, block, 0, ctx->stream>>>(p);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}
#endif

static inline size_t panel_pad(size_t n) { return align_up(n, (size_t)kPanelAlign); }
static_assert(kPanelLanes == kBlock, "panel_steps_per_lane counts the lanes of the panel's one workgroup");

template <int D>
struct PanelParts {
    Part<double> ts_m, ys_m, rs_m, fms, fPs, spine, lpre, sspine, lsuf, ll, lpd;
    Part<int> qslot;
    Part<double> xs, gpart;     // (in the second carver)
};

template <int D>
static PanelParts<D> panel_lay(Carver& cw, Carver& cg, const PanelTotals& t, bool het, bool loo) {
    constexpr int NST = gp_adj_nstat<D>();
    PanelParts<D> p;
    p.ts_m = cw.part<double>(t.merged); p.ys_m = cw.part<double>(t.merged); p.rs_m = cw.part<double>(het ? t.merged : 0);
    p.qslot = cw.part<int>(t.merged);
    p.fms = cw.part<double>(t.fm);      p.fPs = cw.part<double>(t.fP);
    p.spine = cw.part<double>(t.series * Dim<D>::NFILT);  p.lpre = cw.part<double>(t.series * kBlock * Dim<D>::NFILT);
    p.sspine = cw.part<double>(t.series * Dim<D>::NSMTH); p.lsuf = cw.part<double>(t.series * kBlock * Dim<D>::NSMTH);
    p.ll = cw.part<double>(t.series);
    p.lpd = cw.part<double>(loo ? t.series : 0);        // (the predictive checks' second partial; nothing elsewhere)
    p.xs = cg.part<double>(t.xs);       p.gpart = cg.part<double>(t.series * NST);
    return p;
}

// the records, and the groups they fall into: a record is closed into the current group unless the group's layout would then
// exceed the budget (or the grid)
template <int D>
void panel_plan(const pgps_ctx* ctx, const PanelCall& c, PanelWhat what, PanelPlan& plan) {
    constexpr int NX = D + Dim<D>::SYM;
    const bool het = c.rs != nullptr, predict = what == PANEL_PREDICT, grad = what == PANEL_GRAD, loo = what == PANEL_LOO;
    const size_t S = (size_t)c.S, budget = batch_budget_fused(ctx);
    std::vector<PanelDesc>& desc = plan.desc;
    std::vector<PanelGroup>& groups = plan.groups;
    desc.assign(S, PanelDesc{});
    groups.clear();
    size_t need_w = 0, need_g = 0;
    auto bytes_of = [&](const PanelTotals& t, size_t* w, size_t* g) {
        Carver cw(256), cg(256);
        panel_lay<D>(cw, cg, t, het, loo);
        *w = cw.bytes(); *g = cg.bytes();
    };
    for (size_t s = 0; s < S; ++s) {
        PanelDesc& r = desc[s];
        r.row0 = c.offs[s];
        r.n = (int)(c.offs[s + 1] - c.offs[s]);
        r.q0 = predict ? c.qoffs[s] : 0;
        r.k = predict ? (int)(c.qoffs[s + 1] - c.qoffs[s]) : 0;
        r.m = r.n + r.k;
        r.Lc = panel_steps_per_lane(r.m, ctx->chunk);
        r.model = c.nmodels == 1 ? 0 : (int)s;
        const size_t merged = r.k > 0 ? panel_pad((size_t)r.m) : 0;
        // the filtered moments the smoother reads back: of the merged series, and in the predictive checks of EVERY series
        const bool smooth = r.k > 0 || loo;
        const size_t fm = smooth ? panel_pad((size_t)r.m * D) : 0, fP = smooth ? panel_pad((size_t)r.m * D * D) : 0;
        const size_t xs = grad ? panel_pad((size_t)r.Lc * NX * kBlock) : 0;
        bool open = !groups.empty() && groups.back().t.series < kGridYMax;
        if (open) {
            PanelTotals t = groups.back().t;
            t.series += 1; t.merged += merged; t.fm += fm; t.fP += fP; t.xs += xs;
            size_t w, g;
            bytes_of(t, &w, &g);
            open = w + g <= budget;
        }
        if (!open) groups.push_back(PanelGroup{s, PanelTotals{}});
        PanelGroup& G = groups.back();
        r.slot = (int)G.t.series;
        r.m0 = (long)G.t.merged; r.o_fm = (long)G.t.fm; r.o_fP = (long)G.t.fP; r.o_xs = (long)G.t.xs;
        G.t.series += 1; G.t.merged += merged; G.t.fm += fm; G.t.fP += fP; G.t.xs += xs;
        if (r.k > 0) { G.queries = true; if (r.m > G.longest) G.longest = r.m; }
        size_t w, g;
        bytes_of(G.t, &w, &g);
        if (w > need_w) need_w = w;
        if (g > need_g) need_g = g;
    }
    plan.need_w = need_w; plan.need_g = need_g;
}

template <int D>
int panel_enqueue(pgps_ctx* ctx, const PanelCall& c, PanelWhat what, const PanelPlan& plan, const double* dmodels,
                  const PanelDesc* ddesc) {
    constexpr int NST = gp_adj_nstat<D>();
    const bool het = c.rs != nullptr, predict = what == PANEL_PREDICT, grad = what == PANEL_GRAD, loo = what == PANEL_LOO;
    const dim3 block(kBlock);
    for (const PanelGroup& G : plan.groups) {
        Carver cw(256), cg(256);
        const PanelParts<D> q = panel_lay<D>(cw, cg, G.t, het, loo);
        const Scratch s{(char*)ctx->ws.p}, sg{(char*)ctx->gadj.p};         // (sized by the caller for the largest group)
        PanelArgs p{};
        p.desc = ddesc + G.first;
        p.models = dmodels;
        p.ts = c.ts; p.ys = c.ys; p.rs = c.rs; p.tq = c.tq;
        p.ts_m = s(q.ts_m); p.ys_m = s(q.ys_m); p.rs_m = s(q.rs_m); p.qslot = s(q.qslot);
        p.pmean = c.mean; p.pvar = c.var;
        p.ll = c.ll ? c.ll + G.first : nullptr;
        p.out = c.out ? c.out + G.first * (size_t)(1 + NST) : nullptr;
        p.spine = s(q.spine); p.lpre = s(q.lpre); p.sspine = s(q.sspine); p.lsuf = s(q.lsuf); p.llpart = s(q.ll);
        p.fms = s(q.fms); p.fPs = s(q.fPs);
        p.xs = sg(q.xs); p.gpart = sg(q.gpart);
        p.status = ctx->status_word;
        const unsigned n = (unsigned)G.t.series;
        const dim3 grid(1, n);
        if (predict && G.queries)
            if (int rc = launch_panel_merge(ctx, p, (unsigned)((G.longest + kMergeTile - 1) / kMergeTile), n)) return rc;
        if (loo) {
            PanelLooArgs l{};
            l.p = p;
            l.o = GpLooOut<double>{c.osa_mean, c.osa_var, c.loo_mean, c.loo_var, s(q.lpd)};
            l.sums = c.sums + G.first * 2;
            if (het) timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_loo<D, true>, grid, block, 0, l);
            else timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_loo<D, false>, grid, block, 0, l);
        } else if (grad) {
            if (het) timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_gone<D, true>, grid, block, 0, p);
            else timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_gone<D, false>, grid, block, 0, p);
        } else if (predict) {
            if (het) timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_one<D, true, 2>, grid, block, 0, p);
            else timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_one<D, false, 2>, grid, block, 0, p);
        } else {
            if (het) timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_one<D, true, 0>, grid, block, 0, p);
            else timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_one<D, false, 0>, grid, block, 0, p);
        }
        HIPCHK(ctx, hipGetLastError());
    }
    return PGPS_OK;
}

// plan, both tables in ONE copy, [models | records], and the one synchronisation of the call (the host vectors die with it),
// then the launches
template <int D>
int launch_gp_panel(pgps_ctx* ctx, const PanelCall& c, PanelWhat what) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PanelPlan plan;
    panel_plan<D>(ctx, c, what, plan);
    const size_t S = (size_t)c.S;
    const size_t mbytes = align_up((size_t)c.nmodels * kGpModelStride * sizeof(double), 256);
    std::vector<char> tables(mbytes + S * sizeof(PanelDesc));
    memcpy(tables.data(), c.models, (size_t)c.nmodels * kGpModelStride * sizeof(double));
    memcpy(tables.data() + mbytes, plan.desc.data(), S * sizeof(PanelDesc));
    if (int rc = ensure(ctx, ctx->panel, tables.size())) return rc;
    if (int rc = ensure(ctx, ctx->ws, plan.need_w)) return rc;
    if (int rc = ensure(ctx, ctx->gadj, plan.need_g)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->panel.p, tables.data(), tables.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return panel_enqueue<D>(ctx, c, what, plan, reinterpret_cast<const double*>(ctx->panel.p),
                            reinterpret_cast<const PanelDesc*>((const char*)ctx->panel.p + mbytes));
}

template void panel_plan<PGPS_PANEL_D>(const pgps_ctx*, const PanelCall&, PanelWhat, PanelPlan&);
template int panel_enqueue<PGPS_PANEL_D>(pgps_ctx*, const PanelCall&, PanelWhat, const PanelPlan&, const double*, const PanelDesc*);
template int launch_gp_panel<PGPS_PANEL_D>(pgps_ctx*, const PanelCall&, PanelWhat);

}  // namespace pgps
