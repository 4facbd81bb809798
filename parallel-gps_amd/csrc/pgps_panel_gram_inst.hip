// pgps_panel_gram_inst.hip -- one translation unit per state dimension d = 1, 2, 3 (fp64): the panel's Gram kernel
// (pgps_panel_gram.hip.h: one workgroup per series, scalar and per-observation noise) and the launch function the C ABI
// dispatches to (pgps_panel_gram_api.hip).  The d = 1 unit also holds the residual kernel and
// the plan of a call (pgps_panel_plan.h), which know nothing of d.
//
// launch_gp_panel_gram lays a call out as launch_gp_panel does (pgps_panel_inst.hip): series run in GROUPS of consecutive series,
// one launch's grid.y each (at most 65535), as many as fit the context's batch budget (pgps_set_batch_scratch; one series is the
// least a group can hold).  All a group needs besides the caller's arrays is the whitened columns W: one ragged slice (n, C)
// per series, padded to kPanelAlign, carved from ctx->ws and reused by the next group on the same stream.  The scan's lane
// prefixes stay in registers (one workgroup per series: nothing is handed over through memory).  A record does not depend on
// the group its series lands in except through WHERE its slice lies.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pgps_panel_gram.hip.h"
#include "pgps_panel_plan.h"
#include "pgps_scratch.h"

#ifndef PGPS_PANEL_GRAM_D
#error "compile with -DPGPS_PANEL_GRAM_D=<1|2|3>"
#endif

namespace pgps {

static inline size_t panel_pad(size_t n) { return align_up(n, (size_t)kPanelAlign); }

// a group's scratch: the W slices of its series, back to back
static Part<double> panel_gram_lay(Carver& cw, size_t w_elems) { return cw.part<double>(w_elems); }

#if PGPS_PANEL_GRAM_D == 1
int panel_residual_enqueue(pgps_ctx* ctx, long S, const long* offs, const long* doffs, int C, const double* V, const double* betas,
                           double* ys_out) {
    for (size_t first = 0; first < (size_t)S; first += kGridYMax) {
        const size_t n = std::min((size_t)S - first, kGridYMax);
        long longest = 1;
        for (size_t s = first; s < first + n; ++s) longest = std::max(longest, offs[s + 1] - offs[s]);
        const dim3 grid((unsigned)((longest + kBlock - 1) / kBlock), (unsigned)n), block(kBlock);
        k_panel_residual<<<grid, block, 0, ctx->stream>>>(doffs + first, C, V, betas + first * (size_t)(C - 1), ys_out);
        HIPCHK(ctx, hipGetLastError());
    }
    return PGPS_OK;
}

int launch_panel_residual(pgps_ctx* ctx, long S, const long* offs, int C, const double* V, const double* betas, double* ys_out) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the offsets go up through the panel's table buffer: ONE copy and the one synchronisation of the call
    const size_t bytes = ((size_t)S + 1) * sizeof(long);
    if (int rc = ensure(ctx, ctx->panel, bytes)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->panel.p, offs, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return panel_residual_enqueue(ctx, S, offs, reinterpret_cast<const long*>(ctx->panel.p), C, V, betas, ys_out);
}

void panel_gram_plan(const pgps_ctx* ctx, const PanelGramCall& c, PanelGramPlan& plan) {
    const size_t S = (size_t)c.S, budget = batch_budget_fused(ctx);
    std::vector<PanelDesc>& desc = plan.desc;
    std::vector<PanelGramGroup>& groups = plan.groups;
    desc.assign(S, PanelDesc{});
    groups.clear();
    size_t need_w = 0;
    auto bytes_of = [&](size_t w) {
        Carver cw(256);
        panel_gram_lay(cw, w);
        return cw.bytes();
    };
    for (size_t s = 0; s < S; ++s) {
        PanelDesc& r = desc[s];
        r.row0 = c.offs[s];
        r.n = (int)(c.offs[s + 1] - c.offs[s]);
        r.m = r.n;
        r.Lc = panel_steps_per_lane(r.n, ctx->chunk);
        r.model = c.nmodels == 1 ? 0 : (int)s;
        const size_t w = panel_pad((size_t)r.n * (size_t)c.C);
        const bool open = !groups.empty() && groups.back().series < kGridYMax && bytes_of(groups.back().w + w) <= budget;
        if (!open) groups.push_back(PanelGramGroup{s, 0, 0});
        PanelGramGroup& G = groups.back();
        r.slot = (int)G.series;
        r.o_fm = (long)G.w;
        G.series += 1; G.w += w;
        need_w = std::max(need_w, bytes_of(G.w));
    }
    plan.need_w = need_w;
}
#endif

template <int D>
int panel_gram_enqueue(pgps_ctx* ctx, const PanelGramCall& c, const PanelGramPlan& plan, const double* dmodels,
                       const PanelDesc* ddesc) {
    const dim3 block(kBlock);
    const size_t rec = (size_t)c.C * c.C + 2;
    for (const PanelGramGroup& G : plan.groups) {
        Carver cw(256);
        const Part<double> pw = panel_gram_lay(cw, G.w);
        const Scratch s{(char*)ctx->ws.p};              // (sized by the caller for the largest group)
        PanelGramArgs p{};
        p.desc = ddesc + G.first;
        p.models = dmodels;
        p.ts = c.ts; p.V = c.V; p.rs = c.rs; p.C = c.C;
        p.w = s(pw);
        p.out = c.out + G.first * rec;
        const dim3 grid(1, (unsigned)G.series);
        if (c.rs) timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_gram<D, true>, grid, block, 0, p);
        else timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_gram<D, false>, grid, block, 0, p);
        HIPCHK(ctx, hipGetLastError());
    }
    return PGPS_OK;
}

// plan, both tables in ONE copy, [models | records], and the one synchronisation of the call (the host vectors die with it),
// then the launches
template <int D>
int launch_gp_panel_gram(pgps_ctx* ctx, const PanelGramCall& c) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PanelGramPlan plan;
    panel_gram_plan(ctx, c, plan);
    const size_t S = (size_t)c.S;
    const size_t mbytes = align_up((size_t)c.nmodels * kGpModelStride * sizeof(double), 256);
    std::vector<char> tables(mbytes + S * sizeof(PanelDesc));
    memcpy(tables.data(), c.models, (size_t)c.nmodels * kGpModelStride * sizeof(double));
    memcpy(tables.data() + mbytes, plan.desc.data(), S * sizeof(PanelDesc));
    if (int rc = ensure(ctx, ctx->panel, tables.size())) return rc;
    if (int rc = ensure(ctx, ctx->ws, plan.need_w)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->panel.p, tables.data(), tables.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return panel_gram_enqueue<D>(ctx, c, plan, reinterpret_cast<const double*>(ctx->panel.p),
                                 reinterpret_cast<const PanelDesc*>((const char*)ctx->panel.p + mbytes));
}

template int panel_gram_enqueue<PGPS_PANEL_GRAM_D>(pgps_ctx*, const PanelGramCall&, const PanelGramPlan&, const double*, const PanelDesc*);
template int launch_gp_panel_gram<PGPS_PANEL_GRAM_D>(pgps_ctx*, const PanelGramCall&);

}  // namespace pgps
