// pgps_panel_plan.h -- the panel's launch functions in two parts: a PLAN, made on the host from the
// call's offsets and the context's settings alone (the PanelDesc records, the groups they fall into, the scratch bytes of the
// largest group), and an ENQUEUE, which queues one launch per group on the context's stream against tables that already lie on
// the device and buffers that are already sized.  launch_gp_panel, launch_gp_panel_gram and launch_panel_residual are
// plan + ONE table copy + ONE stream synchronisation + enqueue, as before; a call that chains several phases
// (pgps_gp_panel_profile_grad_*, pgps_panel_trend_api.hip) plans them all, lays ONE table out, sizes every buffer for the
// largest phase, copies and synchronises once, and only then enqueues -- no ensure() can move a buffer under a queued kernel.
// Included by the panel's kernel units and by the host unit of the chained call; nothing here is device code.
#pragma once

#include <vector>

#include "pgps_internal.h"

namespace pgps {

// what a group of series needs in launch_gp_panel's scratch: counts of elements, every ragged slice padded to kPanelAlign
struct PanelTotals {
    size_t series = 0, merged = 0, fm = 0, fP = 0, xs = 0;
};
struct PanelGroup {
    size_t first;               // its first series
    PanelTotals t;
    int longest = 0;            // the longest merged series with queries (the merge's grid)
    bool queries = false;
};
struct PanelPlan {
    std::vector<PanelDesc> desc;        // (S,)
    std::vector<PanelGroup> groups;
    size_t need_w = 0, need_g = 0;      // bytes of ctx->ws / ctx->gadj the largest group takes
};
// c.S, c.offs, c.qoffs, c.nmodels, c.rs (null or not) and `what` decide the plan; the context gives the chunk and the budget
template <int D>
void panel_plan(const pgps_ctx* ctx, const PanelCall& c, PanelWhat what, PanelPlan& plan);
// one launch per group (predict: the merge before it).  dmodels (nmodels, kGpModelStride) and ddesc (S,) [device] hold what the
// plan was copied to; ctx->ws and ctx->gadj hold at least plan.need_w / need_g bytes.  Queues, does not synchronise
template <int D>
int panel_enqueue(pgps_ctx* ctx, const PanelCall& c, PanelWhat what, const PanelPlan& plan, const double* dmodels,
                  const PanelDesc* ddesc);

struct PanelGramGroup { size_t first, series, w; };
struct PanelGramPlan {
    std::vector<PanelDesc> desc;
    std::vector<PanelGramGroup> groups;
    size_t need_w = 0;                  // bytes of ctx->ws
};
// (the plan knows nothing of d: the d = 1 unit holds it)
void panel_gram_plan(const pgps_ctx* ctx, const PanelGramCall& c, PanelGramPlan& plan);
template <int D>
int panel_gram_enqueue(pgps_ctx* ctx, const PanelGramCall& c, const PanelGramPlan& plan, const double* dmodels,
                       const PanelDesc* ddesc);

// the residual kernel over offs [host] / doffs [device, the same S + 1 values]: one launch per kGridYMax series
int panel_residual_enqueue(pgps_ctx* ctx, long S, const long* offs, const long* doffs, int C, const double* V, const double* betas,
                           double* ys_out);

// k_panel_trend_solve (pgps_panel_trend.hip.h): records (S, C C + 2), betas (S, C - 1), sol (S, (C-1)^2 + 4) [device]; one launch,
// no tables, no synchronisation
int launch_panel_trend_solve(pgps_ctx* ctx, long S, int C, const double* records, double* betas, double* sol);

}  // namespace pgps
