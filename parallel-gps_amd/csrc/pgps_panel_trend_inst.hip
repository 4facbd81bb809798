// pgps_panel_trend_inst.hip -- the one translation unit of the panel's GLS solve kernel (pgps_panel_trend.hip.h: one lane per
// series; it knows nothing of the state dimension) and its launch function (pgps_panel_plan.h), which the C ABI dispatches to
// (pgps_panel_trend_api.hip).  One launch over ceil(S / kBlock) workgroups; no table goes up and nothing is synchronised: the
// records, betas and sol are device arrays of the caller.
#include "pgps_panel_trend.hip.h"
#include "pgps_panel_plan.h"

namespace pgps {

int launch_panel_trend_solve(pgps_ctx* ctx, long S, int C, const double* records, double* betas, double* sol) {
    const dim3 grid((unsigned)((S + kBlock - 1) / kBlock)), block(kBlock);
    k_panel_trend_solve<<<grid, block, 0, ctx->stream>>>(S, C, records, betas, sol);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

}  // namespace pgps
