// pgps_panel_site.h -- what pgps_panel_site_api.hip and pgps_panel_site_inst.hip share: a call of pgps_gp_panel_laplace_* as the
// C ABI hands it over, and the launch functions (fp64, d <= 3).
#pragma once

#include "pgps_internal.h"

namespace pgps {

// offs / models / pars HOST, everything else device
struct PanelSiteCall {
    long S;
    const long* offs;           // (S + 1)
    int nmodels;                // 1 or S
    const double* models;       // (nmodels, kGpModelStride), column 31 (R) = 0
    int lik;                    // PGPS_LIK_*
    int npars;                  // 1 or S
    const double* pars;         // (npars,)
    const double *ts, *ys;      // concatenated series
    double tol;
    int max_iter;
    double *f, *v, *zs, *ss;    // (offs[S],): outputs of the search, inputs of the gradient
    double* info;               // (S, 8): the search
    double* out;                // (S, 1 + d^2 + 2 d + 1): the gradient
};
// lays the series out in groups that fit the context's batch budget, copies the three tables in (ONE stream synchronisation),
// then one launch of k_gpp_newton per group.  The caller has checked the arguments
template <int D>
int launch_gp_panel_laplace(pgps_ctx* ctx, const PanelSiteCall& c);
// ... the gradient's inputs, three launches of k_gpp_gone<D, true> per group and one combination
template <int D>
int launch_gp_panel_laplace_grad(pgps_ctx* ctx, const PanelSiteCall& c);

}  // namespace pgps
