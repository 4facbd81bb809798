// pgps_panel_fit.h -- what pgps_panel_fit_api.hip and pgps_panel_fit_inst.hip share: a call of pgps_gp_panel_fit_* as the C ABI
// hands it over, and the launch function (fp64, d <= 3).
#pragma once

#include "pgps_fit.h"
#include "pgps_internal.h"

namespace pgps {

// The start record of one series: the host fills it (pgps_panel_fit_api.hip), the kernel reads it (pgps_panel_fit.hip.h), both by
// these offsets.  x = log theta and theta itself; a coordinate that is not free has x0 = log lo = log hi = 0 and lo = hi = theta0
constexpr int kFitRecX0 = 0;                    // log theta0 (kFitP)
constexpr int kFitRecXlo = kFitP;               // log lo
constexpr int kFitRecXhi = 2 * kFitP;           // log hi
constexpr int kFitRecTheta0 = 3 * kFitP;        // theta0
constexpr int kFitRecLo = 4 * kFitP;            // lo
constexpr int kFitRecHi = 5 * kFitP;            // hi
constexpr int kFitRecord = 6 * kFitP;           // doubles of a record

// offs / unit / records HOST, everything else device
struct PanelFitCall {
    long S;
    const long* offs;           // (S + 1)
    const double* unit;         // (kGpModelStride): the unit model row
    const double* records;      // (S, kFitRecord) start records
    const double *ts, *ys, *rs; // concatenated series (rs: null = scalar noise)
    int free_[3];
    double gtol;
    int max_iter;
    double* thetas;             // (S, 3)
    double* info;               // (S, 8)
};
// lays the series out in groups that fit the context's batch budget (the rule and the layout of the Laplace panel's gradient,
// pgps_panel_site_lay.h), copies the three tables in (ONE stream synchronisation), then one launch of k_gpp_fit per group.
// The caller has checked the arguments
template <int D>
int launch_gp_panel_fit(pgps_ctx* ctx, const PanelFitCall& c);

}  // namespace pgps
