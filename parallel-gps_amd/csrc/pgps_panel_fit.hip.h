// pgps_panel_fit.hip.h -- the hyper-parameter fit of S series in ONE launch.
//
// StateSpaceGPPanel.log_likelihoods_and_grads is one evaluation; a fit of every series' own variance, lengthscale and noise
// variance driven from the host pays a launch, a table and a contraction per evaluation.  Here the optimiser's control flow
// lives in the kernel, as the Newton search of a Laplace approximation does in k_gpp_newton (pgps_panel_site.hip.h):
// k_gpp_fit gives every series of a panel one workgroup (grid (1, series of the group), as k_gpp_gone), and the workgroup runs
// fit_search (pgps_fit.h: projected BFGS with a backtracking Armijo search over x = log theta) to the end -- its own iteration
// count, its own halvings -- before anything comes back.
//
//   eval     model    theta from x (fit_theta; a coordinate that is not free keeps its given theta), then the fused model of
//                     the Matern kernel in registers (fit_matern_model, pgps_fit_model.h; Matern-5/2 from the unit row the
//                     host passed).  Every lane computes the same row from the same x; nothing is stored, the model table
//                     of PanelArgs holds the unit row alone
//            passes   gp_reduce_body<HET>, gp_gfwd_body<HET>, gp_gback_body<HET> -- the three bodies of k_gpp_gone -- back to
//                     back behind the view of gp_panel_select, on the series' own scratch slot, which every evaluation reuses
//            sums     ll = llpart[0] and the adjoints [Abar | Ubar | Hbar | Rbar] = gpart[0 ..] (nblocks = 1: the workgroup's
//                     partials are the series' totals), contracted by fit_contract into f = -ll / max(1, n_obs) and g
//
// What k_gpp_newton keeps, kept here:
// Uniformity.  Every decision is a function of sums that every lane holds with the same bits: block_sum_double returns the
// one LDS total to all lanes, and the passes' totals are read by every lane from the series' own partial slots (site_word: a
// vector load) behind wg_sync.  No lane decides from a partial of its own; there is no return inside the loop.
// Bounds.  No spin wait, no other workgroup is met.  fit_search ends after at most 1 + 2 (kFitMaxHalvings + 1) max_iter
// evaluations whatever the data; the entry point caps max_iter at kFitMaxIterCap.
// Visibility.  lpre, lsuf, spine, sspine, xs, llpart and gpart are written by vector stores and read by other lanes of the SAME
// workgroup later in the launch: one CU, one vector L1, stores drained by s_waitcnt vmcnt(0) before the barrier (wg_sync).
// None of them takes a non-temporal store or a scalar load; only what the host wrote before the launch -- the descriptor, the
// unit row, the series' start record -- may go through the scalar path, and it is read before the first store.
// Look-ahead.  Row n of a view is the neighbour's (pgps_panel.hip.h lists the bodies' guards): gp_reduce_body and gp_gfwd_body
// read ts / ys / rs[k + 1] only where k + 1 < k1 <= N, gp_gback_body ts[k - 1] only where k > 0.  The count of observed rows
// runs k < n.
// A row's bits depend on that series alone: its steps per lane, its scratch slot and its start record are its own.
#pragma once

#include "pgps_fit.h"
#include "pgps_fit_model.h"
#include "pgps_panel.hip.h"
#include "pgps_panel_fit.h"

namespace pgps {

// (the start record of one series, host-made and read-only in the launch: kFitRec* of pgps_panel_fit.h)

// what one launch of k_gpp_fit (one group of series) sees.  PanelDesc is read as the gradient call fills it (k = 0, m = n)
struct PanelFitArgs {
    PanelArgs p;                // desc, models = the unit row, ts, ys, rs, the scan records, xs, gpart, status; nothing else is set
    const double* records;      // (the group's series, kFitRecord)
    int free_[kFitP];
    double gtol;
    int max_iter;
    double* thetas;             // (the group's series, kFitP)
    double* info;               // (the group's series, kFitInfo)
};

// the one operation of fit_search on one series' scratch slot
template <int D, bool HET>
struct PanelFitOps {
    GpAdjArgs ga;                   // the series' view, built ONCE before any store of the launch
    GpLds<double, D>* sh;
    const double* rs;
    FitModel unit;                  // the Matern-5/2 unit form (D = 3)
    double rec[kFitRecord];
    int free_[kFitP];
    double n_obs;

    __device__ __forceinline__ void thetas_of(const double x[kFitP], double th[kFitP]) const {
#pragma unroll
        for (int i = 0; i < kFitP; ++i)
            th[i] = free_[i] ? fit_theta(x[i], rec[kFitRecX0 + i], rec[kFitRecXlo + i], rec[kFitRecXhi + i], rec[kFitRecTheta0 + i],
                                         rec[kFitRecLo + i], rec[kFitRecHi + i])
                             : rec[kFitRecTheta0 + i];
    }

    __device__ __forceinline__ void eval(const double x[kFitP], double* f, double g[kFitP]) {
        constexpr int NST = gp_adj_nstat<D>();
        double th[kFitP];
        thetas_of(x, th);
        FitModel m;
        fit_matern_model<D>(th[0], th[1], unit, m);
        ga.g.m.lam = m.lam;
#pragma unroll
        for (int i = 0; i < D * D; ++i) { ga.g.m.N1[i] = m.N1[i]; ga.g.m.N2[i] = m.N2[i]; ga.g.m.Pinf[i] = m.Pinf[i]; }
#pragma unroll
        for (int i = 0; i < D; ++i) ga.g.m.H[i] = m.H[i];
        ga.g.s.R = th[2];
        // The series' length, steps per lane and bases pass through an empty asm in every evaluation (as PanelNewtonOps::pass
        // does): to the compiler they are new values each time, so the lanes' index and address arithmetic of the three bodies
        // is redone per evaluation instead of being hoisted out of the search loops, where it would be live through every body
        int lc = ga.g.s.Lc;
        long len = ga.g.s.N;
        asm volatile("" : "+s"(lc), "+s"(len));
        ga.g.s.Lc = lc;
        ga.g.s.N = len;
        asm volatile("" : "+s"(ga.g.s.lpre), "+s"(ga.g.s.lsuf), "+s"(ga.g.s.spine), "+s"(ga.g.s.sspine), "+s"(ga.g.s.llpart));
        asm volatile("" : "+s"(ga.g.s.ys), "+s"(ga.g.m.ts), "+s"(rs), "+s"(ga.xs), "+s"(ga.gpart), "+s"(ga.g.s.status));
        gp_reduce_body<double, D, HET>(ga.g, sh->lds, rs);
        wg_sync();
        gp_gfwd_body<D, HET>(ga, *sh, rs);
        wg_sync();
        gp_gback_body<D, HET>(ga, *sh, rs);
        wg_sync();
        const double ll = site_word(ga.g.s.llpart);
        double stats[NST];
#pragma unroll
        for (int i = 0; i < NST; ++i) stats[i] = site_word(ga.gpart + i);
        double gv[kFitP];
        fit_contract<D>(m, th, free_, n_obs, ll, stats, f, gv);
        *f = uniform_word(*f);
#pragma unroll
        for (int i = 0; i < kFitP; ++i) g[i] = uniform_word(gv[i]);
    }
};

template <int D, bool HET>
__global__ __launch_bounds__(kBlock) void k_gpp_fit(const PanelFitArgs a) {
    constexpr int NST = gp_adj_nstat<D>();
    __shared__ GpLds<double, D> sh;
    const PanelDesc r = a.p.desc[blockIdx.y];
    PanelFitOps<D, HET> o;
    o.ga = GpAdjArgs{};
    o.ga.g = gp_panel_select<D, HET>(a.p, r, false, &o.rs);
    o.ga.g.s.ll = nullptr;                      // (the totals are read from the series' own slots)
    o.ga.xs = a.p.xs + r.o_xs;
    o.ga.gpart = a.p.gpart + (long)r.slot * NST;
    o.sh = &sh;
    // the unit row came through the view (gp_panel_select reads the table's row r.model = 0)
    o.unit.lam = o.ga.g.m.lam;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        o.unit.N1[i] = i < D * D ? o.ga.g.m.N1[i] : 0.0;
        o.unit.N2[i] = i < D * D ? o.ga.g.m.N2[i] : 0.0;
        o.unit.Pinf[i] = i < D * D ? o.ga.g.m.Pinf[i] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) o.unit.H[i] = i < D ? o.ga.g.m.H[i] : 0.0;
    const double* rec = a.records + (long)blockIdx.y * kFitRecord;
#pragma unroll
    for (int i = 0; i < kFitRecord; ++i) o.rec[i] = rec[i];
#pragma unroll
    for (int i = 0; i < kFitP; ++i) o.free_[i] = a.free_[i];

    // the observed rows of the series: the scale of f
    double cnt = 0.0;
    for (int k = threadIdx.x; k < r.n; k += kBlock) cnt += is_nan(o.ga.g.s.ys[k]) ? 0.0 : 1.0;
    o.n_obs = uniform_word(block_sum_double(cnt, sh.lds_ll));

    FitResult res;
    fit_search(o, o.rec + kFitRecX0, o.rec + kFitRecXlo, o.rec + kFitRecXhi, o.free_, a.gtol, a.max_iter, res);

    if (threadIdx.x == 0) {
        double th[kFitP];
        o.thetas_of(res.x, th);
        double* t = a.thetas + (long)blockIdx.y * kFitP;
#pragma unroll
        for (int i = 0; i < kFitP; ++i) t[i] = th[i];
        const double scale = o.n_obs > 1.0 ? o.n_obs : 1.0;
        double* w = a.info + (long)blockIdx.y * kFitInfo;
        w[0] = -res.f * scale; w[1] = -res.f0 * scale; w[2] = (double)res.iterations; w[3] = (double)res.evaluations;
        w[4] = (double)res.status; w[5] = res.gnorm; w[6] = o.n_obs; w[7] = 0.0;
    }
}

}  // namespace pgps
