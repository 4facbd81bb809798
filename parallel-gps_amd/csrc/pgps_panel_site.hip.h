// pgps_panel_site.hip.h -- the mode search of a Laplace approximation for S series in ONE launch.
//
// LaplaceStateSpaceGP runs its damped Newton search from the host: four launches per step, six doubles back, a host decision.
// At the series lengths of a panel (10^2 .. 10^3 rows) that is all launch latency and round trip.  Here the search's control
// flow lives in the kernel: k_gpp_newton gives every series of a panel one workgroup (grid (1, series of the group), as
// k_gpp_one), and the workgroup runs newton_search (pgps_newton.h: the rule of LaplaceStateSpaceGP._search) to the end -- its
// own iteration count, its own halvings -- before anything comes back.
//
//   start    the sites at f = 0, alpha = 0: lik_site elementwise over the series' rows, lanes strided; Psi = lp - f alpha / 2
//   pass     gp_reduce_body<HET>, gp_apply_body<SMOOTH, HET>, gp_smooth_body<SITE> -- the three bodies launch_gp_newton
//            launches -- back to back behind the view of gp_panel_select with ys = zs, rs = ss, R = 0; nblocks = 1, so the
//            SITE epilogue's partials and llpart[0] are the series' totals
//   halve    the elementwise update of k_lik_sites on the segment between iterate and proposal (in place in the proposal)
//   accept   a swap of the iterate's and the proposal's pointers
//
// Uniformity.  Every loop and branch of the search contains workgroup barriers.  The decisions are functions of the sums
// alone, and every lane holds the SAME sums: block_sum_double returns the one LDS total to all lanes, and the pass's totals
// are read by every lane from the series' own partial slot (site_word: a vector load) behind wg_sync.  No lane decides from a
// partial of its own; there is no return inside the loop.
// Bounds.  No spin wait, no other workgroup is met.  newton_search ends after at most max_iter + 1 passes and
// kNewtonMaxHalvings max_iter damped updates whatever the data; the entry point caps max_iter at kNewtonMaxIterCap.
// Visibility.  zs, ss, f, alpha, v, fms, fPs, lpre, lsuf and the partials are written by vector stores and read by other lanes
// of the SAME workgroup later in the launch: one CU, one vector L1, stores drained by s_waitcnt vmcnt(0) before the barrier
// (wg_sync, what k_gp_one / k_gpp_one rely on between their bodies).  None of them takes a non-temporal store (NT = false) or
// a scalar load; only the read-only model row and the descriptor may go through the scalar path.
// Look-ahead.  Row n of a view is the neighbour's (pgps_panel.hip.h lists the bodies' guards).  The SITE reads of the smoother,
// so.ss / so.ys / so.f_prev, are [k1 - 1] under k0 < k1 <= N and [k - 1] under k > k0: inside [k0, k1).  The elementwise loops
// run k < n.
#pragma once

#include "pgps_newton.h"
#include "pgps_panel.hip.h"
#include "pgps_panel_site_lay.h"

namespace pgps {

static_assert(kSiteAlign == kPanelAlign && kSiteLanes == kBlock && kSitePartials == kSiteParts, "pgps_panel_site_lay.h restates them");

// what one launch of k_gpp_newton (one group of series) sees.  PanelDesc is read as the panel's own calls fill it, with
// k = 0, m = n and m0 = the element offset of the series' per-row arrays in `rows`
struct PanelSiteArgs {
    PanelArgs p;                // desc, models (R ignored), ts, ys, the scan records, fms / fPs, status; nothing else is set
    int lik;
    const double* pars;         // the parameter of the group's first series
    int par_stride;             // 0: one parameter shared by all series, 1: one per series
    double tol;
    int max_iter;
    double* rows;               // the group's per-row arrays (kSiteRowArrays slices of site_pad(n) per series)
    double* part;               // (series, kSiteParts)
    double *f, *v, *zs, *ss;    // (rows of the call,) outputs
    double* info;               // (the group's series, kSiteInfo)
};

// (wg_sync, uniform_word, site_word: pgps_panel.hip.h)

// the four operations of newton_search on one series' slices
template <int D>
struct PanelNewtonOps {
    GpArgs<double> g;               // the series' view, built ONCE before any store of the launch: the model row and the
                                    // descriptor are read-only and come through the scalar path, nothing else does
    GpLds<double, D>* sh;
    int lik;
    double par;
    const double* ys;
    int n;
    double *cf, *ca, *cz, *cs;      // the iterate and the sites formed at it
    double *pf, *pa, *pz, *ps;      // the proposal
    double* v;
    double* part;

    // the sites at 0 (into the iterate) or at the midpoint of iterate and proposal (into the proposal, in place)
    __device__ __forceinline__ void sites(bool at_zero, double s[3]) {
        double lp = 0.0, fa = 0.0, corr = 0.0;
        double *fo = at_zero ? cf : pf, *ao = at_zero ? ca : pa, *zo = at_zero ? cz : pz, *so = at_zero ? cs : ps;
        for (int k = threadIdx.x; k < n; k += kBlock) {
            double f = 0.0, al = 0.0;
            if (!at_zero) {
                f = cf[k]; al = ca[k];
                f += 0.5 * (pf[k] - f);
                al += 0.5 * (pa[k] - al);
            }
            const double y = ys[k];
            double z_new = y, s_new = 1.0;              // (y is NaN at a missing row)
            if (!is_nan(y)) {
                const LikSite ls = lik_site(lik, par, y, f);
                z_new = ls.z;
                s_new = ls.s;
                lp += ls.lp;
                corr += ls.corr;
            }
            fa += f * al;
            fo[k] = f; ao[k] = al; zo[k] = z_new; so[k] = s_new;
        }
        s[0] = uniform_word(block_sum_double(lp, sh->lds_ll));
        s[1] = uniform_word(block_sum_double(fa, sh->lds_ll));
        s[2] = uniform_word(block_sum_double(corr, sh->lds_ll));
        wg_sync();
    }
    __device__ __forceinline__ void start(double s[3]) { sites(true, s); }
    __device__ __forceinline__ void halve(double s[3]) { sites(false, s); }

    // The series' length and steps per lane pass through an empty asm in every pass: to the compiler they are new values each
    // time, so the lanes' index and address arithmetic of the three bodies is redone per pass (a few dozen integer
    // instructions) instead of being hoisted out of the search loop, where it would be live -- a register pair per address --
    // through every body and spill
    __device__ __forceinline__ void pass(double s[6]) {
        int lc = g.s.Lc, len = n;
        asm volatile("" : "+s"(lc), "+s"(len));
        g.s.Lc = lc;
        g.s.N = len;
        // ... and so do the bases of the scratch and the model row: the lanes' addresses and the vector-register copies the
        // bodies make of the model are made per pass
        asm volatile("" : "+s"(g.s.lpre), "+s"(g.s.lsuf), "+s"(g.s.spine), "+s"(g.s.sspine), "+s"(g.s.llpart));
        asm volatile("" : "+s"(g.s.fms), "+s"(g.s.fPs), "+s"(g.m.ts), "+s"(g.m.t_prev), "+s"(ys), "+s"(v), "+s"(part));
        asm volatile("" : "+s"(g.m.lam), "+s"(par), "+s"(lik), "+s"(g.s.status));
#pragma unroll
        for (int i = 0; i < D * D; ++i) asm volatile("" : "+s"(g.m.N1[i]), "+s"(g.m.N2[i]), "+s"(g.m.Pinf[i]));
#pragma unroll
        for (int i = 0; i < D; ++i) asm volatile("" : "+s"(g.m.H[i]));
        g.s.ys = cz;
        const GpSiteOut<double> so{lik, par, ys, cs, cf, pf, v, pa, pz, ps, part};
        gp_reduce_body<double, D, true>(g, sh->lds, cs);
        wg_sync();
        gp_apply_body<double, D, true, false, true>(g, *sh, cs);
        wg_sync();
        gp_smooth_body<double, D, false, false, false, true>(g, *sh, GpLooOut<double>{}, so);
        wg_sync();
        s[0] = site_word(g.s.llpart);
#pragma unroll
        for (int i = 0; i < kSiteParts; ++i) s[1 + i] = site_word(part + i);      // lp | f alpha | corr | move | observed rows
    }

    __device__ __forceinline__ void accept() {
        double* t;
        t = cf; cf = pf; pf = t;
        t = ca; ca = pa; pa = t;
        t = cz; cz = pz; pz = t;
        t = cs; cs = ps; ps = t;
    }
};

template <int D>
__global__ __launch_bounds__(kBlock) void k_gpp_newton(const PanelSiteArgs a) {
    __shared__ GpLds<double, D> sh;
    const PanelDesc r = a.p.desc[blockIdx.y];
    const double* unused;
    PanelNewtonOps<D> o;
    o.g = gp_panel_select<D, false>(a.p, r, false, &unused);
    o.g.s.R = 0.0;                              // (the sites carry all the noise; column 31 of the table is ignored)
    o.g.s.ll = nullptr;                         // (the totals are read from the series' own slots)
    o.g.s.fms = a.p.fms + r.o_fm;
    o.g.s.fPs = a.p.fPs + r.o_fP;
    o.sh = &sh;
    o.lik = a.lik;
    o.par = a.pars[(long)a.par_stride * blockIdx.y];
    o.ys = a.p.ys + r.row0;
    o.n = r.n;
    const long pad = (long)((r.n + kPanelAlign - 1) / kPanelAlign) * kPanelAlign;
    double* base = a.rows + r.m0;
    o.cf = base;           o.ca = base + pad;     o.cz = base + 2 * pad; o.cs = base + 3 * pad;
    o.pf = base + 4 * pad; o.pa = base + 5 * pad; o.pz = base + 6 * pad; o.ps = base + 7 * pad;
    o.v = base + 8 * pad;
    o.part = a.part + (long)r.slot * kSiteParts;

    NewtonResult res;
    newton_search(o, a.tol, a.max_iter, res);

    // the accepted iterate with its sites, and the variances of the last pass (every operation ended in wg_sync)
    for (int k = threadIdx.x; k < r.n; k += kBlock) {
        a.f[r.row0 + k] = o.cf[k];
        a.v[r.row0 + k] = o.v[k];
        a.zs[r.row0 + k] = o.cz[k];
        a.ss[r.row0 + k] = o.cs[k];
    }
    if (threadIdx.x == 0) {
        double* w = a.info + (long)blockIdx.y * kSiteInfo;
        w[0] = res.ll_sites; w[1] = res.corr; w[2] = res.psi; w[3] = (double)res.iterations;
        w[4] = (double)res.halvings; w[5] = (double)res.converged; w[6] = res.move; w[7] = res.n_obs;
    }
}

// The observation arrays of the gradient's identity  grad log q = grad [G(z + w) - G(w) + G(0)],  w = v d3 / (2 W)  at the
// mode, elementwise over the rows of the group's series (NaN at the missing rows): x1 = z + w, x2 = w, x3 = 0
struct PanelSiteGradArgs {
    const PanelDesc* desc;
    int lik;
    const double* pars;
    int par_stride;
    const double *ys, *f, *v, *zs;
    double *x1, *x2, *x3;
};
static __global__ __launch_bounds__(kBlock) void k_gpp_grad_inputs(const PanelSiteGradArgs a) {
    const PanelDesc r = a.desc[blockIdx.y];
    const double par = a.pars[(long)a.par_stride * blockIdx.y];
    for (int k = threadIdx.x; k < r.n; k += kBlock) {
        const long i = r.row0 + k;
        const double y = a.ys[i];
        double x1 = y, x2 = y, x3 = y;                  // (NaN)
        if (!is_nan(y)) {
            double lp, g, W, d3;
            lik_eval(a.lik, par, y, a.f[i], lp, g, W, d3);
            const double w = 0.5 * a.v[i] * d3 / W;
            x1 = a.zs[i] + w;
            x2 = w;
            x3 = 0.0;
        }
        a.x1[i] = x1; a.x2[i] = x2; a.x3[i] = x3;
    }
}

// out = (a - b) + c, elementwise: the three adjoint rows of every series combined as the host combines them
static __global__ __launch_bounds__(kBlock) void k_gpp_grad_combine(long n, const double* a, const double* b, const double* c,
                                                                    double* out) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = (a[i] - b[i]) + c[i];
}

}  // namespace pgps
