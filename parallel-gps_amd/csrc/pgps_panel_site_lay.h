// pgps_panel_site_lay.h -- how pgps_gp_panel_laplace_* lays out its device scratch: the carver parts of a
// group of series, the slices of one series inside them, its steps per lane, and the rule by which series close into groups
// that fit a budget.  Plain C++ on pgps_scratch.h (tests/cpu_math/newton_ctl.cpp checks it on the host); the launch functions
// of pgps_panel_site_inst.hip are its only users on the device side.
#pragma once

#include <cstddef>

#include "pgps_scratch.h"

namespace pgps {

constexpr int kSiteAlign = 32;          // == kPanelAlign: every ragged slice starts on a multiple (elements)
constexpr int kSiteLanes = 256;         // == kBlock: lanes of the one workgroup a series has
// the per-row arrays of a series, each site_pad(n) doubles, in this order behind its o_rows:
//   0..3 the iterate (f, alpha, zs, ss)    4..7 the proposal (f, alpha, zs, ss)    8 v, the variances of the last pass
constexpr int kSiteRowArrays = 9;
constexpr int kSiteInfo = 8;            // doubles of an info row
constexpr int kSitePartials = 5;        // == kSiteParts

inline size_t site_pad(size_t n) { return align_up(n, (size_t)kSiteAlign); }

// record lengths by state dimension (Dim<D> of pgps_math.h and gp_adj_nstat<D>, restated for the host: the device unit
// static_asserts that they agree)
struct SiteRecLens { int nfilt, nsmth, nx, nst; };
constexpr SiteRecLens site_rec_lens(int d) {
    return {d * d + d + d * (d + 1) + d, d * d + d + d * (d + 1) / 2, d + d * (d + 1) / 2, d * d + 2 * d + 1};
}

// steps per lane of a series of n rows: the panel's rule (pgps_scratch.h)
static_assert(kSiteLanes == kPanelLanes, "panel_steps_per_lane counts the lanes of a series' one workgroup");
inline int site_steps_per_lane(int n, int chunk) { return panel_steps_per_lane(n, chunk); }

// element counts of a group
struct SiteTotals {
    size_t series = 0, rows = 0, fm = 0, fP = 0, xs = 0;
};
// where one series lies in its group's parts (element offsets, multiples of kSiteAlign) and its place among the fixed records
struct SiteSlices {
    size_t o_rows, o_fm, o_fP, o_xs, slot;
};
// the search needs rows / fm / fP; the gradient's adjoint passes need xs (kept states, (d + sym) Lc lanes)
inline SiteSlices site_add(SiteTotals& t, size_t n, int d, bool grad, int Lc) {
    const SiteSlices s{t.rows, t.fm, t.fP, t.xs, t.series};
    t.series += 1;
    if (grad) {
        t.xs += site_pad((size_t)Lc * site_rec_lens(d).nx * kSiteLanes);
    } else {
        t.rows += kSiteRowArrays * site_pad(n);
        t.fm += site_pad(n * d);
        t.fP += site_pad(n * d * d);
    }
    return s;
}

struct SiteParts {
    Part<double> rows, fms, fPs, spine, lpre, sspine, lsuf, ll, part, xs, gpart;
};
inline SiteParts site_lay(Carver& c, const SiteTotals& t, int d) {
    const SiteRecLens r = site_rec_lens(d);
    SiteParts p;
    p.rows = c.part<double>(t.rows);
    p.fms = c.part<double>(t.fm);
    p.fPs = c.part<double>(t.fP);
    p.spine = c.part<double>(t.series * r.nfilt);
    p.lpre = c.part<double>(t.series * kSiteLanes * r.nfilt);
    p.sspine = c.part<double>(t.series * r.nsmth);
    p.lsuf = c.part<double>(t.series * kSiteLanes * r.nsmth);
    p.ll = c.part<double>(t.series);
    p.part = c.part<double>(t.series * kSitePartials);
    p.xs = c.part<double>(t.xs);
    p.gpart = c.part<double>(t.xs ? t.series * r.nst : 0);
    return p;
}
inline size_t site_bytes(const SiteTotals& t, int d) {
    Carver c(256);
    site_lay(c, t, d);
    return c.bytes();
}

// Series close into groups in order: series s joins the open group unless the group's layout would then exceed the budget
// or the grid (kGridYMax); one series is the least a group holds.  visit(s, first series of its group, slices) per series;
// returns the bytes of the largest group.
struct SiteGroup {
    size_t first;
    SiteTotals t;
};
template <typename LenOf, typename Visit>
inline size_t site_groups(size_t S, int d, bool grad, int chunk, size_t budget, LenOf len_of, Visit visit, SiteGroup* groups,
                          size_t* ngroups) {
    size_t need = 0, ng = 0;
    for (size_t s = 0; s < S; ++s) {
        const size_t n = (size_t)len_of(s);
        const int Lc = site_steps_per_lane((int)n, chunk);
        bool open = ng > 0 && groups[ng - 1].t.series < kGridYMax;
        if (open) {
            SiteTotals t = groups[ng - 1].t;
            site_add(t, n, d, grad, Lc);
            open = site_bytes(t, d) <= budget;
        }
        if (!open) groups[ng++] = SiteGroup{s, SiteTotals{}};
        SiteGroup& G = groups[ng - 1];
        const SiteSlices sl = site_add(G.t, n, d, grad, Lc);
        visit(s, G.first, sl, Lc);
        const size_t b = site_bytes(G.t, d);
        if (b > need) need = b;
    }
    *ngroups = ng;
    return need;
}

}  // namespace pgps
