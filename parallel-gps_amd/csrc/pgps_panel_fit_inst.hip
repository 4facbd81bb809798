// pgps_panel_fit_inst.hip -- one translation unit per state dimension d = 1, 2, 3 (fp64): the hyper-parameter fit of a panel of
// series in one launch per group (pgps_panel_fit.hip.h: k_gpp_fit, one workgroup per series, the whole projected-BFGS search
// inside) and the launch function the C ABI dispatches to (pgps_panel_fit_api.hip).  DESIGN.md section 4af.
//
// Scratch (all of it in the context's scan scratch): what one adjoint pass of a series needs -- its kept states xs and the fixed
// records lpre, lsuf, spine, sspine, llpart, gpart at slot * record length -- laid out by pgps_panel_site_lay.h exactly as the
// Laplace panel's gradient lays it out; every evaluation of the search reuses it.  Series close into groups by the panel's
// rule (the group's layout fits pgps_set_batch_scratch, at most 65535 series); the next group reuses the scratch on the same
// stream.  Steps per lane come from the series' own length and the pinned chunk alone, and no arithmetic crosses workgroups: a
// row's bits depend on that series alone.
#include <cstring>
#include <vector>

#include "pgps_panel_fit.h"
#include "pgps_panel_fit.hip.h"
#include "pgps_panel_site_lay.h"
#include "pgps_scratch.h"

#ifndef PGPS_PANEL_FIT_D
#error "compile with -DPGPS_PANEL_FIT_D=<1|2|3>"
#endif

namespace pgps {

static_assert(kSiteAlign == kPanelAlign && kSiteLanes == kBlock, "pgps_panel_site_lay.h restates them");

template <int D>
int launch_gp_panel_fit(pgps_ctx* ctx, const PanelFitCall& c) {
    constexpr SiteRecLens lens = site_rec_lens(D);
    static_assert(lens.nfilt == Dim<D>::NFILT && lens.nsmth == Dim<D>::NSMTH && lens.nx == D + Dim<D>::SYM &&
                  lens.nst == gp_adj_nstat<D>(), "pgps_panel_site_lay.h restates the record lengths");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t S = (size_t)c.S;
    std::vector<PanelDesc> desc(S);
    std::vector<SiteGroup> groups(S);
    size_t ngroups = 0;
    const size_t need = site_groups(
        S, D, true, ctx->chunk, batch_budget_fused(ctx), [&](size_t s) { return c.offs[s + 1] - c.offs[s]; },
        [&](size_t s, size_t first, const SiteSlices& sl, int Lc) {
            (void)first;
            PanelDesc& r = desc[s];
            r = PanelDesc{};
            r.row0 = c.offs[s];
            r.o_xs = (long)sl.o_xs;
            r.n = (int)(c.offs[s + 1] - c.offs[s]);
            r.m = r.n;
            r.Lc = Lc;
            r.slot = (int)sl.slot;
            r.model = 0;                                            // (the table is the unit row)
        },
        groups.data(), &ngroups);
    // [unit row | start records | descriptors] on the device behind ONE copy and the one synchronisation of the call
    const size_t mbytes = align_up((size_t)kGpModelStride * sizeof(double), 256);
    const size_t rbytes = align_up(S * kFitRecord * sizeof(double), 256);
    std::vector<char> tables(mbytes + rbytes + S * sizeof(PanelDesc));
    memcpy(tables.data(), c.unit, (size_t)kGpModelStride * sizeof(double));
    memcpy(tables.data() + mbytes, c.records, S * kFitRecord * sizeof(double));
    memcpy(tables.data() + mbytes + rbytes, desc.data(), S * sizeof(PanelDesc));
    if (int rc = ensure(ctx, ctx->panel, tables.size())) return rc;
    if (int rc = ensure(ctx, ctx->ws, need)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->panel.p, tables.data(), tables.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the host vector dies with this function)
    const char* base = (const char*)ctx->panel.p;
    const double* dunit = reinterpret_cast<const double*>(base);
    const double* drec = reinterpret_cast<const double*>(base + mbytes);
    const PanelDesc* ddesc = reinterpret_cast<const PanelDesc*>(base + mbytes + rbytes);
    const dim3 block(kBlock);
    for (size_t i = 0; i < ngroups; ++i) {
        const SiteGroup& G = groups[i];
        Carver cw(256);
        const SiteParts q = site_lay(cw, G.t, D);
        const Scratch s{(char*)ctx->ws.p};                          // (ensured above for the largest group)
        PanelFitArgs a{};
        a.p.desc = ddesc + G.first;
        a.p.models = dunit;
        a.p.ts = c.ts; a.p.ys = c.ys; a.p.rs = c.rs;
        a.p.spine = s(q.spine); a.p.lpre = s(q.lpre); a.p.sspine = s(q.sspine); a.p.lsuf = s(q.lsuf); a.p.llpart = s(q.ll);
        a.p.xs = s(q.xs); a.p.gpart = s(q.gpart);
        a.p.status = ctx->status_word;
        a.records = drec + G.first * (size_t)kFitRecord;
        for (int j = 0; j < kFitP; ++j) a.free_[j] = c.free_[j];
        a.gtol = c.gtol;
        a.max_iter = c.max_iter;
        a.thetas = c.thetas + G.first * (size_t)kFitP;
        a.info = c.info + G.first * (size_t)kFitInfo;
        const dim3 grid(1, (unsigned)G.t.series);
        // (no timer slot of its own: a whole search is charged to the adjoint pass's, PGPS_K_FILTER_APPLY; include/pgps.h says so)
        if (c.rs) timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_fit<D, true>, grid, block, 0, a);
        else timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_fit<D, false>, grid, block, 0, a);
        HIPCHK(ctx, hipGetLastError());
    }
    return PGPS_OK;
}

template int launch_gp_panel_fit<PGPS_PANEL_FIT_D>(pgps_ctx*, const PanelFitCall&);

}  // namespace pgps
