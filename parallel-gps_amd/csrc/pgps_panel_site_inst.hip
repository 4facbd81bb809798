// pgps_panel_site_inst.hip -- one translation unit per state dimension d = 1, 2, 3 (fp64): the mode search of a Laplace
// approximation for a panel of series in one launch per group (pgps_panel_site.hip.h: k_gpp_newton, one workgroup per series,
// the whole damped Newton loop inside), the gradient's inputs and combination, and the launch functions the C ABI dispatches
// to (pgps_panel_site_api.hip).  DESIGN.md section 4ab.
//
// Scratch (pgps_panel_site_lay.h, all of it in the context's scan scratch): a series needs its nine per-row arrays -- the
// iterate (f, alpha, zs, ss), the proposal (f, alpha, zs, ss) and v -- and its filtered moments once, every slice padded to
// kPanelAlign, plus the fixed records lpre, lsuf, spine, sspine, llpart and the five site partials at slot * record length.
// Series close into groups by the panel's rule (the group's layout fits pgps_set_batch_scratch, at most 65535 series); the
// next group reuses the scratch on the same stream.  Steps per lane come from the series' own length and the pinned chunk
// alone, and no arithmetic crosses workgroups: a row's bits depend on that series alone.
#include <cstring>
#include <vector>

#include "pgps_panel_site.h"
#include "pgps_panel_site.hip.h"
#include "pgps_scratch.h"

#ifndef PGPS_PANEL_SITE_D
#error "compile with -DPGPS_PANEL_SITE_D=<1|2|3>"
#endif

namespace pgps {

// The panel's adjoint kernel is instantiated in pgps_panel_inst.hip and nowhere else: this unit launches that copy (one device
// function, one resource report), it does not compile a second one under its own flags
extern template __global__ void k_gpp_gone<PGPS_PANEL_SITE_D, true>(const PanelArgs);

// the records and groups of a call, and its three tables [models | pars | records] on the device behind ONE copy and the one
// synchronisation of the call
struct SiteTables {
    std::vector<PanelDesc> desc;
    std::vector<SiteGroup> groups;
    size_t ngroups = 0, need = 0;
    const double* dmodels = nullptr;
    const double* dpars = nullptr;
    const PanelDesc* ddesc = nullptr;
};

template <int D>
static int site_tables(pgps_ctx* ctx, const PanelSiteCall& c, bool grad, size_t fixed_bytes, SiteTables* t) {
    constexpr SiteRecLens lens = site_rec_lens(D);
    static_assert(lens.nfilt == Dim<D>::NFILT && lens.nsmth == Dim<D>::NSMTH && lens.nx == D + Dim<D>::SYM &&
                  lens.nst == gp_adj_nstat<D>(), "pgps_panel_site_lay.h restates the record lengths");
    const size_t S = (size_t)c.S;
    t->desc.resize(S);
    t->groups.resize(S);
    t->need = site_groups(
        S, D, grad, ctx->chunk, batch_budget_fused(ctx), [&](size_t s) { return c.offs[s + 1] - c.offs[s]; },
        [&](size_t s, size_t first, const SiteSlices& sl, int Lc) {
            (void)first;
            PanelDesc& r = t->desc[s];
            r.row0 = c.offs[s];
            r.q0 = 0;
            r.m0 = (long)sl.o_rows;
            r.o_fm = (long)sl.o_fm; r.o_fP = (long)sl.o_fP; r.o_xs = (long)sl.o_xs;
            r.n = (int)(c.offs[s + 1] - c.offs[s]);
            r.k = 0;
            r.m = r.n;
            r.Lc = Lc;
            r.slot = (int)sl.slot;
            r.model = c.nmodels == 1 ? 0 : (int)s;
        },
        t->groups.data(), &t->ngroups);
    const size_t mbytes = align_up((size_t)c.nmodels * kGpModelStride * sizeof(double), 256);
    const size_t pbytes = align_up((size_t)c.npars * sizeof(double), 256);
    std::vector<char> tables(mbytes + pbytes + S * sizeof(PanelDesc));
    memcpy(tables.data(), c.models, (size_t)c.nmodels * kGpModelStride * sizeof(double));
    memcpy(tables.data() + mbytes, c.pars, (size_t)c.npars * sizeof(double));
    memcpy(tables.data() + mbytes + pbytes, t->desc.data(), S * sizeof(PanelDesc));
    if (int rc = ensure(ctx, ctx->panel, tables.size())) return rc;
    if (int rc = ensure(ctx, ctx->ws, fixed_bytes + t->need)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->panel.p, tables.data(), tables.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the host vector dies with this function)
    const char* base = (const char*)ctx->panel.p;
    t->dmodels = reinterpret_cast<const double*>(base);
    t->dpars = reinterpret_cast<const double*>(base + mbytes);
    t->ddesc = reinterpret_cast<const PanelDesc*>(base + mbytes + pbytes);
    return PGPS_OK;
}

// the panel's view of one group over the parts of its layout
static PanelArgs site_panel_args(pgps_ctx* ctx, const PanelSiteCall& c, const SiteTables& t, const SiteGroup& G, const Scratch& s,
                                 const SiteParts& q) {
    PanelArgs p{};
    p.desc = t.ddesc + G.first;
    p.models = t.dmodels;
    p.ts = c.ts;
    p.ys = c.ys;
    p.spine = s(q.spine); p.lpre = s(q.lpre); p.sspine = s(q.sspine); p.lsuf = s(q.lsuf); p.llpart = s(q.ll);
    p.fms = s(q.fms); p.fPs = s(q.fPs);
    p.xs = s(q.xs); p.gpart = s(q.gpart);
    p.status = ctx->status_word;
    return p;
}

template <int D>
int launch_gp_panel_laplace(pgps_ctx* ctx, const PanelSiteCall& c) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SiteTables t;
    if (int rc = site_tables<D>(ctx, c, false, 0, &t)) return rc;
    const dim3 block(kBlock);
    for (size_t i = 0; i < t.ngroups; ++i) {
        const SiteGroup& G = t.groups[i];
        Carver cw(256);
        const SiteParts q = site_lay(cw, G.t, D);
        const Scratch s{(char*)ctx->ws.p};                          // (ensured above for the largest group)
        PanelSiteArgs a{};
        a.p = site_panel_args(ctx, c, t, G, s, q);
        a.lik = c.lik;
        a.pars = t.dpars + (c.npars == 1 ? 0 : G.first);
        a.par_stride = c.npars == 1 ? 0 : 1;
        a.tol = c.tol;
        a.max_iter = c.max_iter;
        a.rows = s(q.rows);
        a.part = s(q.part);
        a.f = c.f; a.v = c.v; a.zs = c.zs; a.ss = c.ss;
        a.info = c.info + G.first * (size_t)kSiteInfo;
        // (no timer slot of its own: a whole search is charged to the smoother's, PGPS_K_SMOOTHER_APPLY, as is the gradient's
        // input kernel below; include/pgps.h says so)
        timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gpp_newton<D>, dim3(1, (unsigned)G.t.series), block, 0, a);
        HIPCHK(ctx, hipGetLastError());
    }
    return PGPS_OK;
}

// out (S, 1 + NST): per group the elementwise inputs, then three launches of the panel's adjoint kernel k_gpp_gone<D, true>
// on (x_i, ss) with R = 0; one combination over all rows at the end
template <int D>
int launch_gp_panel_laplace_grad(pgps_ctx* ctx, const PanelSiteCall& c) {
    constexpr int NST = gp_adj_nstat<D>();
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t S = (size_t)c.S, rows = (size_t)c.offs[S], nout = S * (size_t)(1 + NST);
    Carver fixed(256);
    Part<double> x[3], o[3];
    for (int i = 0; i < 3; ++i) x[i] = fixed.part<double>(rows);
    for (int i = 0; i < 3; ++i) o[i] = fixed.part<double>(nout);
    SiteTables t;
    if (int rc = site_tables<D>(ctx, c, true, fixed.bytes(), &t)) return rc;
    const Scratch sf{(char*)ctx->ws.p}, s{(char*)ctx->ws.p + fixed.bytes()};
    const dim3 block(kBlock);
    for (size_t i = 0; i < t.ngroups; ++i) {
        const SiteGroup& G = t.groups[i];
        Carver cw(256);
        const SiteParts q = site_lay(cw, G.t, D);
        const dim3 grid(1, (unsigned)G.t.series);
        PanelSiteGradArgs ga{};
        ga.desc = t.ddesc + G.first;
        ga.lik = c.lik;
        ga.pars = t.dpars + (c.npars == 1 ? 0 : G.first);
        ga.par_stride = c.npars == 1 ? 0 : 1;
        ga.ys = c.ys; ga.f = c.f; ga.v = c.v; ga.zs = c.zs;
        ga.x1 = sf(x[0]); ga.x2 = sf(x[1]); ga.x3 = sf(x[2]);
        timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gpp_grad_inputs, grid, block, 0, ga);
        for (int j = 0; j < 3; ++j) {
            PanelArgs p = site_panel_args(ctx, c, t, G, s, q);
            p.ys = sf(x[j]);
            p.rs = c.ss;
            p.out = sf(o[j]) + G.first * (size_t)(1 + NST);
            timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpp_gone<D, true>, grid, block, 0, p);
        }
        HIPCHK(ctx, hipGetLastError());
    }
    const unsigned nb = (unsigned)((nout + kBlock - 1) / kBlock);
    timed_launch(ctx, PGPS_K_LL_FINALIZE, k_gpp_grad_combine, dim3(nb), block, 0, (long)nout, (const double*)sf(o[0]),
                 (const double*)sf(o[1]), (const double*)sf(o[2]), c.out);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

template int launch_gp_panel_laplace<PGPS_PANEL_SITE_D>(pgps_ctx*, const PanelSiteCall&);
template int launch_gp_panel_laplace_grad<PGPS_PANEL_SITE_D>(pgps_ctx*, const PanelSiteCall&);

}  // namespace pgps
