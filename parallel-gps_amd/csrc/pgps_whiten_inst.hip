// pgps_whiten_inst.hip -- one translation unit per state dimension d = 1, 2, 3 (fp64): the whitening flavour of the
// multi-column Kalman pass and the Gram kernels of pgps_whiten.hip.h, and the launch function the C ABI dispatches to.
#include "pgps_whiten.hip.h"
#include "pgps_scratch.h"

#ifndef PGPS_MULTI_D
#error "compile with -DPGPS_MULTI_D=<1|2|3>"
#endif

namespace pgps {

template <int D>
int launch_gp_whiten(pgps_ctx* ctx, GpMultiArgs a, double* w, double* gram, double* logdet, long* n_obs) {
    constexpr int MC = MultiTile<D>::MC;
    using FE = FiltElemM<double, D, MC>;
    if ((w == nullptr) == (gram == nullptr)) return PGPS_E_INVALID;
    if (gram && a.M > kGramMax) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int groups_all = (a.M + MC - 1) / MC;
    multi_geometry(ctx, a.N, groups_all, &a.Lc, &a.nblocks);
    a.nlanes = (long)a.nblocks * kBlock;
    if (a.nblocks > 0x7fffff) return PGPS_E_INVALID;
    const size_t nb = (size_t)a.nblocks, nl = (size_t)a.nlanes, n = (size_t)a.N;
    const size_t nparts = gram ? (n + kGramSlab - 1) / kGramSlab : 0;
    const size_t g_spine = nb * FE::N, g_lpre = nl * FE::N;
    Carver c(256);
    const auto ldpart = c.part<double>(2 * nb), gpart = c.part<double>(nparts * kGramRec);
    // the rounds are those of launch_gp_multi: W, which a Gram call keeps in scratch, is no part of what the budget splits
    const size_t group = batch_group(batch_budget_fused(ctx), c.bytes(), (g_spine + g_lpre) * sizeof(double), (size_t)groups_all);
    const auto spine = c.part<double>(group * g_spine), lpre = c.part<double>(group * g_lpre);
    const auto wpart = c.part<double>(gram ? n * (size_t)a.M : 0);
    Scratch s;
    if (int rc = commit(ctx, ctx->ws, c, &s)) return rc;
    a.spine = s(spine); a.lpre = s(lpre);
    GpWhitenOut o;
    o.w = gram ? s(wpart) : w;
    o.ldw = a.M;
    o.w_aligned = ((reinterpret_cast<uintptr_t>(o.w) & 15u) == 0) ? 1 : 0;
    o.ldpart = s(ldpart);
    const dim3 block(kBlock);
    for (size_t g0 = 0; g0 < (size_t)groups_all; g0 += group) {
        const unsigned G = (unsigned)((size_t)groups_all - g0 < group ? (size_t)groups_all - g0 : group);
        a.c_base = (int)(g0 * MC);
        const dim3 grid(a.nblocks, G);
        timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_gpm_reduce<D, MC>, grid, block, 0, a);
        timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gpm_whiten<D, MC>, grid, block, 0, a, o);
        HIPCHK(ctx, hipGetLastError());
    }
    timed_launch(ctx, PGPS_K_LL_FINALIZE, k_whiten_finalize, dim3(1), block, 0, (const double*)o.ldpart, a.nblocks, logdet, n_obs);
    if (gram) {
        timed_launch(ctx, PGPS_K_LL_FINALIZE, k_gram_partial<kGramMax>, dim3((unsigned)nparts), block, 0, (const double*)o.w, a.N, a.M,
                     s(gpart));
        timed_launch(ctx, PGPS_K_LL_FINALIZE, k_gram_finalize, dim3(kGramRec), block, 0, (const double*)s(gpart), (long)nparts, a.M, gram);
    }
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

template int launch_gp_whiten<PGPS_MULTI_D>(pgps_ctx*, GpMultiArgs, double*, double*, double*, long*);

}  // namespace pgps
