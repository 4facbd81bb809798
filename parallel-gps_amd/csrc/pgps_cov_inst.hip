// pgps_cov_inst.hip -- the joint-covariance kernels (pgps_cov.hip.h) for one (dtype, state dimension): PGPS_COV_T,
// PGPS_COV_D.
#include <algorithm>

#include "pgps_cov.hip.h"
#include "pgps_scratch.h"

#ifndef PGPS_COV_T
#error "compile with -DPGPS_COV_T=<float|double> -DPGPS_COV_D=<d>"
#endif

namespace pgps {

template <typename T, int D>
int launch_cov_gains(pgps_ctx* ctx, CovArgs<T> a) {
    constexpr int NREC = ElemTraits<GainElem<T, D>>::N;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    geometry(ctx, a.N, &a.Lc, &a.nblocks, D);
    a.nlanes = (long)a.nblocks * kBlock;
    // the spine starts on a whole 32 elements behind the lane suffixes (those are whole 256-lane rows)
    Carver c(32 * sizeof(T));
    const auto lsuf = c.part<T>((size_t)NREC * (size_t)a.nlanes), spine = c.part<T>((size_t)a.nblocks * NREC);
    Scratch s;
    if (int rc = commit(ctx, ctx->cov[0], c, &s)) return rc;
    a.lsuf = s(lsuf); a.spine = s(spine);
    const dim3 grid(a.nblocks), block(kBlock);
    hipLaunchKernelGGL((k_cov_reduce<T, D>), grid, block, 0, ctx->stream, a);
    hipLaunchKernelGGL((k_cov_apply<T, D>), grid, block, 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

template <typename T, int D>
int launch_cov_fill(pgps_ctx* ctx, CovFillArgs<T> a) {
    constexpr size_t MAT = (size_t)D * D;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long nt = (a.n + kCovTile - 1) / kCovTile;
    if (nt > 65535) return PGPS_E_INVALID;
    a.nt = (int)nt;
    Carver c(32 * sizeof(T));                           // M starts on a whole 32 elements behind U
    const auto U = c.part<T>((size_t)a.n * MAT), M = c.part<T>((size_t)nt * nt * MAT);
    Scratch s;
    if (int rc = commit(ctx, ctx->cov[4], c, &s)) return rc;
    a.U = s(U); a.M = s(M);
    const dim3 wave(kCovTile);
    if (nt > 1) hipLaunchKernelGGL((k_cov_tile_prefix<T, D>), dim3((unsigned)(nt - 1)), wave, 0, ctx->stream, a);
    if (nt > 2)
        hipLaunchKernelGGL((k_cov_tile_chain<T, D>), dim3((unsigned)((nt - 2 + kCovTile - 1) / kCovTile)), wave, 0, ctx->stream, a);
    const dim3 grid((unsigned)nt, (unsigned)nt);
    if (a.proj) hipLaunchKernelGGL((k_cov_fill<T, D, true>), grid, wave, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_cov_fill<T, D, false>), grid, wave, 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

template int launch_cov_gains<PGPS_COV_T, PGPS_COV_D>(pgps_ctx*, CovArgs<PGPS_COV_T>);
template int launch_cov_fill<PGPS_COV_T, PGPS_COV_D>(pgps_ctx*, CovFillArgs<PGPS_COV_T>);

}  // namespace pgps
