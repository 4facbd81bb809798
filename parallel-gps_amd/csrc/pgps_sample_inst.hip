// pgps_sample_inst.hip -- the backward sampler (pgps_sample.hip.h) for one (dtype, state dimension): PGPS_SAMP_T,
// PGPS_SAMP_D.  The unit of d = 1 also carries the draw kernel (k_sample_normals), which takes d at run time.
#include <algorithm>

#include "pgps_sample.hip.h"
#include "pgps_scratch.h"

#ifndef PGPS_SAMP_T
#error "compile with -DPGPS_SAMP_T=<float|double> -DPGPS_SAMP_D=<d>"
#endif

namespace pgps {

template <typename T, int D>
int launch_sample(pgps_ctx* ctx, SampleArgs<T> a) {
    constexpr int SG = SampleGroup<T, D>::SG;
    constexpr int NREC = ElemTraits<SampElem<T, D, SG>>::N;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    geometry(ctx, a.N, &a.Lc, &a.nblocks, D);
    a.nlanes = (long)a.nblocks * kBlock;
    const long groups = ((long)a.S + SG - 1) / SG;
    if (groups > 65535) return PGPS_E_INVALID;
    a.ngroups = (int)groups;
    // the spine starts on a whole 32 elements behind the lane suffixes (those are whole 256-lane rows)
    Carver c(32 * sizeof(T));
    const auto lsuf = c.part<T>((size_t)a.ngroups * NREC * (size_t)a.nlanes), spine = c.part<T>((size_t)a.ngroups * a.nblocks * NREC);
    Scratch s;
    if (int rc = commit(ctx, ctx->smp, c, &s)) return rc;
    a.lsuf = s(lsuf); a.spine = s(spine);
    const dim3 grid(a.nblocks, a.ngroups), block(kBlock);
    hipLaunchKernelGGL((k_sample_reduce<T, D>), grid, block, 0, ctx->stream, a);
    hipLaunchKernelGGL((k_sample_apply<T, D>), grid, block, 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

template int launch_sample<PGPS_SAMP_T, PGPS_SAMP_D>(pgps_ctx*, SampleArgs<PGPS_SAMP_T>);

#if PGPS_SAMP_D == 1
template <typename T>
int launch_sample_normals(pgps_ctx* ctx, long N, int d, int S, long s0, unsigned long long seed, T* z) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long total = (long)S * N * ((d + 1) / 2);
    const long grid = std::min<long>(16384, (total + 255) / 256);
    hipLaunchKernelGGL(k_sample_normals<T>, dim3((unsigned)std::max<long>(1, grid)), dim3(256), 0, ctx->stream, N, d, S, s0,
                       seed, z);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}
template int launch_sample_normals<PGPS_SAMP_T>(pgps_ctx*, long, int, int, long, unsigned long long, PGPS_SAMP_T*);
#endif

}  // namespace pgps
