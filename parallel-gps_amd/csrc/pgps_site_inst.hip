// pgps_site_inst.hip -- one translation unit per state dimension d = 1, 2, 3 (fp64): one Newton step of a Laplace approximation
//  and the launch functions the C ABI dispatches to (pgps_site_api.hip).
//
// A Newton step of the mode search under a log-concave likelihood is a Gaussian smoothing pass over pseudo-observations z_k
// with per-step variances s_k (the SITES, pgps_lik.h).  Four launches: k_gph_reduce and k_gph_apply<D, true> as
// pgps_het_inst.hip launches them, on (zs, ss) with R = 0; k_gps_smooth, the SITE flavour of gp_smooth_body (projection at every
// step, the epilogue site_step: alpha, the likelihood at the new iterate, the new sites, per-lane sums); and a one-workgroup
// finalize that adds the workgroups' partials in index order (repeatable bit for bit; the maximum is exact in any order).
// Between two steps nothing but the six sums has to leave the device.  The d = 1 unit also holds the elementwise kernel of the
// start and of the damped steps (k_lik_sites) and its finalize.  No one-workgroup form, no resident launch, no streaming stores.
#include "pgps_het.hip.h"
#include "pgps_scratch.h"

#ifndef PGPS_SITE_D
#error "compile with -DPGPS_SITE_D=<1|2|3>"
#endif

namespace pgps {

struct GpSiteArgs {
    GpArgs<double> g;
    GpSiteOut<double> o;
};

template <int D>
__global__ __launch_bounds__(kBlock) void k_gps_smooth(const GpSiteArgs l) {
    __shared__ GpLds<double, D> sh;
    gp_smooth_body<double, D, false, false, false, true>(l.g, sh, GpLooOut<double>{}, l.o);
}

// one workgroup: lane-strided partial sums of map.n rows of part (row r at part + r * nblocks) and a fixed tree; the row
// max_row is reduced by maximum instead.  sums[i] takes row src[i]
struct FinalizeMap {
    int n;
    int src[6];             // row of part (or -1: the row llpart)
    int max_row;            // the row that holds maxima, -1: none
};
static __global__ __launch_bounds__(kBlock) void k_site_finalize(const double* llpart, const double* part, int nblocks,
                                                                FinalizeMap map, double* sums) {
    __shared__ double lds_ll[kWaves];
    for (int i = 0; i < map.n; ++i) {
        const int r = map.src[i];
        const double* row = r < 0 ? llpart : part + (long)r * nblocks;
        double t;
        if (r >= 0 && r == map.max_row) {
            double v = 0.0;
            for (int b = threadIdx.x; b < nblocks; b += kBlock) v = max_nan(v, row[b]);
            t = block_max_nan(v, lds_ll);
        } else {
            double v = 0.0;
            for (int b = threadIdx.x; b < nblocks; b += kBlock) v += row[b];
            t = block_sum_double(v, lds_ll);
        }
        if (threadIdx.x == 0) sums[i] = t;
    }
}

template <int D>
int launch_gp_newton(pgps_ctx* ctx, GpArgs<double> g, GpSiteOut<double> o, double* sums) {
    ScanArgs<double>& a = g.s;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    geometry(ctx, a.N, &a.Lc, &a.nblocks);
    a.nlanes = (long)a.nblocks * kBlock;
    a.seg_first = 1;
    a.seg_last = 1;
    a.shortcut = (ctx->shortcut != 0 && (long)kBlock * a.Lc >= 2048) ? 1 : 0;      // (as launch_gp sets it)
    a.ll = nullptr;                             // (the finalize launch sums the partials)
    a.ll_in_apply = 0;
    const size_t nl = (size_t)a.nlanes, nb = (size_t)a.nblocks;
    Carver c(256);
    const auto spine = c.part<double>(nb * Dim<D>::NFILT), lpre = c.part<double>(nl * Dim<D>::NFILT);
    const auto sspine = c.part<double>(nb * Dim<D>::NSMTH), lsuf = c.part<double>(nl * Dim<D>::NSMTH);
    const auto ll = c.part<double>(nb), part = c.part<double>(nb * kSiteParts);
    Scratch s;
    if (int rc = commit(ctx, ctx->ws, c, &s)) return rc;
    a.spine = s(spine); a.lpre = s(lpre); a.sspine = s(sspine); a.lsuf = s(lsuf);
    a.llpart = s(ll);
    a.status = ctx->status_word;
    o.part = s(part);
    const GpHetArgs h{g, o.ss};
    const GpSiteArgs l{g, o};
    const dim3 grid(a.nblocks), block(kBlock);
    timed_launch(ctx, PGPS_K_FILTER_REDUCE, k_gph_reduce<D>, grid, block, 0, h);
    timed_launch(ctx, PGPS_K_FILTER_APPLY, k_gph_apply<D, true>, grid, block, 0, h);
    timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_gps_smooth<D>, grid, block, 0, l);
    // sums = [ll | lp | f alpha | correction | max |f - f_prev| | observed steps]
    const FinalizeMap map{6, {-1, 0, 1, 2, 3, 4}, 3};
    timed_launch(ctx, PGPS_K_LL_FINALIZE, k_site_finalize, dim3(1), block, 0, (const double*)a.llpart, (const double*)o.part,
                 a.nblocks, map, sums);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

template int launch_gp_newton<PGPS_SITE_D>(pgps_ctx*, GpArgs<double>, GpSiteOut<double>, double*);

#if PGPS_SITE_D == 1
// the sites at f = f_a + step (f_b - f_a): lane gt of the grid owns the elements gt, gt + lanes, ... (a grid fixed by N alone)
static __global__ __launch_bounds__(kBlock) void k_lik_sites(const LikSitesArgs a) {
    __shared__ double lds_ll[kWaves];
    const long lanes = (long)gridDim.x * kBlock;
    double lp = 0.0, fa = 0.0, corr = 0.0;
    for (long k = (long)blockIdx.x * kBlock + threadIdx.x; k < a.N; k += lanes) {
        double f = a.f_a[k], al = a.alpha_a[k];
        if (a.f_b != nullptr) {
            f += a.step * (a.f_b[k] - f);
            al += a.step * (a.alpha_b[k] - al);
        }
        const double y = a.ys[k];
        double z_new = y, s_new = 1.0;              // (y is NaN at a missing row)
        if (!is_nan(y)) {
            const LikSite ls = lik_site(a.lik, a.par, y, f);
            z_new = ls.z;
            s_new = ls.s;
            lp += ls.lp;
            corr += ls.corr;
        }
        fa += f * al;
        a.f_out[k] = f;
        a.alpha_out[k] = al;
        a.zs_out[k] = z_new;
        a.ss_out[k] = s_new;
    }
    const double vals[3] = {lp, fa, corr};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double t = block_sum_double(vals[i], lds_ll);
        if (threadIdx.x == 0) a.part[(long)i * a.nblocks + blockIdx.x] = t;
    }
}

int launch_lik_sites(pgps_ctx* ctx, LikSitesArgs a, double* sums) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    a.nblocks = (int)std::min<long>(1024, (a.N + kBlock - 1) / kBlock);
    Carver c(256);
    const auto part = c.part<double>((size_t)a.nblocks * 3);
    Scratch s;
    if (int rc = commit(ctx, ctx->ws, c, &s)) return rc;
    a.part = s(part);
    timed_launch(ctx, PGPS_K_SMOOTHER_APPLY, k_lik_sites, dim3(a.nblocks), dim3(kBlock), 0, a);
    const FinalizeMap map{3, {0, 1, 2, 0, 0, 0}, -1};
    timed_launch(ctx, PGPS_K_LL_FINALIZE, k_site_finalize, dim3(1), dim3(kBlock), 0, (const double*)nullptr,
                 (const double*)a.part, a.nblocks, map, sums);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}
#endif

}  // namespace pgps
