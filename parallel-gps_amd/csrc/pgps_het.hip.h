// pgps_het.hip.h -- the reduce and Kalman-pass kernels of the per-observation-noise flavour, shared by
// the units that launch them: pgps_het_inst.hip (log-likelihood, predict_f) and pgps_site_inst.hip (the Newton step of a
// Laplace approximation, whose sites are per-step variances).
#pragma once

#include "pgps_fused.hip.h"

namespace pgps {

struct GpHetArgs {
    GpArgs<double> g;
    const double* rs;       // (N,) per-step variances added to g.s.R; read at observed steps only      [device]
};

template <int D>
__global__ __launch_bounds__(kBlock) void k_gph_reduce(const GpHetArgs h) {
    __shared__ double lds[kWaves * Dim<D>::NFILT];
    gp_reduce_body<double, D, true>(h.g, lds, h.rs);
}

template <int D, bool SMOOTH>
__global__ __launch_bounds__(kBlock) void k_gph_apply(const GpHetArgs h) {
    __shared__ GpLds<double, D> sh;
    gp_apply_body<double, D, SMOOTH, false, true>(h.g, sh, h.rs);
}

}  // namespace pgps
