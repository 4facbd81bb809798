// pgps_sample.hip.h -- joint posterior draws of x_0 .. x_{N-1} | ys by a parallel backward-sampling scan.
//
// Backward sampling runs the smoother's recursion with noise:  x_{N-1} = fm_{N-1} + C(fP_{N-1}) z_{N-1},
// x_k = E_k x_{k+1} + g_k + C(L_k) z_k, with (E_k, g_k, L_k) the smoothing element of step k (pgps_math.h smth_element)
// and C the diagonally pivoted semidefinite Cholesky factor (pgps_philox.h psd_chol_columns).  Every step is the affine map a_k = (E_k, h_k),
// h_k = g_k + C(L_k) z_k (the last one (0, h_{N-1})), composed by (E_a, h_a) (x) (E_b, h_b) = (E_a E_b, E_a h_b + h_a) --
// smth_combine without its L part -- and x_k is the h of the suffix aggregate that starts at step k.
//
// The lane-chunk structure of the smoother (pgps_kernels.hip.h), two launches per call:
//   k_sample_reduce  each lane composes its chunk's elements into (E_tot, h_tot[SG]); workgroup suffix scan -> lane
//                    suffixes (lsuf) + one record per workgroup (spine)
//   k_sample_apply   folds the spine entries to its right and its lane suffix into x at the first step after the chunk,
//                    then walks the chunk backwards: x_k = E_k x_{k+1} + h_k, writes x_k (or H x_k)
// A lane carries a GROUP of SG samples next to one (E_k, g_k, C(L_k)): the element is built once per group and step, and
// grid.y covers the ceil(S / SG) groups, so the inputs are read 2 ceil(S / SG) times per call, never once per sample.
// The draws are regenerated in both kernels from (seed, s0 + s, k, i), never stored.  What a sample computes depends on
// its own draws only, never on which other samples share its group (the same instructions for every slot of a group).
#pragma once

#include "pgps_kernels.hip.h"
#include "pgps_philox.h"

namespace pgps {

// samples per group: the record (E, h[SG]) and the walk's SG states stay in registers (no scratch at any (dtype, d):
// DESIGN.md 4o has the resource report)
template <typename T, int D>
struct SampleGroup {
    static constexpr int SG = D <= 2 ? 8 : (D <= 4 ? 4 : 2);
};

template <typename T, int D, int SG>
struct SampElem {           // x -> E x + h_j for each of the SG samples
    T E[D * D];
    T h[SG * D];
};

template <typename T, int D, int SG>
__device__ __forceinline__ void pack(const SampElem<T, D, SG>& e, T* v) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) v[i] = e.E[i];
#pragma unroll
    for (int i = 0; i < SG * D; ++i) v[D * D + i] = e.h[i];
}
template <typename T, int D, int SG>
__device__ __forceinline__ void unpack(const T* v, SampElem<T, D, SG>& e) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) e.E[i] = v[i];
#pragma unroll
    for (int i = 0; i < SG * D; ++i) e.h[i] = v[D * D + i];
}

template <typename T, int D, int SG>
struct ElemTraits<SampElem<T, D, SG>> {
    static constexpr int N = D * D + SG * D;
    using Scalar = T;
    __device__ static __forceinline__ void identity(SampElem<T, D, SG>& e) {
#pragma unroll
        for (int i = 0; i < D * D; ++i) e.E[i] = T(0);
#pragma unroll
        for (int i = 0; i < D; ++i) e.E[i * D + i] = T(1);
#pragma unroll
        for (int i = 0; i < SG * D; ++i) e.h[i] = T(0);
    }
    // time order: `a` is the earlier map, (a (x) b)(x) = a(b(x))
    __device__ static __forceinline__ void combine(const SampElem<T, D, SG>& a, const SampElem<T, D, SG>& b,
                                                   SampElem<T, D, SG>& o) {
        mat_mul<T, D>(a.E, b.E, o.E);
#pragma unroll
        for (int j = 0; j < SG; ++j) {
            T v[D];
            mat_vec<T, D>(a.E, b.h + j * D, v);
#pragma unroll
            for (int i = 0; i < D; ++i) o.h[j * D + i] = v[i] + a.h[j * D + i];
        }
    }
};

// (E_k, g_k, L_k) of step k: the smoothing element (smth_element, from F_{k+1}, Q_{k+1}, fm_k, fP_k), or (0, fm, fP) at the
// last step.  L packed symmetric; the return value is the scale of its factor's threshold, max_i fP_ii.
template <typename T, int D>
__device__ __forceinline__ T sample_element(const SampleArgs<T>& a, long k, T* E, T* g, T* L) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM;
    MeanCov<T, D> f;
    T Pf[MAT];
    load_rec<T, D>(a.fms + k * D, f.m);
    load_rec<T, MAT>(a.fPs + k * MAT, Pf);
    sym_from_full<T, D>(Pf, f.P);
    if (k + 1 < a.N) {
        T F[MAT], Qf[MAT], Q[SYM], mp[D], Pp[SYM], FP[MAT];
        load_rec<T, MAT>(a.Fs + (k + 1) * MAT, F);
        load_rec<T, MAT>(a.Qs + (k + 1) * MAT, Qf);
        sym_from_full<T, D>(Qf, Q);
        mat_vec<T, D>(F, f.m, mp);
        predict_cov<T, D>(F, f.P, Q, FP, Pp);
        SmthElem<T, D> e;
        smth_element(f, mp, Pp, FP, e);
#pragma unroll
        for (int i = 0; i < MAT; ++i) E[i] = e.E[i];
#pragma unroll
        for (int i = 0; i < D; ++i) g[i] = e.g[i];
#pragma unroll
        for (int i = 0; i < SYM; ++i) L[i] = e.L[i];
    } else {
#pragma unroll
        for (int i = 0; i < MAT; ++i) E[i] = T(0);
#pragma unroll
        for (int i = 0; i < D; ++i) g[i] = f.m[i];
#pragma unroll
        for (int i = 0; i < SYM; ++i) L[i] = f.P[i];
    }
    return max_diag<T, D>(f.P);
}

// h = g + C(L) z of the group's SG samples at step k (slots past S get z = 0; nothing of theirs is written).  The factor
// is never stored: each of its columns is added to the SG offsets as it comes out (a full D x D C next to the record would
// not fit the registers of fp64 d = 6).  L is consumed.
template <typename T, int D, int SG>
__device__ __forceinline__ void sample_offsets(const SampleArgs<T>& a, long k, int s_first, const T* g, T* L, T scale, T* h) {
    T z[SG * D];
#pragma unroll
    for (int j = 0; j < SG; ++j) {
        const int s = s_first + j;
        if (s >= a.S) {
#pragma unroll
            for (int i = 0; i < D; ++i) z[j * D + i] = T(0);
        } else if (a.z) {
#pragma unroll
            for (int i = 0; i < D; ++i) z[j * D + i] = a.z[((long)s * a.N + k) * D + i];
        } else {
            normal_vec<T, D>(a.seed, k, (uint32_t)(a.s0 + s), z + j * D);
        }
#pragma unroll
        for (int i = 0; i < D; ++i) h[j * D + i] = g[i];
    }
    psd_chol_columns<T, D>(L, scale, [&](int col, const T* c) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < SG; ++j) {
#pragma unroll
            for (int i = 0; i < D; ++i) h[j * D + i] += c[i] * z[j * D + col];
        }
    });
}

template <typename T, int D>
__global__ __launch_bounds__(kBlock) void k_sample_reduce(const SampleArgs<T> a) {
    constexpr int SG = SampleGroup<T, D>::SG, MAT = D * D;
    using SE = SampElem<T, D, SG>;
    using TR = ElemTraits<SE>;
    __shared__ T lds[kWaves * TR::N];
    const int grp = blockIdx.y;
    const long gt = (long)blockIdx.x * kBlock + threadIdx.x;
    const long k0 = gt * a.Lc;
    const long k1 = min(a.N, k0 + a.Lc);
    SE acc;
    TR::identity(acc);
    for (long k = k0; k < k1; ++k) {
        SE e, r;
        T g[D], L[Dim<D>::SYM];
        const T scale = sample_element<T, D>(a, k, e.E, g, L);
        sample_offsets<T, D, SG>(a, k, grp * SG, g, L, scale, e.h);
        TR::combine(acc, e, r);
        acc = r;
    }
    SE excl, total;
    block_scan_exclusive<SE, false>(acc, excl, total, lds);
    ws_store(a.lsuf + (long)grp * TR::N * a.nlanes, a.nlanes, gt, excl);
    if (threadIdx.x == 0) rec_store(a.spine + ((long)grp * a.nblocks + blockIdx.x) * TR::N, total);
}

template <typename T, int D>
__global__ __launch_bounds__(kBlock) void k_sample_apply(const SampleArgs<T> a) {
    constexpr int SG = SampleGroup<T, D>::SG, MAT = D * D;
    using SE = SampElem<T, D, SG>;
    using TR = ElemTraits<SE>;
    __shared__ T lds[kWaves * TR::N];
    const int grp = blockIdx.y;
    const long gt = (long)blockIdx.x * kBlock + threadIdx.x;
    const long k0 = gt * a.Lc;
    const long k1 = min(a.N, k0 + a.Lc);
    const T* spine = a.spine + (long)grp * a.nblocks * TR::N;
    const bool has_right = (int)blockIdx.x + 1 < a.nblocks;         // (uniform over the workgroup)
    SE right_part, ls;
    if (has_right) fold_spine_partial<SE>(spine, (int)blockIdx.x + 1, a.nblocks, right_part);
    ws_load(a.lsuf + (long)grp * TR::N * a.nlanes, a.nlanes, gt, ls);
    // x at the first step after this workgroup: the h of the workgroups to the right (their aggregate holds the last
    // step, E = 0); nothing after the last workgroup
    T x[SG * D];
#pragma unroll
    for (int i = 0; i < SG * D; ++i) x[i] = T(0);
    if (has_right) {
        SE right;
        block_reduce_ordered(right_part, right, lds);
#pragma unroll
        for (int i = 0; i < SG * D; ++i) x[i] = right.h[i];
    }
    // ... after this lane's chunk
#pragma unroll
    for (int j = 0; j < SG; ++j) {
        T v[D];
        mat_vec<T, D>(ls.E, x + j * D, v);
#pragma unroll
        for (int i = 0; i < D; ++i) x[j * D + i] = v[i] + ls.h[j * D + i];
    }
    const int s_first = grp * SG;
    const int width = a.proj ? 1 : D;
    for (long k = k1 - 1; k >= k0; --k) {
        T E[MAT], g[D], L[Dim<D>::SYM], h[SG * D];
        const T scale = sample_element<T, D>(a, k, E, g, L);
        sample_offsets<T, D, SG>(a, k, s_first, g, L, scale, h);
        long col = k;
        if (a.qslot) col = a.qslot[k];
#pragma unroll
        for (int j = 0; j < SG; ++j) {
            T v[D];
            mat_vec<T, D>(E, x + j * D, v);
#pragma unroll
            for (int i = 0; i < D; ++i) x[j * D + i] = v[i] + h[j * D + i];
            const int s = s_first + j;
            if (s < a.S && col >= 0) {
                T* o = a.out + ((long)s * a.out_rows + col) * width;
                if (a.proj) {
                    T acc = T(0);
#pragma unroll
                    for (int i = 0; i < D; ++i) acc += a.h[i] * x[j * D + i];
                    *o = acc;
                } else {
#pragma unroll
                    for (int i = 0; i < D; ++i) o[i] = x[j * D + i];
                }
            }
        }
    }
}

// z (S, N, d) of the library's draws: one lane per (sample, step, pair of components)
template <typename T>
__global__ __launch_bounds__(256) void k_sample_normals(long N, int d, int S, long s0, unsigned long long seed, T* z) {
    const int np = (d + 1) / 2;
    const long total = (long)S * N * np;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int j = (int)(e % np);
        const long sk = e / np;
        const long k = sk % N;
        const int s = (int)(sk / N);
        T z0, z1;
        normal_pair<T>(seed, k, (uint32_t)(s0 + s), (uint32_t)j, z0, z1);
        T* o = z + ((long)s * N + k) * d;
        o[2 * j] = z0;
        if (2 * j + 1 < d) o[2 * j + 1] = z1;
    }
}

}  // namespace pgps
