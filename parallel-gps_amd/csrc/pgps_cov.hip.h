// pgps_cov.hip.h -- joint posterior covariance between selected steps.
//
// The backward sampler's recursion x_k = E_k x_{k+1} + h_k (h_k independent of everything later) read as a covariance:
//   Cov(x_i, x_j | ys) = E_i E_{i+1} .. E_{j-1} sP_j   for i < j,
// E_k the gain of step k's smoothing element (pgps_math.h smth_gain, from F_{k+1}, Q_{k+1}, fP_k), sP_j the smoothed covariance.
// For n selected steps sel[0] < .. < sel[n-1] that is two passes:
//
// 1. The gain products B_a = E_{sel[a]} .. E_{sel[a+1]-1}, a = 0 .. n-2: a SEGMENTED product over the N steps, taken from the
//    right as the sampler's scan is.  Element (f, E) of a range of steps: E = the product of its gains up to the first
//    selected step inside it (that step excluded), f = 1 when there is one; step k itself is (1, I) when selected, else
//    (0, E_k).  (fa, Ea) (x) (fb, Eb) = (fa | fb, fa ? Ea : Ea Eb) is associative, so it is one more ElemTraits on the
//    lane-chunk structure of the smoother (pgps_kernels.hip.h), two launches:
//      k_cov_reduce  each lane composes its chunk; workgroup suffix scan -> lane suffixes (lsuf) + one record per workgroup
//      k_cov_apply   folds the spine entries to its right and its lane suffix into the product that is open behind the
//                    chunk, walks the chunk backwards and writes B_a = E_k (product) whenever it meets selected step a
//    Only E is built per step: no g, no L, no factor, no draws.  3 d^2 values are read per step and pass.
//
// 2. The fill: out[i, j] = G_ij sP_j (projected: h^T G_ij sP_j h), G_ij = B_i .. B_{j-1}.  Lane = column j, v <- B_{i-1} v
//    walking the rows i downwards from v = sP_j h at i = j: at a fixed row the lanes of a wave write consecutive addresses
//    and B_{i-1} is wave-uniform (scalar loads).  Rows are tiled by T = 64 so that the n-step dependence of a column is
//    broken: k_cov_tile_prefix forms U_j = B_{tT-1} .. B_{j-1} (t = j / T; a wave scan per tile), which carries column j to
//    the row above its own tile, k_cov_tile_chain the products M[s][t] of whole tiles between tile t and tile s < t - 1 (one
//    lane per t, nt = n / T steps), and k_cov_fill starts every (row tile s, column tile t >= s) independently from
//    v = M[s][t] U_j sP_j h.  The lower triangle is the mirror of the upper one through an LDS tile (projected) or the
//    transposed block (states), so the output is symmetric bit for bit.
#pragma once

#include "pgps_kernels.hip.h"

namespace pgps {

// ---------------------------------------------------------------------------------------------
// pass 1: gain products between consecutive selected steps
// ---------------------------------------------------------------------------------------------
template <typename T, int D>
struct GainElem {
    T f;                    // 1: a selected step lies inside, E = the product of the gains before the first one; 0: of all
    T E[D * D];
};

template <typename T, int D>
__device__ __forceinline__ void pack(const GainElem<T, D>& e, T* v) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) v[i] = e.E[i];
    v[D * D] = e.f;
}
template <typename T, int D>
__device__ __forceinline__ void unpack(const T* v, GainElem<T, D>& e) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) e.E[i] = v[i];
    e.f = v[D * D];
}

template <typename T, int D>
struct ElemTraits<GainElem<T, D>> {
    static constexpr int N = D * D + 1;
    using Scalar = T;
    __device__ static __forceinline__ void identity(GainElem<T, D>& e) {
#pragma unroll
        for (int i = 0; i < D * D; ++i) e.E[i] = T(0);
#pragma unroll
        for (int i = 0; i < D; ++i) e.E[i * D + i] = T(1);
        e.f = T(0);
    }
    // time order: `a` covers the earlier steps.  What follows a selected step is selected away (replaced by the identity)
    // BEFORE the product, never multiplied away: it cannot reach in front of that step, whatever it holds
    __device__ static __forceinline__ void combine(const GainElem<T, D>& a, const GainElem<T, D>& b, GainElem<T, D>& o) {
        const bool cut = a.f != T(0);
        T Bm[D * D];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) Bm[i * D + j] = cut ? T(i == j) : b.E[i * D + j];
        mat_mul<T, D>(a.E, Bm, o.E);
        o.f = cut ? a.f : b.f;
    }
};

// E_k = fP_k F_{k+1}^T Pp_{k+1}^{-1}; 0 at the last step (only the product behind the last selected step holds it, and that
// one is never written)
template <typename T, int D>
__device__ __forceinline__ void cov_gain(const CovArgs<T>& a, long k, T* E) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM;
    if (k + 1 < a.N) {
        T Pf[MAT], P[SYM], F[MAT], Qf[MAT], Q[SYM], Pp[SYM], FP[MAT];
        load_rec<T, MAT>(a.fPs + k * MAT, Pf);
        load_rec<T, MAT>(a.Fs + (k + 1) * MAT, F);
        load_rec<T, MAT>(a.Qs + (k + 1) * MAT, Qf);
        sym_from_full<T, D>(Pf, P);
        sym_from_full<T, D>(Qf, Q);
        predict_cov<T, D>(F, P, Q, FP, Pp);
        smth_gain<T, D>(FP, Pp, E);
    } else {
#pragma unroll
        for (int i = 0; i < MAT; ++i) E[i] = T(0);
    }
}

template <typename T, int D>
__global__ __launch_bounds__(kBlock) void k_cov_reduce(const CovArgs<T> a) {
    constexpr int MAT = D * D;
    using GE = GainElem<T, D>;
    using TR = ElemTraits<GE>;
    __shared__ T lds[kWaves * TR::N];
    const long gt = (long)blockIdx.x * kBlock + threadIdx.x;
    const long k0 = gt * a.Lc;
    const long k1 = min(a.N, k0 + a.Lc);
    GE acc;
    TR::identity(acc);
    for (long k = k0; k < k1; ++k) {
        if (a.slot[k] >= 0) {               // the first selected step of the chunk closes its product
            acc.f = T(1);
            break;
        }
        T E[MAT], P[MAT];
        cov_gain<T, D>(a, k, E);
        mat_mul<T, D>(acc.E, E, P);
#pragma unroll
        for (int i = 0; i < MAT; ++i) acc.E[i] = P[i];
    }
    GE excl, total;
    block_scan_exclusive<GE, false>(acc, excl, total, lds);
    ws_store(a.lsuf, a.nlanes, gt, excl);
    if (threadIdx.x == 0) rec_store(a.spine + (long)blockIdx.x * TR::N, total);
}

template <typename T, int D>
__global__ __launch_bounds__(kBlock) void k_cov_apply(const CovArgs<T> a) {
    constexpr int MAT = D * D;
    using GE = GainElem<T, D>;
    using TR = ElemTraits<GE>;
    __shared__ T lds[kWaves * TR::N];
    const long gt = (long)blockIdx.x * kBlock + threadIdx.x;
    const long k0 = gt * a.Lc;
    const long k1 = min(a.N, k0 + a.Lc);
    const bool has_right = (int)blockIdx.x + 1 < a.nblocks;         // (uniform over the workgroup)
    GE right_part, ls, acc;
    if (has_right) fold_spine_partial<GE>(a.spine, (int)blockIdx.x + 1, a.nblocks, right_part);
    ws_load(a.lsuf, a.nlanes, gt, ls);
    if (has_right) {
        GE right;
        block_reduce_ordered(right_part, right, lds);
        TR::combine(ls, right, acc);
    } else {
        acc = ls;
    }
    // acc.E = the product of the gains from step k1 up to the next selected step (behind the last one: never written)
    for (long k = k1 - 1; k >= k0; --k) {
        T E[MAT], P[MAT];
        cov_gain<T, D>(a, k, E);
        mat_mul<T, D>(E, acc.E, P);
        const int s = a.slot[k];
        if (s >= 0 && s < a.n - 1) store_rec<T, MAT>(a.B + (long)s * MAT, P);
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) acc.E[i * D + j] = s >= 0 ? T(i == j) : P[i * D + j];
    }
}

// ---------------------------------------------------------------------------------------------
// pass 2: the fill
// ---------------------------------------------------------------------------------------------
template <typename T, int D>
struct MatElem {
    T E[D * D];
};
template <typename T, int D>
__device__ __forceinline__ void pack(const MatElem<T, D>& e, T* v) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) v[i] = e.E[i];
}
template <typename T, int D>
__device__ __forceinline__ void unpack(const T* v, MatElem<T, D>& e) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) e.E[i] = v[i];
}
template <typename T, int D>
struct ElemTraits<MatElem<T, D>> {
    static constexpr int N = D * D;
    using Scalar = T;
    __device__ static __forceinline__ void identity(MatElem<T, D>& e) {
#pragma unroll
        for (int i = 0; i < D * D; ++i) e.E[i] = T(0);
#pragma unroll
        for (int i = 0; i < D; ++i) e.E[i * D + i] = T(1);
    }
    __device__ static __forceinline__ void combine(const MatElem<T, D>& a, const MatElem<T, D>& b, MatElem<T, D>& o) {
        mat_mul<T, D>(a.E, b.E, o.E);
    }
};

// U_j = B_{tT-1} B_{tT} .. B_{j-1} for the columns j of tile t = blockIdx.x + 1 (tile 0 has no row above it): one wave
// per tile, an inclusive scan of the 64 factors
template <typename T, int D>
__global__ __launch_bounds__(kCovTile) void k_cov_tile_prefix(const CovFillArgs<T> a) {
    constexpr int MAT = D * D;
    using ME = MatElem<T, D>;
    const int lane = threadIdx.x;
    const long j = ((long)blockIdx.x + 1) * kCovTile + lane;
    ME e;
    ElemTraits<ME>::identity(e);
    if (j < a.n) load_rec<T, MAT>(a.B + (j - 1) * MAT, e.E);       // 1 <= j <= n - 1: B_{j-1} exists
    wave_scan_inclusive<ME, true>(e, lane);
    if (j < a.n) store_rec<T, MAT>(a.U + j * MAT, e.E);
}

// M[s][t] = W_{s+1} W_{s+2} .. W_{t-1}, W_q = U_{(q+1)T-1} the product over the whole of tile q: what carries a column from
// the row above tile t to the top row of tile s.  One lane per t >= 2, s = t - 2 .. 0; M[t-1][t] = I is not stored.
template <typename T, int D>
__global__ __launch_bounds__(kCovTile) void k_cov_tile_chain(const CovFillArgs<T> a) {
    constexpr int MAT = D * D;
    const int t = (int)(blockIdx.x * kCovTile + threadIdx.x) + 2;
    if (t >= a.nt) return;
    T acc[MAT], Wn[MAT];
#pragma unroll
    for (int i = 0; i < MAT; ++i) acc[i] = T(0);
#pragma unroll
    for (int i = 0; i < D; ++i) acc[i * D + i] = T(1);
    load_rec<T, MAT>(a.U + ((long)t * kCovTile - 1) * MAT, Wn);                 // W_{t-1}: tile t - 1 is whole
    for (int s = t - 2; s >= 0; --s) {
        T W[MAT], r[MAT];
#pragma unroll
        for (int i = 0; i < MAT; ++i) W[i] = Wn[i];
        if (s > 0) load_rec<T, MAT>(a.U + ((long)(s + 1) * kCovTile - 1) * MAT, Wn);   // the next factor, before this one is used
        mat_mul<T, D>(W, acc, r);
#pragma unroll
        for (int i = 0; i < MAT; ++i) acc[i] = r[i];
        store_rec<T, MAT>(a.M + ((long)s * a.nt + t) * MAT, acc);
    }
}

// out = A V, A (D, D), V (D, W)
template <typename T, int D, int W>
__device__ __forceinline__ void mat_mul_dw(const T* A, const T* V, T* out) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int c = 0; c < W; ++c) {
            T acc = T(0);
#pragma unroll
            for (int k = 0; k < D; ++k) acc += A[i * D + k] * V[k * W + c];
            out[i * W + c] = acc;
        }
}

// One wave per (row tile s = blockIdx.y, column tile t = blockIdx.x), s <= t.  PROJ: v (D) = G sP_j h, out (n, n), the mirror
// through an LDS tile; else V (D, D) = G sP_j, out (n, n, D, D), the mirror block transposed.
template <typename T, int D, bool PROJ>
__global__ __launch_bounds__(kCovTile) void k_cov_fill(const CovFillArgs<T> a) {
    constexpr int MAT = D * D, W = PROJ ? 1 : D, TT = kCovTile;
    const int s = blockIdx.y, t = blockIdx.x;
    if (s > t) return;
    __shared__ T tile[PROJ ? TT * (TT + 1) : 1];
    const int r = threadIdx.x;
    const long j = (long)t * TT + r;
    const bool col = j < a.n;
    const long jc = col ? j : a.n - 1;                              // lanes past the last column compute it again, write nothing
    T V0[D * W], V[D * W];
    {
        T P[MAT];
        load_rec<T, MAT>(a.sP + jc * MAT, P);
        if constexpr (PROJ) {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                T acc = T(0);
#pragma unroll
                for (int k = 0; k < D; ++k) acc += T(0.5) * (P[i * D + k] + P[k * D + i]) * a.h[k];
                V0[i] = acc;
            }
        } else {
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int k = 0; k < D; ++k) V0[i * D + k] = T(0.5) * (P[i * D + k] + P[k * D + i]);
        }
    }
#pragma unroll
    for (int i = 0; i < D * W; ++i) V[i] = T(0);
    if (s < t) {
        T U[MAT];
        load_rec<T, MAT>(a.U + jc * MAT, U);
        mat_mul_dw<T, D, W>(U, V0, V);
        if (s < t - 1) {                                            // (uniform)
            T M[MAT], X[D * W];
            load_rec<T, MAT>(a.M + ((long)s * a.nt + t) * MAT, M);
            mat_mul_dw<T, D, W>(M, V, X);
#pragma unroll
            for (int i = 0; i < D * W; ++i) V[i] = X[i];
        }
    }
    const long i_lo = (long)s * TT;
    const long i_hi = min(a.n, i_lo + TT) - 1;
    for (long i = i_hi; i >= i_lo; --i) {                           // (uniform)
        if (s == t) {
#pragma unroll
            for (int q = 0; q < D * W; ++q) V[q] = i == j ? V0[q] : V[q];
        }
        const bool live = col && i <= j;
        if constexpr (PROJ) {
            T c = T(0);
#pragma unroll
            for (int q = 0; q < D; ++q) c += a.h[q] * V[q];
            tile[(int)(i - i_lo) * (TT + 1) + r] = c;
            if (live) a.out[i * a.n + j] = c;
        } else if (live) {
            store_rec<T, MAT>(a.out + (i * a.n + j) * MAT, V);
            if (i < j) {
                T Vt[MAT];
#pragma unroll
                for (int p = 0; p < D; ++p)
#pragma unroll
                    for (int q = 0; q < D; ++q) Vt[p * D + q] = V[q * D + p];
                store_rec<T, MAT>(a.out + (j * a.n + i) * MAT, Vt);
            }
        }
        if (i > i_lo) {
            T B[MAT], X[D * W];
            load_rec<T, MAT>(a.B + (i - 1) * MAT, B);               // wave-uniform address
            mat_mul_dw<T, D, W>(B, V, X);
#pragma unroll
            for (int q = 0; q < D * W; ++q) V[q] = X[q];
        }
    }
    if constexpr (PROJ) {
        __syncthreads();
        // row (t T + c) of the output, columns s T + r: the transposed tile, strictly below the diagonal
        const long i = i_lo + r;
        const int nc = (int)(min(a.n, ((long)t + 1) * TT) - (long)t * TT);
        for (int c = 0; c < nc; ++c) {
            const long jj = (long)t * TT + c;
            if (i <= i_hi && i < jj) a.out[jj * a.n + i] = tile[r * (TT + 1) + c];
        }
    }
}

}  // namespace pgps
