// pgps_philox.h -- the library's standard normal draws: a counter-based generator, so that the draw of (sample s, step k,
// component i) is a fixed function of the seed and those indices -- whatever the launch geometry, the kernel family, the
// chunk size or the host / device side that regenerates it.
//
//   words  = Philox4x32-10, key (lo32(seed), hi32(seed)), counter (lo32(k), hi32(k), s, i / 2)
//   u, v   = 53-bit uniforms in (0, 1) from (w0, w1) and (w2, w3):  ((w0 << 21 | w1 >> 11) + 0.5) 2^-53
//   z_2j   = sqrt(-2 ln u) cos(2 pi v),  z_2j+1 = sqrt(-2 ln u) sin(2 pi v)        (Box-Muller; the last sine dropped at odd d)
//
// fp32 draws round the fp64 uniforms and run Box-Muller in float: they are the fp64 draws to float precision.
// Accurate library log / sqrt / sin / cos on both sides (not the __ intrinsics).  Compiles as plain C++ too (the host twin).
#pragma once

#include <cmath>
#include <cstdint>

#include "pgps_math.h"

namespace pgps {

struct Philox4 {
    uint32_t w[4];
};

PGPS_HD uint32_t philox_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

// Philox4x32 with 10 rounds (Salmon et al., SC'11; the constants of Random123)
PGPS_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = philox_mulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = philox_mulhi(M1, c2), lo1 = M1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

PGPS_HD double philox_u53(uint32_t a, uint32_t b) {
    const uint64_t m = ((uint64_t)a << 21) | (uint64_t)(b >> 11);
    return ((double)m + 0.5) * 0x1p-53;
}

template <typename T> struct TwoPi;
template <> struct TwoPi<double> { static constexpr double v = 6.283185307179586476925286766559; };
template <> struct TwoPi<float> { static constexpr float v = 6.283185307179586476925286766559f; };

// the pair (z_2j, z_2j+1) of sample s, step k, under seed
template <typename T>
PGPS_HD void normal_pair(unsigned long long seed, long k, uint32_t s, uint32_t j, T& z0, T& z1) {
    const Philox4 r = philox4x32_10((uint32_t)(uint64_t)k, (uint32_t)((uint64_t)k >> 32), s, j, (uint32_t)seed,
                                    (uint32_t)(seed >> 32));
    const T u = (T)philox_u53(r.w[0], r.w[1]);
    const T v = (T)philox_u53(r.w[2], r.w[3]);
    const T rad = std::sqrt(T(-2) * std::log(u));
    const T a = TwoPi<T>::v * v;
    z0 = rad * std::cos(a);
    z1 = rad * std::sin(a);
}

// all D components of sample s at step k
template <typename T, int D>
PGPS_HD void normal_vec(unsigned long long seed, long k, uint32_t s, T* z) {
#pragma unroll
    for (int j = 0; j < (D + 1) / 2; ++j) {
        T a, b;
        normal_pair<T>(seed, k, s, (uint32_t)j, a, b);
        z[2 * j] = a;
        if (2 * j + 1 < D) z[2 * j + 1] = b;
    }
}

// Semidefinite Cholesky factor of M (symmetric, packed upper triangle) with diagonal pivoting: C C^T = M, column by
// column.  At each of the D steps the pivot is the largest remaining diagonal entry (the lowest index on ties); the
// factor stops when that entry is not above tau = (D + 3) eps scale, and the remaining columns are zero -- zeros for the singular
// factors of repeated times, query times equal to training times and noise-free (Periodic) transitions, never NaN.  With
// pivot p:  c = A[:, p] / sqrt(A[p, p]),  A -= c c^T,  A[p, p] = 0 (it is, in exact arithmetic), c the next column of C.
// C is not triangular: only C C^T matters.  Pivoting keeps the factor accurate where M is nearly singular (RBF and
// product models, float32 at d >= 3): the plain column order took rounding-sized pivots first there and drew samples whose
// covariance was wrong by a third.
// scale = max_i P_ii of the filtered covariance M was computed from: L = P - E F P carries rounding of P's size, and a
// pivot of that size must not pass (at a repeated time L is rounding only, and a threshold relative to L's own diagonal
// let such a pivot through and divided L's other rounding residues by its square root).  D eps for the D-term sums of
// E F P, 3 eps for the roundings of E itself and of the subtraction: at D = 1 those alone exceed D eps (a 2-ulp pivot
// passed at a query on a training time and moved that draw by 1e-8).  At the last step M = P.
template <typename T> struct CholEps;
template <> struct CholEps<double> { static constexpr double v = 0x1p-52; };
template <> struct CholEps<float> { static constexpr float v = 0x1p-23f; };

template <typename T, int D>
PGPS_HD T max_diag(const T* P) {
    T m = P[symi<D>(0, 0)];
#pragma unroll
    for (int i = 1; i < D; ++i) m = P[symi<D>(i, i)] > m ? P[symi<D>(i, i)] : m;
    return m;
}

// The columns of the factor, one after the other: emit(j, c) gets column j (all zero once the factor has stopped).  A is
// consumed.  The pivot column is picked by unrolled compare-and-select, never by a run-time index into A: on the device A
// lives in registers.
template <typename T, int D, typename Emit>
PGPS_HD void psd_chol_columns(T* A, T scale, Emit&& emit) {
    const T tau = T(D + 3) * CholEps<T>::v * scale;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        T best = A[symi<D>(0, 0)];
        int p = 0;
#pragma unroll
        for (int i = 1; i < D; ++i) {
            const T a = A[symi<D>(i, i)];
            const bool up = a > best;
            best = up ? a : best;
            p = up ? i : p;
        }
        const bool go = best > tau;
        const T r = go ? T(1) / std::sqrt(best) : T(0);
        T c[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            T a = A[symi<D>(i, 0)];
#pragma unroll
            for (int q = 1; q < D; ++q) a = p == q ? A[symi<D>(i, q)] : a;
            c[i] = a * r;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
#pragma unroll
            for (int k = i; k < D; ++k) A[symi<D>(i, k)] -= c[i] * c[k];
            A[symi<D>(i, i)] = (go && p == i) ? T(0) : A[symi<D>(i, i)];
        }
        emit(j, c);
    }
}

}  // namespace pgps
