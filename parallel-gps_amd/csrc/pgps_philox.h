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

// Lower semidefinite Cholesky factor of M (symmetric, packed upper triangle), plain column (Crout) order: a column whose
// pivot p = M_jj - sum_l C_jl^2 is not above tau = D eps scale is zero -- zeros for the singular factors of repeated
// times, query times equal to training times and noise-free (Periodic) transitions, never NaN.  C full D x D, row-major.
// scale = max_i P_ii of the filtered covariance M was computed from: L = P - E F P carries rounding of P's size, and a
// pivot of that size must not pass (at a repeated time L is rounding only, and a threshold relative to L's own diagonal
// let such a pivot through and divided L's other rounding residues by its square root).  At the last step M = P.
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

template <typename T, int D>
PGPS_HD void psd_chol(const T* M, T scale, T* C) {
    const T tau = T(D) * CholEps<T>::v * scale;
#pragma unroll
    for (int i = 0; i < D * D; ++i) C[i] = T(0);
#pragma unroll
    for (int j = 0; j < D; ++j) {
        T p = M[symi<D>(j, j)];
#pragma unroll
        for (int l = 0; l < j; ++l) p -= C[j * D + l] * C[j * D + l];
        if (p > tau) {
            const T c = std::sqrt(p);
            C[j * D + j] = c;
#pragma unroll
            for (int i = j + 1; i < D; ++i) {
                T q = M[symi<D>(i, j)];
#pragma unroll
                for (int l = 0; l < j; ++l) q -= C[i * D + l] * C[j * D + l];
                C[i * D + j] = q / c;
            }
        }
    }
}

}  // namespace pgps
