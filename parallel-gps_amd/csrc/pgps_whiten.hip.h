// pgps_whiten.hip.h -- whitened columns of the multi-column Kalman pass and their Gram matrix (pgps_gp_whiten_multi_f64,
// pgps_gp_gram_multi_f64).
//
// With K_y = K + R I = L L^T on the observed rows in time order, the standardised innovations of column c,
//   w[k, c] = (ys[k, c] - mu_c[k]) / sqrt(S_k),
// are W = L^-1 ys, and G = W^T W = ys^T K_y^-1 ys.  For ys = [y, phi_1 .. phi_p] the (1 + p)^2 entries of G hold the
// likelihood at any trend coefficients, its gradient, the GLS estimate and its covariance.
//
//   k_gpm_whiten   k_gpm_apply<D, MC, false> (pgps_multi.hip.h: same spine, lane prefixes, column groups on blockIdx.y, rounds
//                  with their own c_base) that also stores w[k, c0 : c0 + nc] -- 0.0 at a step that is not observed: the
//                  array is scratch and is not zeroed -- and, from the group that holds column 0, the workgroup's
//                  sum of log S_k and its count of observed steps.  It writes no log-likelihood partials.
//   k_gram_partial one workgroup per slab of kGramSlab rows of W.  Column tiles of 8 / 4 / 2 columns sit in different
//                  workgroups of the scan, so a product of two columns cannot be formed there: W goes through memory once.
//                  The slab is staged through LDS in tiles of kGramTile rows, 16 columns wide (0.0 beyond M and beyond the
//                  slab's last row); a thread owns a 4 x 4 block of G (the 10 blocks on or above the diagonal) for one of
//                  16 row phases: 8 LDS doubles per 16 FMAs.  N M 8 bytes against 2 N M^2 flops: memory-bound at M <= 16.
//   k_gram_finalize one workgroup per entry i <= j sums the partial records in a fixed order and writes G[i, j] and G[j, i]
//                  from the one sum.
// No floating-point atomics: results repeat bit for bit.  fp64, d <= 3.
#pragma once

#include "pgps_multi.hip.h"

namespace pgps {

template <int D, int MC>
__global__ __launch_bounds__(kBlock) void k_gpm_whiten(const GpMultiArgs a, const GpWhitenOut o) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM;
    using FE = FiltElemM<double, D, MC>;
    using MS = MeanCovM<double, D, MC>;
    __shared__ double lds[kWaves * FE::N];
    __shared__ double lds_ll[kWaves];
    const MultiGroup q = multi_group<MC>(a);
    const double* spine = a.spine + (long)q.g * a.nblocks * FE::N;
    const bool wvec = q.vec && o.w_aligned;     // (q.vec: MC even, the group whole, M even -- so every row of w is aligned too)

    double h[D];
    MS s;
    gp_prior<double, D>(a.m, h, s.P);
#pragma unroll
    for (int c = 0; c < MC; ++c)
#pragma unroll
        for (int i = 0; i < D; ++i) s.m[c][i] = 0.0;

    const long gt = (long)blockIdx.x * kBlock + threadIdx.x;
    const long k0 = gt * a.Lc;
    const long k1 = min(a.N, k0 + a.Lc);

    FE left_part, lp;
    if (blockIdx.x > 0) fold_spine_partial<FE>(spine, 0, (int)blockIdx.x, left_part);
    ws_load(a.lpre + (long)q.g * a.nlanes * FE::N, a.nlanes, gt, lp);
    if (blockIdx.x > 0) {
        FE left;
        block_reduce_ordered(left_part, left, lds);
        filt_apply_m(s, left);
    }
    filt_apply_m(s, lp);

    LogLikM<MC> ll;
    if (k0 < k1) {
        double tprev = (k0 > 0) ? a.m.ts[k0 - 1] : a.m.t_prev;
        double tn = a.m.ts[k0], yn[MC];
        bool on = multi_load_y<MC>(a, q, k0, yn);
        for (long k = k0; k < k1; ++k) {
            const double t = tn;
            const bool obs = on;
            double y[MC];
#pragma unroll
            for (int c = 0; c < MC; ++c) y[c] = yn[c];
            if (k + 1 < k1) { tn = a.m.ts[k + 1]; on = multi_load_y<MC>(a, q, k + 1, yn); }
            double F[MAT], Qf[MAT], Q[SYM];
            lti_step<double, D>(a.m, t - tprev, F, Qf);
            sym_from_full<double, D>(Qf, Q);
            tprev = t;
            double mp[MC][D], Pp[SYM], FP[MAT], r[MC], S = 1.0;
#pragma unroll
            for (int c = 0; c < MC; ++c) r[c] = 0.0;
            kf_step_m<double, D, MC>(s, F, Q, y, obs, h, a.R, k == 0, ll, mp, Pp, FP, r, &S);
            const double is = recip(sqrt(S));
            double wv[MC];
#pragma unroll
            for (int c = 0; c < MC; ++c) wv[c] = obs ? r[c] * is : 0.0;
            double* pw = o.w + k * o.ldw + q.c0;
            if (wvec) {
                store_rec<double, MC>(pw, wv);
            } else {
#pragma unroll
                for (int c = 0; c < MC; ++c)
                    if (c < q.nc) pw[c] = wv[c];
            }
        }
    }
    // log S_k and the count are the same in every group: the group that holds column 0 hands them out
    const double ld = block_sum_double(std::log(ll.mant) + double(ll.expo) * 0.6931471805599453, lds_ll);
    const double cnt = block_sum_double(double(ll.count), lds_ll);
    if (threadIdx.x == 0 && q.c0 == 0) {
        o.ldpart[blockIdx.x] = ld;
        o.ldpart[(long)a.nblocks + blockIdx.x] = cnt;
    }
}

// one workgroup: logdet and the number of observed steps from the workgroups' partials, in a fixed order
static __global__ __launch_bounds__(kBlock) void k_whiten_finalize(const double* ldpart, int nblocks, double* logdet, long* n_obs) {
    __shared__ double lds_ll[kWaves];
    double v = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kBlock) { v += ldpart[i]; c += ldpart[(long)nblocks + i]; }
    const double tv = block_sum_double(v, lds_ll);
    const double tc = block_sum_double(c, lds_ll);
    if (threadIdx.x == 0) {
        if (logdet) *logdet = tv;
        if (n_obs) *n_obs = (long)tc;           // (a sum of integers below 2^53: exact)
    }
}

// ---------------------------------------------------------------------------------------------
// Gram matrix of W (N, M), M <= M_MAX = 16
// ---------------------------------------------------------------------------------------------
constexpr int kGramTile = 128;          // rows of W in LDS at a time: 16 KiB at 16 columns
constexpr int kGramBlk = 4;             // a thread's block of G is kGramBlk x kGramBlk
constexpr int kGramPhases = 16;         // row phases: thread = phase * 16 + block slot
constexpr int kGramRec = kGramMax * kGramMax;       // doubles of a partial record: G (16, 16), its blocks on or above the diagonal
static_assert(kGramSlab % kGramTile == 0 && kGramTile % kGramPhases == 0, "whole tiles per slab, whole phases per tile");
static_assert(kBlock == 256, "k_gram_partial: 16 row phases x 16 block slots");

// block slot -> (bi, bj), bi <= bj, of the 4 x 4 grid of blocks; false for the 6 slots that have none
__device__ __forceinline__ bool gram_slot(int slot, int* bi, int* bj) {
    int s = slot, i = 0;
    for (; i < 4; ++i) {
        if (s < 4 - i) break;
        s -= 4 - i;
    }
    *bi = i;
    *bj = i + s;
    return i < 4;
}

template <int M_MAX>
__global__ __launch_bounds__(kBlock) void k_gram_partial(const double* __restrict__ w, long N, int M, double* __restrict__ part) {
    static_assert(M_MAX == 16, "the block grid and the partial record are laid out for 16 columns");
    constexpr int PER = kGramTile * M_MAX / kBlock;         // doubles a thread stages per tile
    __shared__ alignas(16) double tile[kGramTile * M_MAX];
    __shared__ double red[kWaves * 16 * kGramBlk * kGramBlk];
    const int tid = threadIdx.x, slot = tid & 15, phase = tid >> 4;
    int bi, bj;
    const bool have = gram_slot(slot, &bi, &bj) && bj * kGramBlk < M;
    const long r0 = (long)blockIdx.x * kGramSlab;
    const long r1 = min(N, r0 + kGramSlab);

    double acc[kGramBlk][kGramBlk];
#pragma unroll
    for (int i = 0; i < kGramBlk; ++i)
#pragma unroll
        for (int j = 0; j < kGramBlk; ++j) acc[i][j] = 0.0;

    // element e of a tile: row e / 16, column e % 16; 0.0 beyond the slab's last row and beyond column M
    auto fetch = [&](long t0, double* v) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + i * kBlock;
            const long row = t0 + (e >> 4);
            const int col = e & 15;
            v[i] = (row < r1 && col < M) ? w[row * (long)M + col] : 0.0;
        }
    };
    double v[PER];
    fetch(r0, v);
    for (long t0 = r0; t0 < r1; t0 += kGramTile) {
        __syncthreads();                        // the tile before this one has been read
#pragma unroll
        for (int i = 0; i < PER; ++i) tile[tid + i * kBlock] = v[i];
        __syncthreads();
        if (t0 + kGramTile < r1) fetch(t0 + kGramTile, v);          // the next tile's loads under this tile's products
        if (have) {
#pragma unroll 4
            for (int r = phase; r < kGramTile; r += kGramPhases) {
                double x[kGramBlk], y[kGramBlk];
                load_rec<double, kGramBlk>(&tile[r * M_MAX + bi * kGramBlk], x);
                load_rec<double, kGramBlk>(&tile[r * M_MAX + bj * kGramBlk], y);
#pragma unroll
                for (int i = 0; i < kGramBlk; ++i)
#pragma unroll
                    for (int j = 0; j < kGramBlk; ++j) acc[i][j] += x[i] * y[j];
            }
        }
    }
    // the 16 row phases of a slot: 4 inside a wave (lanes 16 and 32 apart), then the 4 waves through LDS, in a fixed order
    const int lane = tid & (kWave - 1), wave = tid / kWave;
#pragma unroll
    for (int i = 0; i < kGramBlk; ++i)
#pragma unroll
        for (int j = 0; j < kGramBlk; ++j) {
            double t = acc[i][j];
            t += __shfl_down(t, 32, kWave);
            t += __shfl_down(t, 16, kWave);
            if (lane < 16) red[(wave * 16 + slot) * (kGramBlk * kGramBlk) + i * kGramBlk + j] = t;
        }
    __syncthreads();
    // thread = (slot, element of its block): the record is G (16, 16) row-major; the blocks below the diagonal are not written
    // (and not read: k_gram_finalize takes i <= j)
    {
        const int s2 = tid >> 4, e = tid & 15, i = e >> 2, j = e & 3;
        int ci, cj;
        const bool own = gram_slot(s2, &ci, &cj);
        double t = 0.0;
#pragma unroll
        for (int wv = 0; wv < kWaves; ++wv) t += red[(wv * 16 + s2) * (kGramBlk * kGramBlk) + e];
        if (own) part[(long)blockIdx.x * kGramRec + (ci * kGramBlk + i) * M_MAX + cj * kGramBlk + j] = t;
    }
}

// one workgroup per entry (i, j), i <= j < M, of G: its lanes take the partial records' (i, j) in slab order, 256 apart, and the
// workgroup's sum (block_sum_double: a fixed tree) is written to G[i, j] and G[j, i] -- as k_gpb_finalize sums a model's partials
static __global__ __launch_bounds__(kBlock) void k_gram_finalize(const double* __restrict__ part, long nparts, int M, double* __restrict__ gram) {
    __shared__ double lds_ll[kWaves];
    const int i = (int)blockIdx.x >> 4, j = (int)blockIdx.x & 15;
    if (i > j || j >= M) return;
    double v = 0.0;
    for (long p = threadIdx.x; p < nparts; p += kBlock) v += part[p * kGramRec + i * kGramMax + j];
    const double t = block_sum_double(v, lds_ll);
    if (threadIdx.x == 0) {
        gram[i * M + j] = t;
        gram[j * M + i] = t;
    }
}

}  // namespace pgps
