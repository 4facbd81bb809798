// pgps_merge.hip.h -- the tiled merge of a sorted training series with a sorted query grid, as a body: k_merge_sorted
// (pgps_gp_api.hip) runs it on one series, k_panel_merge (pgps_panel_inst.hip) behind a per-series view of a ragged batch.
//
// As _merge_sorted (pssgp/model.py:15-55): the shorter array is scattered into the longer one at
// arange + searchsorted(longer, shorter, side="left"), so on equal times the shorter array's point
// comes first; the training series is the "longer" one when N >= K (model.py:25 swaps only if N < K).
//
// That is a stable merge in which array A = the shorter one wins ties, done here as a tiled merge path: a workgroup owns
// kMergeTile consecutive OUTPUT positions; two of its lanes find where the tile's first and last diagonals cut A and B
// (one binary search each -- per tile, not per element), the at most kMergeTile input times (and the training
// observations that go with them) come into LDS with coalesced loads, every lane finds the cut of its own four
// outputs by a binary search in LDS and merges them serially, and the merged times, observations (NaN at query rows)
// and query slots leave through LDS as whole coalesced rows.  (Before: one 20-level binary search over global memory
// and three scattered stores per element -- 40 of the 131 us of a 2^20 + 2^18 predict_f.)
#pragma once

#include "pgps_internal.h"

namespace pgps {

constexpr int kMergeItems = 4;
constexpr int kMergeTile = kBlock * kMergeItems;

template <typename T, int N>
__device__ __forceinline__ void store_vec(T* p, const T* v) {
    using V4 = __attribute__((ext_vector_type(4))) unsigned int;
    static_assert((N * sizeof(T)) % 16 == 0, "whole 16-byte pieces");
    V4 tmp[N * sizeof(T) / 16];
    __builtin_memcpy(tmp, v, N * sizeof(T));
#pragma unroll
    for (unsigned i = 0; i < N * sizeof(T) / 16; ++i) reinterpret_cast<V4*>(p)[i] = tmp[i];
}

// number of A's elements among the first `diag` outputs of merge(A, B) with A winning ties, found by the whole
// workgroup: a kBlock-ary search (every lane probes one candidate, the count of "goes before" answers narrows the range
// kBlock-fold) -- three dependent rounds of loads for 2^20 elements where a binary search takes twenty
template <typename T>
__device__ __forceinline__ long merge_path_block(const T* A, long nA, const T* B, long nB, long diag) {
    long lo = diag > nB ? diag - nB : 0, hi = diag < nA ? diag : nA;      // the answer lies in [lo, hi]
    while (hi > lo) {                                                      // (uniform: every lane holds the same range)
        const long step = (hi - lo + kBlock - 1) / kBlock;
        const long mid = lo + (long)threadIdx.x * step;
        const bool before = mid < hi && A[mid] <= B[diag - 1 - mid];      // monotone in mid: true ... true false ... false
        const long c = __syncthreads_count(before);
        const long nlo = c > 0 ? lo + (c - 1) * step + 1 : lo;
        const long nhi = lo + c * step < hi ? lo + c * step : hi;
        lo = nlo; hi = nhi;
    }
    return lo;
}

// LDS of one merging workgroup
template <typename T, bool HET>
struct MergeLds {
    T t[kMergeTile];            // A's part of the tile, then B's
    T y[kMergeTile];            // observations of the training part
    T r[HET ? kMergeTile : 1];
};

// The tile `tile` of the merge of (ts, ys[, rs]) (N) with tq (K) into ts_m, ys_m[, rs_m], qslot (N + K): the whole workgroup
// calls it.  A query row's slot is qbase + its index in tq.
// HET (pgps_gp_predict_het_*): a second payload of the training steps, rs -> rs_m, takes the road of ys (NaN at query rows)
template <typename T, bool HET>
__device__ __forceinline__ void merge_sorted_body(MergeLds<T, HET>& sh, long tile, long N, long K, const T* ts, const T* ys,
                                                  const T* tq, T* ts_m, T* ys_m, int* qslot, long qbase, const T* rs,
                                                  T* rs_m) {
    T* s_t = sh.t;
    T* s_y = sh.y;
    [[maybe_unused]] T* s_r = sh.r;
    const bool query_first = (N >= K);      // A = the queries when they are the shorter array
    const T* A = query_first ? tq : ts;
    const T* B = query_first ? ts : tq;
    const long nA = query_first ? K : N, nB = query_first ? N : K, M = N + K;
    const long d0 = tile * kMergeTile, d1 = d0 + kMergeTile < M ? d0 + kMergeTile : M;
    const long a0 = merge_path_block(A, nA, B, nB, d0), a1 = merge_path_block(A, nA, B, nB, d1);
    const long b0 = d0 - a0, b1 = d1 - a1;
    const int na = (int)(a1 - a0), nb = (int)(b1 - b0);
    for (int e = threadIdx.x; e < na + nb; e += kBlock) {
        const bool inA = e < na;
        const long g = inA ? a0 + e : b0 + (e - na);
        s_t[e] = inA ? A[g] : B[g];
        const bool training = (inA != query_first);
        s_y[e] = training ? ys[g] : (T)__builtin_nan("");
        if constexpr (HET) s_r[e] = training ? rs[g] : (T)__builtin_nan("");
    }
    __syncthreads();
    // this lane's kMergeItems consecutive outputs: cut of its first diagonal inside the tile, then a serial merge
    const int n = na + nb;
    const int ld = min((int)threadIdx.x * kMergeItems, n);
    int lo = ld > nb ? ld - nb : 0, hi = ld < na ? ld : na;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_t[mid] <= s_t[na + (ld - 1 - mid)]) lo = mid + 1; else hi = mid;
    }
    int ia = lo, ib = ld - lo;
    T rt[kMergeItems], ry[kMergeItems];
    [[maybe_unused]] T rr[kMergeItems];
    int rq[kMergeItems];
#pragma unroll
    for (int r = 0; r < kMergeItems; ++r) {
        rt[r] = T(0); ry[r] = T(0); rq[r] = -1;
        if constexpr (HET) rr[r] = T(0);
        if (ld + r < n) {
            const bool takeA = ib >= nb || (ia < na && s_t[ia] <= s_t[na + ib]);
            const int e = takeA ? ia : na + ib;
            rt[r] = s_t[e];
            ry[r] = s_y[e];
            if constexpr (HET) rr[r] = s_r[e];
            rq[r] = (takeA == query_first) ? (int)(qbase + (takeA ? a0 + ia : b0 + ib)) : -1;
            if (takeA) ++ia; else ++ib;
        }
    }
    // four consecutive outputs per lane: whole 16-byte stores.  They rely on outputs whose first element is 16-byte aligned
    // (the staging buffers are 256-byte aligned; a panel pads every series' merged slot to 256 bytes) and on whole tiles
    const long o = d0 + ld;
    if (ld + kMergeItems <= n) {
        store_vec<T, kMergeItems>(ts_m + o, rt);
        store_vec<T, kMergeItems>(ys_m + o, ry);
        store_vec<int, kMergeItems>(qslot + o, rq);
        if constexpr (HET) store_vec<T, kMergeItems>(rs_m + o, rr);
    } else {
        for (int r = 0; r < kMergeItems && ld + r < n; ++r) {
            ts_m[o + r] = rt[r]; ys_m[o + r] = ry[r]; qslot[o + r] = rq[r];
            if constexpr (HET) rs_m[o + r] = rr[r];
        }
    }
}

}  // namespace pgps
