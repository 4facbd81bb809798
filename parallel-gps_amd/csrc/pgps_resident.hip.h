// pgps_resident.hip.h -- filter + log-likelihood + smoother of a whole series in ONE resident launch (d <= 2).
//
// The three-launch path (pgps_kernels.hip.h) reads Fs, Qs three times -- reduce, Kalman pass, RTS pass -- and writes
// the filtered moments only to read them back: 389 real bytes per step at d = 2 fp64 where the reference's contract
// (pssgp/kalman/parallel.py:121-152, 187-201) touches each array once per function.  At 2^20 steps its streaming loops
// already run at the rate a CU's memory path sustains (10 - 13 B/clk per CU, profiles/r03_stamps_before.txt), so the
// pass gets shorter only by moving fewer bytes.  Here every workgroup keeps its 256 x LC steps ON CHIP between the
// phases of the scan and the only traffic is the contract's minimum: Fs, Qs, ys in once (72 B/step), fms, fPs, sms,
// sPs out once (96 B/step).
//
//   phase 1   stream the lane's LC steps in (coalesced, transposed through the wave's LDS slots): F stays in
//             registers, Q stays in the lane's LDS slot, y in registers; lane-serial filt_extend -> lane aggregate;
//             workgroup scan; the workgroup's total is published (write-through stores) the moment the scan has it
//   barrier 1 grid-wide (every workgroup resident: grid <= CUs, one workgroup per CU by its LDS footprint)
//   phase 2   fold the totals to the left, Kalman pass over the kept F, Q, y: fms, fPs out (through the slots Q has
//             left, drained coalesced), log-likelihood, and the smoothing element (E, g, L) of every step
//             (parallel.py:159-166) IN PLACE of the step's inputs: E, g in the registers F and y have left, L in
//             the slot; lane aggregate of the elements, workgroup suffix scan, total published; then the workgroup's
//             log-likelihood partial, while the right neighbour's total is still on its way.
//             The stores are spread under the arithmetic: the filtered P of a sub-tile (four steps per lane) leaves
//             in groups of 3, 3, 2 wave-instructions behind the first three steps of the NEXT sub-tile, its means in
//             one group of 4 at its own end; the L records of a sub-tile wait in registers until its P has left the
//             slots; the last sub-tile's P leaves around the element of the chunk's last step
//   barrier 2
//   phase 3   fold the totals to the right, lane-serial smoothing-operator pass (parallel.py:176-184) backwards over
//             the kept elements: sms, sPs out through the slots
//
// On chip per lane at d = 2 fp64, LC = 16: 64 doubles of F / E and 16 of y (later 32 of g) in registers, 512 B of
// Q / filtered P / L / smoothed P in LDS: 528 B slots x 256 lanes = 132 KiB of the CU's 160, one workgroup per CU,
// one wave per SIMD on 512 registers.
//
// Inter-workgroup visibility.  A workgroup's total travels as TAGGED GRANULES (MI355X_MICROARCH.md, price list: handoff-1to1):
// one naturally aligned 8-byte word {32 bits of the total, the launch's epoch} per 32-bit word of the total, each written by one
// lane of the publishing wave in ONE agent-scope atomic (write-through) wave-store -- the data is its own flag: no drain in
// front of a signal, no flag, no second load behind the poll.  The neighbour's lanes poll one granule each with relaxed
// agent-scope loads until its tag is the epoch, and the poll that sees the tag holds the data.  The grid-wide barriers stay
// as they were: the publishing wave drains its stores (s_waitcnt vmcnt(0)) behind the scan's tail, one lane adds an arrival to
// the counter shard of its tile; eight lanes poll one shard each; records read behind a barrier are read with agent-scope
// atomic loads only (the granules' data halves).  Every spin is bounded (status bit 1).
// Each of the two barriers of a launch counts on eight shards of its OWN (target n each): a workgroup that runs ahead --
// workgroup 0 never waits in phase 2, nor does one whose left neighbour's total has forgotten -- arrives at barrier 2
// while others are still in phase 1, and on shared counters its second arrival could stand in for a first arrival that
// has not happened (a record read before it was published).  Two sets of both alternate between launches and every
// launch zeroes the set of the next one, so nothing is memset in front of a launch and a launch that gave up leaves no
// debt.
//
// Ragged series: steps at or beyond N are padded ON LOAD with the scan's identity step (F = I, Q = 0, y = NaN: a pure
// predict that changes nothing), the element of step N - 1 is the reference's last element (0, m, P) (parallel.py:155-156)
// with E exactly zero, the padded steps' elements (about the identity, from smth_element on F = I, Q = 0) lie to its right
// and reach nothing as long as they are finite (tests/test_gpu_resident_skew.py: near-singular filtered P before the
// padding), and stores beyond N are predicated off -- one code path for the arithmetic; each group of output stores
// exists twice, for a whole wave (no predicate, the group's LDS reads issued together) and for a ragged one, behind one
// scalar branch.
#pragma once

#include <type_traits>

#include "pgps_fused.hip.h"
#include "pgps_kernels.hip.h"

namespace pgps {


template <typename T, int D, int LC>
struct ResCfg {
    static constexpr int W = (int)sizeof(T), MAT = D * D, G = 4;
    static_assert(LC % G == 0, "whole sub-tiles");
    static constexpr int S = LC / G;
    using GF = StageGeom<MAT * W, G>;               // F, Q, P records of one sub-tile: global side
    using GM = StageGeom<D * W, G>;                 // m records
    static constexpr int SLOT = LC * MAT * W + 16;  // a lane's LDS slot (LC matrix records) + 16 B: conflict-free owner reads
    static constexpr int SLOTS = kWave * SLOT;      // per wave
    static constexpr int MST = GM::BYTES > 5120 ? GM::BYTES : 5120;     // per wave: staging of the means of one sub-tile / of 64 B per lane of y, t
    static constexpr int NREC = Dim<D>::NFILT * W;                      // the largest record the scans and hand-offs pass through LDS
    static constexpr int NSCAN = (kWaves + 1) * NREC;                   // the four wave totals of a scan, and one record handed over
    static_assert(NSCAN % 8 == 0, "the log-likelihood sum's doubles follow the scan scratch");
    static constexpr int BYTES = kWaves * (SLOTS + MST) + NSCAN + kWaves * 8;
};

// Ordering of a wave's own LDS accesses (one lane writes what another lane of the SAME wave reads next): the LDS executes a
// wave's instructions in issue order, so the hardware needs nothing -- only the compiler must keep the accesses in program
// order.  wave_lds_sync() of pgps_kernels.hip.h fences at WORKGROUP scope, which on gfx950 also drains every vector-memory
// operation of the wave (s_waitcnt vmcnt(0)): each sub-tile then waited for its prefetched loads and for the previous
// sub-tile's output stores (18 such waits in the Kalman pass alone).  Wavefront scope orders without waiting.
__device__ __forceinline__ void res_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// max |A| (|E|) of a neighbouring tile's total below which its own (b, C) ((g, L)) ARE the carry: see the forgetting shortcut
template <typename T> struct ResForget;
template <> struct ResForget<double> { static constexpr double kA = 0x1p-120; };
template <> struct ResForget<float> { static constexpr float kA = 0x1p-60f; };

#define PGPS_RSTAMP(IDX)                                                                              \
    do {                                                                                              \
        if (ra.stamps && threadIdx.x == 0) ra.stamps[(long)blockIdx.x * 16 + (IDX)] = __builtin_readcyclecounter(); \
    } while (0)
// every wave's own stamp K (0 = end of its reduce, 1 = end of its Kalman pass): the (nblocks, 8) table after the stamps
// rows, [K * 4 + wave] -- the workgroup stamps above are wave 0's, which includes its wait for slower waves at a barrier
#define PGPS_RSTAMP_WAVE(K)                                                                           \
    do {                                                                                              \
        if (ra.stamps && lane == 0)                                                                   \
            ra.stamps[(long)gridDim.x * 16 + (long)blockIdx.x * 8 + (K) * kWaves + wave] = __builtin_readcyclecounter(); \
    } while (0)

// Diagnostics (pgps_debug_resident_delay): a deterministic start skew.  The armed workgroup's publishing lane waits
// `ticks` of the wall clock (constant rate, one clock for the whole chip) before it publishes the total of the armed phase,
// and wall-clock stamps go to slots 10 .. 13 of the stamps rows: 10 / 11 = the workgroup's phase-1 / phase-2 publish
// (drained, just before its arrival), 12 = the start of the wait, 13 = its length in ticks.  Only the SKEW instantiations
// of the kernel carry it (launched while the hook is armed): the default ones hold none of its code.
template <typename T>
__device__ __forceinline__ void res_skew(const ResArgs<T>& ra, int tile, int phase) {
    if (tile == ra.delay_tile && phase == ra.delay_phase) {
        const long long t0 = wall_clock64();
        ra.wstamps[(long)tile * 16 + 12] = t0;
        ra.wstamps[(long)tile * 16 + 13] = ra.delay_ticks;
        while (wall_clock64() - t0 < ra.delay_ticks) __builtin_amdgcn_s_sleep(8);
    }
}
template <typename T>
__device__ __forceinline__ void res_wstamp(const ResArgs<T>& ra, int tile, int slot) {
    if (ra.wstamps) ra.wstamps[(long)tile * 16 + slot] = wall_clock64();
}

// one 16-byte piece of an identity-step record: kind 0 = F (identity matrix), 1 = Q (zero)
template <typename T, int D>
__device__ __forceinline__ V4 res_pad_piece(int kind, int pos_in_rec) {
    constexpr int PER = 16 / (int)sizeof(T);
    T tmp[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int e = (pos_in_rec * PER + j) % (D * D);
        tmp[j] = (kind == 0 && (e / D) == (e % D)) ? T(1) : T(0);
    }
    V4 v;
    __builtin_memcpy(&v, tmp, 16);
    return v;
}

// Addressing of the transposing copies.  Piece q = v * 64 + lane of a sub-tile belongs to owner q / NV, position q % NV;
// with OPI = 64 / NV owners per wave-instruction that is owner v * OPI + lane / NV, position lane % NV: ONE lane-dependent
// 32-bit offset per array kind and a wave-uniform (scalar) part per instruction -- written out so, because left to the
// compiler every instruction of every sub-tile kept a vector address of its own alive across the phases (scratch).
//
// global -> registers: the pieces of sub-tile `sb` of one matrix array of this wave; `lim` = bytes of the array from the
// wave's first record on: pieces at or beyond it are padded with the identity step.
template <typename T, int D, typename GEO, int PITCH>
__device__ __forceinline__ void res_issue(const char* __restrict__ g /*wave-uniform*/, int sb, long lim, bool full, int kind, V4* r) {
    const int lane = threadIdx.x & (kWave - 1);
    constexpr int NV = GEO::NV, OPI = kWave / NV;
    constexpr int PPR = D * D * (int)sizeof(T) / 16 > 0 ? D * D * (int)sizeof(T) / 16 : 1;     // pieces per record
    const unsigned loff = (unsigned)(lane / NV) * PITCH + (unsigned)(lane % NV) * 16u;
    if (full) {
#pragma unroll
        for (int v = 0; v < NV; ++v) r[v] = *reinterpret_cast<const V4*>(g + ((long)sb * GEO::SEG + (long)v * OPI * PITCH) + loff);
    } else {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const long off = (long)sb * GEO::SEG + (long)v * OPI * PITCH + loff;
            if (off < lim) r[v] = *reinterpret_cast<const V4*>(g + off);
            else r[v] = res_pad_piece<T, D>(kind, (lane % NV) % PPR);
        }
    }
}
// registers -> the owners' slots
template <typename GEO, int SLOT>
__device__ __forceinline__ void res_commit(char* slots, int sb, const V4* r) {
    const int lane = threadIdx.x & (kWave - 1);
    constexpr int NV = GEO::NV, OPI = kWave / NV;
    char* base = slots + (lane / NV) * SLOT + (lane % NV) * 16;
#pragma unroll
    for (int v = 0; v < NV; ++v) *reinterpret_cast<V4*>(base + sb * GEO::SEG + v * OPI * SLOT) = r[v];
}
// A store predicate is one 32-bit compare: `lim` (res_lim32) = the bytes of the wave's span of the array that lie below N,
// clamped to [0, 2^30] -- a span is 64 * PITCH bytes -- against the lane's offset; the piece's own offset is a scalar.
__device__ __forceinline__ int res_lim32(long lim) { return lim < 0 ? 0 : (lim > (1L << 30) ? (1 << 30) : (int)lim); }
// the owners' slots -> global (coalesced), pieces at or beyond `lim` dropped: pieces v0 .. v0 + nv - 1 of sub-tile `sb`
// (one wave-instruction each: OPI owners, all G records of each)
template <typename GEO, int SLOT, int PITCH>
__device__ __forceinline__ void res_drain_part(char* __restrict__ g /*wave-uniform*/, int sb, int v0, int nv, int lim, bool full,
                                               const char* slots) {
    const int lane = threadIdx.x & (kWave - 1);
    constexpr int NV = GEO::NV, OPI = kWave / NV;
    const char* base = slots + (lane / NV) * SLOT + (lane % NV) * 16;
    const unsigned loff = (unsigned)(lane / NV) * PITCH + (unsigned)(lane % NV) * 16u;
    if (full) {
        // a whole wave (one scalar branch for the group): every read is issued before the first store waits for its data
        V4 x[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v)
            if (v >= v0 && v < v0 + nv) x[v] = *reinterpret_cast<const V4*>(base + sb * GEO::SEG + v * OPI * SLOT);
#pragma unroll
        for (int v = 0; v < NV; ++v)
            if (v >= v0 && v < v0 + nv) *reinterpret_cast<V4*>(g + ((long)sb * GEO::SEG + (long)v * OPI * PITCH) + loff) = x[v];
    } else {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if (v < v0 || v >= v0 + nv) continue;
            const V4 x = *reinterpret_cast<const V4*>(base + sb * GEO::SEG + v * OPI * SLOT);
            if ((int)loff < lim - (sb * GEO::SEG + v * OPI * PITCH))
                *reinterpret_cast<V4*>(g + ((long)sb * GEO::SEG + (long)v * OPI * PITCH) + loff) = x;
        }
    }
}
// the whole sub-tile
template <typename GEO, int SLOT, int PITCH>
__device__ __forceinline__ void res_drain(char* __restrict__ g /*wave-uniform*/, int sb, int lim, bool full, const char* slots) {
    res_drain_part<GEO, SLOT, PITCH>(g, sb, 0, GEO::NV, lim, full, slots);
}
// the means of one sub-tile: staging buffer (one sub-tile deep) -> global
template <typename GEO, int PITCH>
__device__ __forceinline__ void res_drain_m(char* __restrict__ g /*wave-uniform*/, int sb, int lim, bool full, const char* mst) {
    const int lane = threadIdx.x & (kWave - 1);
    constexpr int NV = GEO::NV, OPI = kWave / NV;
    const char* base = mst + (lane / NV) * GEO::STRIDE + (lane % NV) * 16;
    const unsigned loff = (unsigned)(lane / NV) * PITCH + (unsigned)(lane % NV) * 16u;
    if (full) {
        V4 x[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) x[v] = *reinterpret_cast<const V4*>(base + v * OPI * GEO::STRIDE);
#pragma unroll
        for (int v = 0; v < NV; ++v) *reinterpret_cast<V4*>(g + ((long)sb * GEO::SEG + (long)v * OPI * PITCH) + loff) = x[v];
    } else {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const V4 x = *reinterpret_cast<const V4*>(base + v * OPI * GEO::STRIDE);
            if ((int)loff < lim - (sb * GEO::SEG + v * OPI * PITCH))
                *reinterpret_cast<V4*>(g + ((long)sb * GEO::SEG + (long)v * OPI * PITCH) + loff) = x;
        }
    }
}

// the wait for every workgroup's arrival at the grid-wide barrier whose counters `bar` holds (one arrival per workgroup).
// The publishing wave has drained the stores it publishes (s_waitcnt vmcnt(0)) before one of its lanes arrives.
__device__ __forceinline__ void res_wait_all(int* bar, int nblocks, int* status) {
    if (threadIdx.x < 8) {
        const int want = (nblocks - (int)threadIdx.x + 7) / 8;       // tiles whose index is threadIdx.x mod 8
        if (want > 0) wait_flag(bar + threadIdx.x * 32, want, status);
    }
    __syncthreads();
}
__device__ __forceinline__ void res_arrive(int* bar, int tile) {
    __hip_atomic_fetch_add(bar + (tile & 7) * 32, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The neighbour hand-off (with the forgetting shortcut): a workgroup that can take its carry from ONE neighbour's total waits
// for that neighbour's record only, and falls back to the grid-wide wait when the total has not forgotten its past.  Every
// workgroup still ARRIVES at both barriers (the fallback and the log-likelihood sum count on it); nobody waits for the slowest
// of 256 workgroups unless the data asks for it.  Waits go left in phase 2 and right in phase 3, each for a record published
// before its owner's own wait: no cycle.
//
// The record is ResGran::NG granules {low word: data, high word: tag}; a granule is current when its tag EQUALS the launch's
// epoch (the arrays are zeroed once, with the context; epochs start at 1 and only grow: tags are never reset).
template <typename T, int N>
struct ResGran {
    static constexpr int WPS = (int)sizeof(T) / 4;      // 32-bit words per scalar
    static constexpr int NG = N * WPS;                  // granules per record
    static_assert(NG <= kWave && NG * 8 <= kResGranStride, "one wave-instruction and one place per record");
};
__device__ __forceinline__ unsigned long long* res_gran_rec(unsigned long long* g, int tile) {
    return g + (long)tile * (kResGranStride / 8);
}
// Producer; called by the whole of wave 0, whose lane `holder` has the total in v[].  The holder hands it to its wave through
// `hand` (LDS keeps a wave's accesses in order), lanes 0 .. NG - 1 store one granule each: ONE 8-byte wave-store.  Nothing
// waits here: the wave drains behind the scan's tail, in front of its arrival.
template <typename T, int N>
__device__ __forceinline__ void res_publish(unsigned long long* rec, unsigned* hand, const T* v, int holder, int epoch) {
    constexpr int NG = ResGran<T, N>::NG;
    const int lane = threadIdx.x & (kWave - 1);
    if (lane == holder) {
        unsigned w[NG];
        __builtin_memcpy(w, v, sizeof(w));
#pragma unroll
        for (int i = 0; i < NG; ++i) hand[i] = w[i];
    }
    res_wave_sync();
    if (lane < NG) {
        const unsigned long long x = ((unsigned long long)(unsigned)epoch << 32) | hand[lane];
        __hip_atomic_store(rec + lane, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// Consumer.  Lanes 0 .. NG - 1 of wave 0 poll one granule each; res_poll_first() puts the first load in flight (work may
// follow it), res_take() re-reads the record until every polling lane has seen the epoch (the spin is bounded as every spin
// of the launch is: a lane whose granule is still stale then raises status bit 1), passes the data words through `hand` and
// leaves the record in every lane.
template <typename T, int N>
__device__ __forceinline__ unsigned long long res_poll_first(const unsigned long long* rec) {
    if (threadIdx.x < ResGran<T, N>::NG) return __hip_atomic_load(rec + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return 0ull;
}
template <typename T, int N>
__device__ __forceinline__ void res_take(const unsigned long long* rec, unsigned long long x, int epoch, unsigned* hand, int* status, T* v) {
    constexpr int NG = ResGran<T, N>::NG;
    if (__builtin_amdgcn_readfirstlane((int)threadIdx.x) == 0) {        // wave 0: a scalar branch, and a scalar loop
        const bool polls = threadIdx.x < NG;
        bool stale = polls && (unsigned)(x >> 32) != (unsigned)epoch;
        int spins = 0;
        while (__builtin_amdgcn_ballot_w64(stale) != 0 && ++spins <= (1 << 22)) {
            __builtin_amdgcn_s_sleep(2);
            if (polls) x = __hip_atomic_load(rec + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            stale = polls && (unsigned)(x >> 32) != (unsigned)epoch;
        }
        if (stale) atomicOr(status, 2);
        if (polls) hand[threadIdx.x] = (unsigned)x;
    }
    __syncthreads();
    unsigned w[NG];
#pragma unroll
    for (int i = 0; i < NG; ++i) w[i] = hand[i];
    __builtin_memcpy(v, w, sizeof(w));
}
// a record every granule of which is known to be out (its owner has arrived at the barrier this workgroup waited at)
template <typename T, int N>
__device__ __forceinline__ void res_load_record(const unsigned long long* rec, T* v) {
    constexpr int NG = ResGran<T, N>::NG;
    unsigned w[NG];
#pragma unroll
    for (int i = 0; i < NG; ++i) w[i] = (unsigned)__hip_atomic_load(rec + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_memcpy(v, w, sizeof(w));
}

// ---------------------------------------------------------------------------------------------
// Branch-free forms of the lane-serial steps (same arithmetic, same rounding as filt_extend / kf_step of pgps_math.h for
// finite operands): a missing observation multiplies the gain by zero instead of branching around the update, so the 16
// unrolled steps of a phase are ONE basic block and the scheduler can run a step's update chain beside the previous step's
// smoothing element and hoist the next step's LDS reads -- with the branches every step was four small blocks and each
// LDS read was waited for where it was issued (25 k cycles for the Kalman pass of 16 steps at d = 2: 3074 vector
// instructions, half of the time stalls).
// ---------------------------------------------------------------------------------------------
template <typename T, int D>
__device__ __forceinline__ void res_filt_extend(FiltElem<T, D>& e, const T* F, const T* Q /*sym*/, T y, const T* h, T R) {
    T Ap[D * D], bp[D], FC[D * D], Cp[Dim<D>::SYM];
    mat_mul<T, D>(F, e.A, Ap);
    mat_vec<T, D>(F, e.b, bp);
    predict_cov<T, D>(F, e.C, Q, FC, Cp);
    const bool obs = !is_nan(y);
    T u[D], v[D];
    sym_vec<T, D>(Cp, h, u);
    mat_t_vec<T, D>(Ap, h, v);
    T S = R, hb = T(0);
#pragma unroll
    for (int i = 0; i < D; ++i) { S += h[i] * u[i]; hb += h[i] * bp[i]; }
    const T inv = obs ? recip(S) : T(0);
    const T res = obs ? y - hb : T(0);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const T Ki = u[i] * inv;
#pragma unroll
        for (int j = 0; j < D; ++j) e.A[i * D + j] = Ap[i * D + j] - Ki * v[j];
        e.b[i] = bp[i] + Ki * res;
        e.eta[i] += v[i] * (res * inv);
    }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i; j < D; ++j) {
            e.C[symi<D>(i, j)] = Cp[symi<D>(i, j)] - u[i] * u[j] * inv;
            e.J[symi<D>(i, j)] += v[i] * v[j] * inv;
        }
}

// one Kalman step (not the first of the series) with its log-likelihood term; mp, Pp, FP = the predict, for the smoother
template <typename T, int D>
__device__ __forceinline__ void res_kf_step(MeanCov<T, D>& s, const T* F, const T* Q /*sym*/, T y, const T* h, T R, LogLik& ll,
                                            T* mp, T* Pp, T* FP) {
    mat_vec<T, D>(F, s.m, mp);
    predict_cov<T, D>(F, s.P, Q, FP, Pp);
    const bool obs = !is_nan(y);
    T u[D];
    sym_vec<T, D>(Pp, h, u);
    T S = R, mu = T(0);
#pragma unroll
    for (int i = 0; i < D; ++i) { S += h[i] * u[i]; mu += h[i] * mp[i]; }
    const T rinv = recip(S);
    {
        // LogLik::add without the branch: a missing step contributes r = 0, S = 1 (mantissa product and exponent unchanged)
        const double r = obs ? ll_diff(y, mu) : 0.0;
        const double Sw = obs ? ll_wide(S) : 1.0;
        ll.quad += r * r * (obs ? double(rinv) : 0.0);
        int e;
        ll.mant = std::frexp(ll.mant * Sw, &e);
        ll.expo += e;
        ll.count += obs ? 1 : 0;
    }
    const T inv = obs ? rinv : T(0);
    const T res = obs ? y - mu : T(0);
#pragma unroll
    for (int i = 0; i < D; ++i) s.m[i] = mp[i] + u[i] * (res * inv);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i; j < D; ++j) s.P[symi<D>(i, j)] = Pp[symi<D>(i, j)] - u[i] * u[j] * inv;
}

// ---------------------------------------------------------------------------------------------
// Workgroup scans whose cross-wave level runs on LANES: the four wave totals sit in lanes 0..3 of every wave and are
// scanned by two DPP steps (two combines) and the wave's own prefix is read with v_readlane; block_scan_exclusive of
// pgps_kernels.hip.h walks the four totals one after the other, twice (six combines, every lane the same work).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float res_readlane(float x, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
}
__device__ __forceinline__ double res_readlane(double x, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l), hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}
template <typename E>
__device__ __forceinline__ E res_readlane_elem(const E& e, int l) {
    using TR = ElemTraits<E>;
    typename TR::Scalar v[TR::N];
    pack(e, v);
#pragma unroll
    for (int i = 0; i < TR::N; ++i) v[i] = res_readlane(v[i], l);
    E r;
    unpack(v, r);
    return r;
}
// DPP moves with bound_ctrl set and every row and bank enabled: a lane whose source lies outside its row (row_shr /
// row_shl) or outside the wave (wave_shr / wave_shl) reads ZERO.  No `old` operand is kept, so nothing is copied ahead of
// the move: one v_mov_b32_dpp per dword and level.
template <int CTRL>
__device__ __forceinline__ float res_dpp0(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ double res_dpp0(double x) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// x where `keep`, else 1, for an x that is +0 wherever !keep: one select, on the word that holds the exponent
__device__ __forceinline__ float res_one_unless(float x, bool keep) {
    return __builtin_bit_cast(float, keep ? __builtin_bit_cast(int, x) : 0x3f800000);
}
__device__ __forceinline__ double res_one_unless(double x, bool keep) {
    return __hiloint2double(keep ? __double2hiint(x) : 0x3ff00000, __double2loint(x));
}
// the all-zero element is the identity but for the unit diagonal of A (filter) / E (smoother)
template <typename T, int D>
__device__ __forceinline__ void res_unit_diag(FiltElem<T, D>& e, bool keep) {
#pragma unroll
    for (int i = 0; i < D; ++i) e.A[i * D + i] = res_one_unless(e.A[i * D + i], keep);
}
template <typename T, int D>
__device__ __forceinline__ void res_unit_diag(SmthElem<T, D>& e, bool keep) {
#pragma unroll
    for (int i = 0; i < D; ++i) e.E[i * D + i] = res_one_unless(e.E[i * D + i], keep);
}
// the element the DPP pattern CTRL moves into this lane, or the identity where it has no source (`has` false): D selects
// in place of one per dword.  Combining with the identity returns the other operand bit for bit for finite operands
// (every product is x * 1 or y * 0 and every sum adds a zero: tests/test_res_identity.py), so every lane combines at the
// row levels and no lane keeps its old value by a select.
template <int CTRL, typename E>
__device__ __forceinline__ E res_dpp_elem(const E& e, bool has) {
    using TR = ElemTraits<E>;
    typename TR::Scalar v[TR::N];
    pack(e, v);
#pragma unroll
    for (int i = 0; i < TR::N; ++i) v[i] = res_dpp0<CTRL>(v[i]);
    E r;
    unpack(v, r);
    res_unit_diag(r, has);
    return r;
}
// inclusive scan over the 64 lanes of a wave, in place.  wave_scan_inclusive of pgps_kernels.hip.h without its per-level
// `if (lane takes part)`: the four row levels combine in every lane (with the identity where the shift has no source), the
// two cross-row levels keep the rows they do not reach by a select -- six levels in one basic block instead of six
// divergent regions (PGPS_RES_SCAN_SELECT=0: the shared branching version)
#ifndef PGPS_RES_SCAN_SELECT
#define PGPS_RES_SCAN_SELECT 1
#endif
template <typename E, bool FORWARD>
__device__ __forceinline__ void res_wave_scan_inclusive(E& incl, int lane) {
#if PGPS_RES_SCAN_SELECT
    using TR = ElemTraits<E>;
    const int r = lane & 15;
    auto all = [&](const E& other) {
        E t;
        if (FORWARD) TR::combine(other, incl, t); else TR::combine(incl, other, t);
        incl = t;
    };
    auto step = [&](const E& other, bool act) {
        E t;
        if (FORWARD) TR::combine(other, incl, t); else TR::combine(incl, other, t);
        typename TR::Scalar a[TR::N], b[TR::N];
        pack(t, a);
        pack(incl, b);
#pragma unroll
        for (int i = 0; i < TR::N; ++i) b[i] = act ? a[i] : b[i];
        unpack(b, incl);
    };
    if constexpr (FORWARD) {
        all(res_dpp_elem<kDppRowShr + 1>(incl, r >= 1));
        all(res_dpp_elem<kDppRowShr + 2>(incl, r >= 2));
        all(res_dpp_elem<kDppRowShr + 4>(incl, r >= 4));
        all(res_dpp_elem<kDppRowShr + 8>(incl, r >= 8));
        step(dpp_elem<kDppBcast15, 0xa>(incl), (lane & 16) != 0);
        step(dpp_elem<kDppBcast31, 0xc>(incl), lane >= 32);
    } else {
        all(res_dpp_elem<kDppRowShl + 1>(incl, r + 1 < 16));
        all(res_dpp_elem<kDppRowShl + 2>(incl, r + 2 < 16));
        all(res_dpp_elem<kDppRowShl + 4>(incl, r + 4 < 16));
        all(res_dpp_elem<kDppRowShl + 8>(incl, r + 8 < 16));
        const int row = lane >> 4;
        step(shfl_idx_elem(incl, ((row + 1) & 3) * 16), row < 3);
        step(shfl_idx_elem(incl, ((row + 2) & 3) * 16), row < 2);
    }
#else
    wave_scan_inclusive<E, FORWARD>(incl, lane);
#endif
}

// inclusive scan of the values lanes 0..3 hold (identity elsewhere), in place: lanes 0..3 end with the prefixes (FORWARD)
// or the suffixes of the four
template <typename E, bool FORWARD>
__device__ __forceinline__ void res_scan4(E& x, int lane) {
    using TR = ElemTraits<E>;
    const int r = lane & 15;
    auto all = [&](const E& other) {
        E t;
        if (FORWARD) TR::combine(other, x, t); else TR::combine(x, other, t);
        x = t;
    };
    if constexpr (FORWARD) {
        all(res_dpp_elem<kDppRowShr + 1>(x, r >= 1));
        all(res_dpp_elem<kDppRowShr + 2>(x, r >= 2));
    } else {
        all(res_dpp_elem<kDppRowShl + 1>(x, r + 1 < 16));
        all(res_dpp_elem<kDppRowShl + 2>(x, r + 2 < 16));
    }
}
// Exclusive workgroup scan.  The workgroup's total exists in ONE lane as soon as the cross-wave level is done -- lane 3
// (FORWARD) / lane 0 of every wave -- and `publish(total)` runs at once, in the whole of wave 0 (the total is valid in its
// lane 3 / 0: res_publish): the neighbour that waits for it does not wait for the v_readlane broadcast, the final combine
// and the barrier below, under which the publishing wave's stores drain.
template <typename E, bool FORWARD, typename PUB>
__device__ __forceinline__ void res_block_scan_exclusive(const E& mine, E& excl, typename ElemTraits<E>::Scalar* lds, PUB&& publish) {
    using TR = ElemTraits<E>;
    static_assert(kWaves == 4, "four wave totals in lanes 0..3");
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    E incl = mine;
    res_wave_scan_inclusive<E, FORWARD>(incl, lane);
    // the neighbour lane's inclusive value; the identity in the first (FORWARD) / last lane, which has none
    E wex = FORWARD ? res_dpp_elem<kDppWaveShr1>(incl, lane != 0) : res_dpp_elem<kDppWaveShl1>(incl, lane != kWave - 1);
    if (FORWARD ? (lane == kWave - 1) : (lane == 0)) rec_store(lds + wave * TR::N, incl);
    __syncthreads();
    E t;
    TR::identity(t);
    if (lane < kWaves) rec_load(lds + lane * TR::N, t);
    res_scan4<E, FORWARD>(t, lane);
    if (wave == 0) publish(t);
    // (no branch on the wave's position: the first / last wave combines with the identity, which is exact)
    typename TR::Scalar pv[TR::N], iv[TR::N];
    {
        E id;
        TR::identity(id);
        pack(id, iv);
        pack(t, pv);
    }
    const bool edge = FORWARD ? (wave == 0) : (wave == kWaves - 1);
    const int src = FORWARD ? (edge ? 0 : wave - 1) : (edge ? 0 : wave + 1);
#pragma unroll
    for (int i = 0; i < TR::N; ++i) { const typename TR::Scalar x = res_readlane(pv[i], src); pv[i] = edge ? iv[i] : x; }
    E p;
    unpack(pv, p);
    if (FORWARD) TR::combine(p, wex, excl); else TR::combine(wex, p, excl);
    __syncthreads();
}
// ordered reduction of one element per lane over the workgroup (lane order = time order), result in every lane
template <typename E>
__device__ __forceinline__ void res_block_reduce_ordered(const E& mine, E& total, typename ElemTraits<E>::Scalar* lds) {
    using TR = ElemTraits<E>;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    E acc = mine;
    res_wave_scan_inclusive<E, true>(acc, lane);
    if (lane == kWave - 1) rec_store(lds + wave * TR::N, acc);
    __syncthreads();
    E t;
    TR::identity(t);
    if (lane < kWaves) rec_load(lds + lane * TR::N, t);
    res_scan4<E, true>(t, lane);
    total = res_readlane_elem(t, kWaves - 1);
    __syncthreads();
}

// the lane's LC values of a vector array (ys, ts), loaded coalesced and transposed through the wave's staging buffer
// (64 bytes per lane and round); whole waves only.  issue() first, other loads may follow, finish() waits for these alone.
template <typename T, int LC>
struct ResLaneValues {
    using GY = StageGeom<64, 1>;
    static constexpr int PER = 64 / (int)sizeof(T);             // values per lane and round
    static constexpr int R = LC / PER > 0 ? LC / PER : 1;
    static_assert(LC % PER == 0, "whole rounds");
    V4 r[R][GY::NV];
    __device__ __forceinline__ void issue(const T* __restrict__ g /*the wave's first value*/) {
        const int lane = threadIdx.x & (kWave - 1);
        constexpr int NV = GY::NV, OPI = kWave / NV, PITCH = LC * (int)sizeof(T);
        const unsigned loff = (unsigned)(lane / NV) * PITCH + (unsigned)(lane % NV) * 16u;
#pragma unroll
        for (int rd = 0; rd < R; ++rd)
#pragma unroll
            for (int v = 0; v < NV; ++v)
                r[rd][v] = *reinterpret_cast<const V4*>(reinterpret_cast<const char*>(g) + ((long)rd * 64 + (long)v * OPI * PITCH) + loff);
    }
    __device__ __forceinline__ void finish(char* mst, T* out) {
        const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
        for (int rd = 0; rd < R; ++rd) {
            res_wave_sync();
            constexpr int NV = GY::NV, OPI = kWave / NV;
            char* base = mst + (lane / NV) * GY::STRIDE + (lane % NV) * 16;
#pragma unroll
            for (int v = 0; v < NV; ++v) *reinterpret_cast<V4*>(base + v * OPI * GY::STRIDE) = r[rd][v];
            res_wave_sync();
            load_rec<T, PER>(reinterpret_cast<const T*>(mst + lane * GY::STRIDE), out + rd * PER);
        }
        res_wave_sync();
    }
};

// The lane's smoothing aggregate e_0 (x) e_1 (x) ... (x) e_{LC-1}, strictly left to right, is folded INSIDE the Kalman pass: it
// is independent of the pass's own chain (m, P) and fills issue slots that chain leaves empty.  Nothing but the suffix scan
// behind the pass reads it, so without a pin the compiler sinks all LC combines there, out of the unrolled steps and across
// their sched_barriers, onto the stretch the left neighbour waits for.  With 16 steps per lane an element
// joins the chain one step AFTER the step that computes it, when its operands are long ready (the last two behind the
// loop); with 8 in its own step: chosen per LC by measurement (profiles/resident_aggregate_placements.txt).
// The chain starts AT its first element: smth_combine(identity, e) returns e bit for bit (tests/test_res_identity.py,
// tests/test_gpu_resident_aggregate.py).
template <int LC> struct ResAggLate { static constexpr bool value = LC >= 16; };
template <typename T, int D>
__device__ __forceinline__ void res_pin(SmthElem<T, D>& e) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) asm volatile("" : "+v"(e.E[i]));
#pragma unroll
    for (int i = 0; i < D; ++i) asm volatile("" : "+v"(e.g[i]));
#pragma unroll
    for (int i = 0; i < Dim<D>::SYM; ++i) asm volatile("" : "+v"(e.L[i]));
}
// sagg <- sagg (x) e (the chain's first link: sagg <- e), kept where it is written
template <typename T, int D>
__device__ __forceinline__ void res_agg_fold(SmthElem<T, D>& sagg, const SmthElem<T, D>& e, bool first) {
    if (first) {
        sagg = e;
    } else {
        SmthElem<T, D> r;
        smth_combine(sagg, e, r);
        sagg = r;
    }
    res_pin(sagg);
}

// SMOOTH = false: the filter alone (pkf: filtered moments and / or the log-likelihood) -- phases 1 and 2 without the smoothing
// elements, one hand-off; the series still stays on chip between the reduce and the Kalman pass, i.e. Fs, Qs, ys are read once.
template <typename T, int D, int LC, bool FUSED, bool SMOOTH = true, bool SKEW = false>
__global__ __launch_bounds__(kBlock) void k_pkfs_resident(const ResArgs<T> ra) {
    using CFG = ResCfg<T, D, LC>;
    using GF = typename CFG::GF;
    using GM = typename CFG::GM;
    using FE = FiltElem<T, D>;
    using SE = SmthElem<T, D>;
    using MC = MeanCov<T, D>;
    constexpr int MAT = D * D, SYM = Dim<D>::SYM, NF = Dim<D>::NFILT, NS = Dim<D>::NSMTH, G = CFG::G, S = CFG::S;
    constexpr int SLOT = CFG::SLOT;
    static_assert(kBlock == 256, "one workgroup of four waves per CU");
    static_assert(D <= 2, "resident pass: d <= 2");
    const ScanArgs<T>& a = ra.s;

    __shared__ __attribute__((aligned(16))) char smem[CFG::BYTES];
    const int tile = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));    // a scalar: the wave's addresses stay scalar
    char* slots = smem + wave * CFG::SLOTS;                                 // this wave's 64 slots
    char* mst = smem + kWaves * CFG::SLOTS + wave * CFG::MST;               // this wave's staging of the means
    T* lds = reinterpret_cast<T*>(smem + kWaves * (CFG::SLOTS + CFG::MST));   // the workgroup scans' scratch
    unsigned* hand = reinterpret_cast<unsigned*>(smem + kWaves * (CFG::SLOTS + CFG::MST) + kWaves * CFG::NREC);     // one record handed over
    double* lds_ll = reinterpret_cast<double*>(smem + kWaves * (CFG::SLOTS + CFG::MST) + CFG::NSCAN);
    char* myslot = slots + lane * SLOT;
    T* myrec = reinterpret_cast<T*>(myslot);

    PGPS_RSTAMP(0);
    if (tile == 0 && threadIdx.x < 16) ra.bar_next[threadIdx.x * 32] = 0;        // both barriers' shards of the next launch

    const long N = a.N;
    const long gt = (long)tile * kBlock + threadIdx.x;
    const long k0 = gt * LC;
    const long wbase = ((long)tile * kBlock + wave * kWave) * LC;
    const bool full = (wbase + (long)kWave * LC <= N);                      // wave-uniform: no padding, no predicates
    constexpr int PF = LC * MAT * (int)sizeof(T), PM = LC * D * (int)sizeof(T);        // a lane's bytes of a matrix / vector array
    const long limF = (N - wbase) * MAT * (long)sizeof(T);
    const int limP = res_lim32(limF), limM = res_lim32((N - wbase) * D * (long)sizeof(T));     // the output stores' predicates

    T h[D], P0[SYM];
    if constexpr (FUSED) {
        gp_prior<T, D>(ra.m, h, P0);
    } else {
        T P0f[MAT];
#pragma unroll
        for (int i = 0; i < MAT; ++i) P0f[i] = a.P0[i];
        sym_from_full<T, D>(P0f, P0);
#pragma unroll
        for (int i = 0; i < D; ++i) h[i] = a.H[i];
    }
    const T Rn = a.R;

    // ---------------------------------------------------------------------------------------------
    // phase 1: the chunk comes on chip and is reduced
    // ---------------------------------------------------------------------------------------------
    T Freg[LC][MAT];            // F_k; from phase 2 on: E_k
    T yreg[LC];                 // y_k; from phase 2 on the last component of g_k (the others travel with L_k in the slot)
    constexpr int GL = MAT - SYM;       // components of g that fit beside L in a step's 'matrix record' of the slot (d = 2: one, d = 1: none)
    static_assert(D - GL == 1, "one component of g per step stays in registers");
    FE agg;
    filt_identity(agg);
    auto reduce_step = [&](int j, const T* Qf) {
        T Q[SYM];
        sym_from_full<T, D>(Qf, Q);
        if (j == 0) {
            if (k0 == 0) filt_first(agg, P0, yreg[0], h, Rn);
            else res_filt_extend(agg, Freg[0], Q, yreg[0], h, Rn);
        } else {
            res_filt_extend(agg, Freg[j], Q, yreg[j], h, Rn);
        }
    };
    {
        const T nanv = T(__builtin_nan(""));
        if constexpr (FUSED) {
            T tv[LC];
            const T* tp = ra.m.ts;
            T tprev;
            if (full) {
                ResLaneValues<T, LC> lt, ly;
                lt.issue(tp + wbase);
                ly.issue(a.ys + wbase);
                lt.finish(mst, tv);
                ly.finish(mst, yreg);
                tprev = wshfl_up(tv[LC - 1], 1);
                if (lane == 0) tprev = (k0 > 0) ? tp[k0 - 1] : ra.m.t_prev;
            } else {
                const T tl = tp[N - 1];
#pragma unroll
                for (int j = 0; j < LC; ++j) {
                    const bool in = k0 + j < N;
                    tv[j] = in ? tp[in ? k0 + j : 0] : tl;
                    yreg[j] = in ? a.ys[in ? k0 + j : 0] : nanv;
                }
                tprev = (k0 > 0) ? (k0 - 1 < N ? tp[k0 - 1 < N ? k0 - 1 : 0] : tl) : ra.m.t_prev;
            }
#pragma unroll
            for (int j = 0; j < LC; ++j) {
                T Qf[MAT];
                lti_step<T, D>(ra.m, tv[j] - tprev, Freg[j], Qf);
                tprev = tv[j];
                store_rec<T, MAT>(myrec + j * MAT, Qf);
                reduce_step(j, Qf);
            }
        } else {
            const char* gF = reinterpret_cast<const char*>(a.Fs + wbase * MAT);
            const char* gQ = reinterpret_cast<const char*>(a.Qs + wbase * MAT);
            // two sub-tiles of F and of Q in flight per wave (128 KiB per CU): one did not keep the memory path busy
            // (9.2 B/clk per CU in this phase against 11 - 13 in the three-launch kernels' loops)
            // whole waves and ragged ones run two copies of the loop: inside one copy every wait counts exactly the loads
            // it needs (a full / ragged choice per load made hipcc drain the whole prefetch at each join: s_waitcnt vmcnt(0))
            auto stream = [&](auto full_tag) {
                constexpr bool FULL = decltype(full_tag)::value;
                V4 rF[2][GF::NV], rQ[2][GF::NV];
                ResLaneValues<T, LC> ly;
                if constexpr (FULL) ly.issue(a.ys + wbase);
                res_issue<T, D, GF, PF>(gF, 0, limF, FULL, 0, rF[0]);
                res_issue<T, D, GF, PF>(gQ, 0, limF, FULL, 1, rQ[0]);
                if (S > 1) {
                    res_issue<T, D, GF, PF>(gF, 1, limF, FULL, 0, rF[1]);
                    res_issue<T, D, GF, PF>(gQ, 1, limF, FULL, 1, rQ[1]);
                }
                if constexpr (FULL) {
                    ly.finish(mst, yreg);
                } else {
#pragma unroll
                    for (int j = 0; j < LC; ++j) yreg[j] = (k0 + j < N) ? a.ys[k0 + j < N ? k0 + j : 0] : nanv;
                }
#pragma unroll
                for (int sb = 0; sb < S; ++sb) {
                    const int p = sb & 1;
                    // F of the sub-tile through the slots into registers, then Q into the same place, where it stays
                    res_wave_sync();
                    res_commit<GF, SLOT>(slots, sb, rF[p]);
                    if (sb + 2 < S) res_issue<T, D, GF, PF>(gF, sb + 2, limF, FULL, 0, rF[p]);
                    res_wave_sync();
#pragma unroll
                    for (int i = 0; i < G; ++i) load_rec<T, MAT>(myrec + (sb * G + i) * MAT, Freg[sb * G + i]);
                    res_wave_sync();
                    res_commit<GF, SLOT>(slots, sb, rQ[p]);
                    if (sb + 2 < S) res_issue<T, D, GF, PF>(gQ, sb + 2, limF, FULL, 1, rQ[p]);
                    res_wave_sync();
#pragma unroll
                    for (int i = 0; i < G; ++i) {
                        const int j = sb * G + i;
                        T Qf[MAT];
                        load_rec<T, MAT>(myrec + j * MAT, Qf);
                        reduce_step(j, Qf);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            };
            if (full) stream(std::true_type{}); else stream(std::false_type{});
        }
    }
    PGPS_RSTAMP_WAVE(0);
    PGPS_RSTAMP(1);
    FE excl;
    // the workgroup's total is published from inside the scan, by wave 0, the moment its lane 3 holds it
    res_block_scan_exclusive<FE, true>(agg, excl, lds, [&](const FE& total) {
        T v[NF];
        pack(total, v);
        if constexpr (SKEW) { if (lane == kWaves - 1) res_skew(ra, tile, 1); }
        res_publish<T, NF>(res_gran_rec(ra.gran1, tile), hand, v, kWaves - 1, ra.epoch);
    });
    // the arrival: behind the scan's tail, under which the granule stores have drained
    if (wave == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            if constexpr (SKEW) res_wstamp(ra, tile, 10);
            res_arrive(ra.bar, tile);
        }
    }
    PGPS_RSTAMP(2);
    // (the wait: below, where the carry is taken -- for the left neighbour alone when its total has forgotten its past)

    // ---------------------------------------------------------------------------------------------
    // phase 2: carry in, Kalman pass, smoothing elements in place
    // ---------------------------------------------------------------------------------------------
    MC s;
#pragma unroll
    for (int i = 0; i < D; ++i) s.m[i] = T(0);
#pragma unroll
    for (int i = 0; i < SYM; ++i) s.P[i] = P0[i];
    if (tile > 0) {
        // The forgetting shortcut.  The carry into this tile is the prefix T_0 (x) ... (x) T_{tile-1} applied to the prior; in
        // ANY bracketing its (b, C) are those of the last total whenever that total's A vanishes: out.b = A_2 w + b_2,
        // out.C = A_2 N A_2^T + C_2 (parallel.py:100-118).  A total over 4096 steps of a filter that forgets (|A| shrinks by a
        // factor per step: 0.917^4096 = 1e-154 for config c2 before the update's own contraction) has |A| far below anything a
        // sum with b or C can see, so the left neighbour's record alone is the carry and the fold of up to 255 records -- eight
        // combine levels, 10 % of the launch -- is skipped.  Decided per launch FROM THE DATA (max |A| <= 2^-120 in fp64, 2^-60 in
        // fp32: thirty orders below the unit round-off; a NaN fails the test), identical in every lane (they read the same
        // words); otherwise the general fold below runs.  Both roads give the same bits whenever the shortcut applies.
        FE nb;
        bool forget = false;
        if (a.shortcut != 0) {
            const unsigned long long* rec = res_gran_rec(ra.gran1, tile - 1);
            T v[NF];
            res_take<T, NF>(rec, res_poll_first<T, NF>(rec), ra.epoch, hand, a.status, v);
            unpack(v, nb);
            T amax = T(0);
#pragma unroll
            for (int i = 0; i < MAT; ++i) amax = fmax(amax, fabs(nb.A[i]));
            forget = amax <= ResForget<T>::kA;
        }
        if (__builtin_amdgcn_readfirstlane((int)forget)) {
#pragma unroll
            for (int i = 0; i < D; ++i) s.m[i] = nb.b[i];
#pragma unroll
            for (int i = 0; i < SYM; ++i) s.P[i] = nb.C[i];
        } else {
            res_wait_all(ra.bar, a.nblocks, a.status);      // every total to the left is needed
            FE mine, left;
            filt_identity(mine);
            if ((int)threadIdx.x < tile) {
                T v[NF];
                res_load_record<T, NF>(res_gran_rec(ra.gran1, (int)threadIdx.x), v);
                unpack(v, mine);
            }
            res_block_reduce_ordered(mine, left, lds);
            filt_apply(s, left);
        }
    }
    PGPS_RSTAMP(3);
    filt_apply(s, excl);
    PGPS_RSTAMP(4);

    LogLik ll;
    constexpr bool AGG_LATE = ResAggLate<LC>::value;
    SE sagg, epend;             // the lane's aggregate; AGG_LATE: the element that joins it in the next step
    smth_identity(sagg);
    smth_identity(epend);
    // F, Q of the step after the chunk: the next lane's first step (its registers / its slot); the wave's last lane
    // reads global memory (the next wave's or workgroup's first step), or pads
    T Fh[MAT], Qh[MAT];
    T Qn[MAT];
    load_rec<T, MAT>(myrec, Qn);
    if constexpr (SMOOTH) {
#pragma unroll
        for (int i = 0; i < MAT; ++i) {
            Fh[i] = wshfl_down(Freg[0][i], 1);
            Qh[i] = wshfl_down(Qn[i], 1);
        }
        if (lane == kWave - 1) {
            const long k1 = k0 + LC;
            if (k1 < N) {
                if constexpr (FUSED) {
                    lti_step<T, D>(ra.m, ra.m.ts[k1] - ra.m.ts[k1 - 1], Fh, Qh);
                } else {
                    load_rec<T, MAT>(a.Fs + k1 * MAT, Fh);
                    load_rec<T, MAT>(a.Qs + k1 * MAT, Qh);
                }
            } else {
#pragma unroll
                for (int i = 0; i < MAT; ++i) { Fh[i] = (i / D == i % D) ? T(1) : T(0); Qh[i] = T(0); }
            }
        }
    }
    // smoothing element of step k0 + j_next - 1 from the predict of step k0 + j_next (parallel.py:159-166).  At step N: the
    // series' last element (0, m, P) (parallel.py:155-156) -- which is what the formulas give for F P = 0 (E = 0, g = m,
    // L = P).  Beyond N the padded steps (F = I, Q = 0) give the identity element up to rounding, to the RIGHT of an element
    // whose E is exactly zero: they reach nothing.
    const int to_end = (N - k0 < 0) ? -1 : (N - k0 > LC ? LC + 1 : (int)(N - k0));      // steps from the lane's first to step N, as far as the test needs it
    auto element = [&](int j_next, const MC& prev, const T* mp, const T* Pp, T* FP, SE& e) {
        const bool last = (j_next == to_end);
#pragma unroll
        for (int q = 0; q < MAT; ++q) FP[q] = last ? T(0) : FP[q];
        smth_element(prev, mp, Pp, FP, e);
    };
    // Drain schedule (filtered outputs requested).  A wave with a burst of stores in front of it stands still until the memory
    // path has taken them, and with one wave per SIMD nothing else runs meanwhile; spread out, the stores leave under the
    // arithmetic.  The means of sub-tile sb leave at its end (NV = 4 pieces; their staging buffer is one sub-tile deep).  The
    // NVP = 8 pieces of its filtered P leave DURING sub-tile sb + 1: PPS = 3, 3, 2 behind its first three steps, none behind
    // the fourth, which the means follow.  A piece holds all G records of OPI owners, so the slot records of sub-tile sb stay
    // "filtered P" until the last of its pieces has been read: their L records wait in registers one sub-tile longer (Lwait).
    // The last sub-tile's pieces go around the element of the chunk's last step, half before it and half behind, and its L
    // records into their slots after them, before phase 3 reads them.
    const bool store_f = (a.fms != nullptr);
    char* gP = reinterpret_cast<char*>(a.fPs + wbase * MAT);
    char* gM = reinterpret_cast<char*>(a.fms + wbase * D);
    constexpr int NVP = GF::NV, PPS = (NVP + G - 2) / (G - 1);
    T Lhold[MAT];               // [L | leading components of g] of the step before a sub-tile's first, until its slot record has been drained
    T Lwait[G - 1][MAT];        // those of the previous sub-tile's other steps
#pragma unroll
    for (int sb = 0; sb < S; ++sb) {
        T Lnew[G - 1][MAT];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int j = sb * G + i;
            T Q[SYM];
            sym_from_full<T, D>(Qn, Q);
            if (j + 1 < LC) load_rec<T, MAT>(myrec + (j + 1) * MAT, Qn);       // the next step's Q: requested a step ahead
            MC prev = s;
            T mp[D], Pp[SYM], FP[MAT];
            if (j == 0) {
                if (k0 == 0) kf_step(s, Freg[0], Q, yreg[0], h, Rn, true, ll, mp, Pp, FP);
                else res_kf_step(s, Freg[0], Q, yreg[0], h, Rn, ll, mp, Pp, FP);
            } else {
#ifndef PGPS_RES_BRANCHFREE
                kf_step(s, Freg[j], Q, yreg[j], h, Rn, false, ll, mp, Pp, FP);
#else
                res_kf_step(s, Freg[j], Q, yreg[j], h, Rn, ll, mp, Pp, FP);
#endif
                if constexpr (SMOOTH) {
                    // element of step j - 1: E, g take the registers F_{j-1}, y_{j-1} have left; L waits for its slot
                    SE e;
                    element(j, prev, mp, Pp, FP, e);
                    if constexpr (AGG_LATE) {
                        if (j >= 2) res_agg_fold(sagg, epend, j == 2);
                        epend = e;
                    } else {
                        res_agg_fold(sagg, e, j == 1);
                    }
#pragma unroll
                    for (int q = 0; q < MAT; ++q) Freg[j - 1][q] = e.E[q];
                    yreg[j - 1] = e.g[D - 1];
#pragma unroll
                    for (int q = 0; q < MAT; ++q) {
                        const T x = q < SYM ? e.L[q < SYM ? q : 0] : e.g[q < SYM ? 0 : q - SYM];
                        if (i == 0) Lhold[q] = x; else Lnew[i - 1][q] = x;
                    }
                }
            }
            // filtered moments of step j: P into the slot Q_j has left, m into the staging buffer
            T Pf[MAT];
            full_from_sym<T, D>(s.P, Pf);
            store_rec<T, MAT>(myrec + j * MAT, Pf);
            store_rec<T, D>(reinterpret_cast<T*>(mst + lane * GM::STRIDE) + i * D, s.m);
            // pieces of the previous sub-tile's filtered P (in the slots since the sync at its end)
            if (sb > 0 && store_f) res_drain_part<GF, SLOT, PF>(gP, sb - 1, i * PPS, PPS, limP, full, slots);
#ifndef PGPS_RES_NOSB
            // steps stay apart: across them the scheduler only lengthens live ranges (scratch) and gathers the stores
            __builtin_amdgcn_sched_barrier(0);
#endif
        }
        res_wave_sync();
        if (store_f) res_drain_m<GM, PM>(gM, sb, limM, full, mst);
        res_wave_sync();
        if constexpr (SMOOTH) {
            // L of steps 4 sb - 4 .. 4 sb - 1 into their slots: every piece of that sub-tile has been read (LDS keeps a wave's
            // accesses in order)
            if (sb > 0) {
#pragma unroll
                for (int i = 0; i + 1 < G; ++i) store_rec<T, MAT>(myrec + ((sb - 1) * G + i) * MAT, Lwait[i]);
                store_rec<T, MAT>(myrec + (sb * G - 1) * MAT, Lhold);
            }
#pragma unroll
            for (int i = 0; i + 1 < G; ++i)
#pragma unroll
                for (int q = 0; q < MAT; ++q) Lwait[i][q] = Lnew[i][q];
        }
    }
    if constexpr (!SMOOTH) {
        // the filter alone: the last sub-tile's pieces, then the workgroup's log-likelihood partial out, one arrival; workgroup 0
        // sums when everyone has arrived
        if (store_f) res_drain_part<GF, SLOT, PF>(gP, S - 1, 0, NVP, limP, full, slots);
        PGPS_RSTAMP_WAVE(1);
        PGPS_RSTAMP(5);
        const double v = ll.value();
        const double t = block_sum_double(v, lds_ll);
        if (threadIdx.x == 0) {
            if constexpr (SKEW) res_skew(ra, tile, 2);
            pub_store(a.llpart + tile, t);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if constexpr (SKEW) res_wstamp(ra, tile, 11);
            res_arrive(ra.bar2, tile);
        }
        if (tile == 0 && a.ll != nullptr) {
            res_wait_all(ra.bar2, a.nblocks, a.status);
            double w = 0.0;
            for (int b = threadIdx.x; b < a.nblocks; b += kBlock) w += pub_load(a.llpart + b);
            const double tt = block_sum_double(w, lds_ll);
            if (threadIdx.x == 0) *a.ll = tt;
        }
        PGPS_RSTAMP(9);
        return;
    }
    {
        // element of the chunk's last step from the step after the chunk, between the halves of the last sub-tile's pieces
        if (store_f) res_drain_part<GF, SLOT, PF>(gP, S - 1, 0, NVP / 2, limP, full, slots);
        constexpr int j = LC - 1;
        T Q[SYM], mp[D], Pp[SYM], FP[MAT];
        sym_from_full<T, D>(Qh, Q);
        mat_vec<T, D>(Fh, s.m, mp);
        predict_cov<T, D>(Fh, s.P, Q, FP, Pp);
        SE e;
        element(LC, s, mp, Pp, FP, e);
        if constexpr (AGG_LATE) res_agg_fold(sagg, epend, false);
        res_agg_fold(sagg, e, false);
#pragma unroll
        for (int q = 0; q < MAT; ++q) Freg[j][q] = e.E[q];
        yreg[j] = e.g[D - 1];
        T Lg[MAT];
#pragma unroll
        for (int q = 0; q < MAT; ++q) Lg[q] = q < SYM ? e.L[q < SYM ? q : 0] : e.g[q < SYM ? 0 : q - SYM];
        // (the element is computed HERE, between the two halves: without the pin it sinks below the second one)
#pragma unroll
        for (int q = 0; q < MAT; ++q) asm volatile("" : "+v"(Lg[q]));
        __builtin_amdgcn_sched_barrier(0);
        if (store_f) res_drain_part<GF, SLOT, PF>(gP, S - 1, NVP / 2, NVP - NVP / 2, limP, full, slots);
        res_wave_sync();
#pragma unroll
        for (int i = 0; i + 1 < G; ++i) store_rec<T, MAT>(myrec + ((S - 1) * G + i) * MAT, Lwait[i]);
        store_rec<T, MAT>(myrec + j * MAT, Lg);
    }
    PGPS_RSTAMP_WAVE(1);
    PGPS_RSTAMP(5);
    // (diagnostics: whatever of the aggregate's chain is left behind the pass stands between stamps 5 and 14)
    PGPS_RSTAMP(14);
    SE sexcl;
    // the smoothing total first, from inside the scan (wave 0; its lane 0 holds it): the left neighbour waits for it alone
    res_block_scan_exclusive<SE, false>(sagg, sexcl, lds, [&](const SE& stotal) {
        T vv[NS];
        pack(stotal, vv);
        if constexpr (SKEW) { if (lane == 0) res_skew(ra, tile, 2); }
        res_publish<T, NS>(res_gran_rec(ra.gran2, tile), hand, vv, 0, ra.epoch);
    });
    PGPS_RSTAMP(6);
    // the first poll of the right neighbour's record goes out in front of the log-likelihood work below
    const bool take_right = tile + 1 < a.nblocks && a.shortcut != 0;
    unsigned long long poll0 = 0ull;
    if (take_right) poll0 = res_poll_first<T, NS>(res_gran_rec(ra.gran2, tile + 1));
    {
        // then the log-likelihood partial, which only workgroup 0 reads, at the very end: its fp64 log and workgroup sum
        // run while this workgroup would wait for its right neighbour anyway (same values, same order of summation).
        // The arrival at barrier 2 comes after BOTH records -- the smoothing total's granules above and the partial here,
        // all stored by wave 0 -- are drained: the general fold below and workgroup 0's final sum wait for every arrival
        // and then read both kinds.
        const double v = ll.value();
        const double t = block_sum_double(v, lds_ll);
        if (threadIdx.x == 0) {
            pub_store(a.llpart + tile, t);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if constexpr (SKEW) res_wstamp(ra, tile, 11);
            res_arrive(ra.bar2, tile);
        }
    }

    // ---------------------------------------------------------------------------------------------
    // phase 3: carry back, smoothing pass over the kept elements
    // ---------------------------------------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < D; ++i) s.m[i] = T(0);
#pragma unroll
    for (int i = 0; i < SYM; ++i) s.P[i] = T(0);
    bool waited_all = false;
    if (tile + 1 < a.nblocks) {
        // the same shortcut backwards: a smoothing total whose E vanishes (the product of 4096 smoother gains) hands the tile
        // before it its own (g, L), whatever follows (parallel.py:176-184: E = E_a E_b, g = E_a g_b + g_a, L = E_a L_b E_a^T + L_a)
        SE nb;
        bool forget = false;
        if (take_right) {
            T v[NS];
            res_take<T, NS>(res_gran_rec(ra.gran2, tile + 1), poll0, ra.epoch, hand, a.status, v);
            unpack(v, nb);
            T emax = T(0);
#pragma unroll
            for (int i = 0; i < MAT; ++i) emax = fmax(emax, fabs(nb.E[i]));
            forget = emax <= ResForget<T>::kA;
        }
        if (__builtin_amdgcn_readfirstlane((int)forget)) {
#pragma unroll
            for (int i = 0; i < D; ++i) s.m[i] = nb.g[i];
#pragma unroll
            for (int i = 0; i < SYM; ++i) s.P[i] = nb.L[i];
        } else {
            res_wait_all(ra.bar2, a.nblocks, a.status);
            waited_all = true;
            SE mine, right;
            smth_identity(mine);
            const int b = tile + 1 + (int)threadIdx.x;
            if (b < a.nblocks) {
                T v[NS];
                res_load_record<T, NS>(res_gran_rec(ra.gran2, b), v);
                unpack(v, mine);
            }
            res_block_reduce_ordered(mine, right, lds);
            smth_apply(right, s);
        }
    }
    PGPS_RSTAMP(7);
    smth_apply(sexcl, s);
    PGPS_RSTAMP(8);
    if (tile == 0 && a.ll != nullptr) {
        if (!waited_all) res_wait_all(ra.bar2, a.nblocks, a.status);         // every workgroup's partial is out
        double v = 0.0;
        for (int b = threadIdx.x; b < a.nblocks; b += kBlock) v += pub_load(a.llpart + b);
        const double t = block_sum_double(v, lds_ll);
        if (threadIdx.x == 0) *a.ll = t;
    }
    char* oP = reinterpret_cast<char*>(a.sPs + wbase * MAT);
    char* oM = reinterpret_cast<char*>(a.sms + wbase * D);
    T Ln[MAT];
    load_rec<T, MAT>(myrec + (LC - 1) * MAT, Ln);
#pragma unroll
    for (int sb = S - 1; sb >= 0; --sb) {
#pragma unroll
        for (int i = G - 1; i >= 0; --i) {
            const int j = sb * G + i;
            SE e;
#pragma unroll
            for (int q = 0; q < MAT; ++q) e.E[q] = Freg[j][q];
            e.g[D - 1] = yreg[j];
#pragma unroll
            for (int q = 0; q < SYM; ++q) e.L[q] = Ln[q];
#pragma unroll
            for (int q = SYM; q < MAT; ++q) e.g[q - SYM] = Ln[q];
            if (j > 0) load_rec<T, MAT>(myrec + (j - 1) * MAT, Ln);            // the next step's L: requested a step ahead
            smth_apply(e, s);
            T Pf[MAT];
            full_from_sym<T, D>(s.P, Pf);
            store_rec<T, MAT>(myrec + j * MAT, Pf);
            store_rec<T, D>(reinterpret_cast<T*>(mst + lane * GM::STRIDE) + i * D, s.m);
        }
        res_wave_sync();
        res_drain<GF, SLOT, PF>(oP, sb, limP, full, slots);
        res_drain_m<GM, PM>(oM, sb, limM, full, mst);
        res_wave_sync();
    }
    PGPS_RSTAMP(9);
}

}  // namespace pgps
