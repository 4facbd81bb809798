// pgps_fused.hip.h -- the scan with the LTI discretisation fused in ("gp" entry points).
//
// For SDEs whose drift is  F = -lambda I + N  with N nilpotent (every Matern kernel, balanced or not:
// pssgp/kernels/matern/common.py:10-18) the transition matrix has the closed form
//     expm(dt F) = exp(-lambda dt) (I + dt N + dt^2 N^2 / 2 + ...)          (d terms)
// so  Fs[k], Qs[k] = Pinf - Fs[k] Pinf Fs[k]^T  (pssgp/kernels/base.py:29-47) cost one exp and a few
// dozen FMAs per step.  These kernels compute them in registers from (t_k, t_{k-1}) inside the three
// scan launches instead of reading the (N, d, d) arrays: a pass reads 2 scalars per step (t, y)
// instead of 2 d^2 + 1.  This is the StateSpaceGP path (model.py:92-117): times and observations in,
// log-likelihood and posterior out; Fs / Qs never exist in HBM.
//
// Structure, scratch and combine order are those of pgps_kernels.hip.h (k_filter_reduce /
// k_filter_apply / k_smoother_apply); only the source of (F, Q) differs.  Outputs go through the
// wave-private LDS staging so the stores stay coalesced; the filtered moments the smoother reads
// back are staged in the same way.  The discretisation arithmetic is fp64 whatever T is.
#pragma once

#include "pgps_kernels.hip.h"
#include "pgps_lik.h"

namespace pgps {

template <typename T, int D>
__device__ __forceinline__ void lti_step(const GpModel<T>& m, T dt_in, T* F, T* Qf) {
    constexpr int MAT = D * D;
    const double dt = double(dt_in);
    const double e = exp(-m.lam * dt);
    if constexpr (D == 1) {
        F[0] = T(e);
        Qf[0] = T(-m.Pinf[0] * expm1(-2.0 * m.lam * dt));
    } else {
        double Fd[MAT], X[MAT];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double v = (i == j ? 1.0 : 0.0) + dt * m.N1[i * D + j];
                if (D >= 3) v += dt * dt * m.N2[i * D + j];
                Fd[i * D + j] = e * v;
            }
        mat_mul<double, D>(Fd, m.Pinf, X);
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double acc = 0.0, acct = 0.0;
#pragma unroll
                for (int l = 0; l < D; ++l) { acc += X[i * D + l] * Fd[j * D + l]; acct += X[j * D + l] * Fd[i * D + l]; }
                Qf[i * D + j] = T(0.5 * (m.Pinf[i * D + j] + m.Pinf[j * D + i]) - 0.5 * (acc + acct));
                F[i * D + j] = T(Fd[i * D + j]);
            }
    }
}

template <typename T, int D>
__device__ __forceinline__ void gp_prior(const GpModel<T>& m, T* h, T* P0 /*sym*/) {
#pragma unroll
    for (int i = 0; i < D; ++i) h[i] = m.H[i];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i; j < D; ++j) P0[symi<D>(i, j)] = T(0.5 * (m.Pinf[i * D + j] + m.Pinf[j * D + i]));
}

// ---------------------------------------------------------------------------------------------
// per-observation noise variances: a compile-time flavour of the bodies below, HET, off by default --
// the scalar instantiations are what they were.  With HET a body takes `rs` (N given variances s_k), a lane loads rs[k + 1]
// next to its prefetch of ts[k + 1], ys[k + 1], and the step's noise variance is R + s_k.  At a missing step the loaded value
// never reaches the add (it may be NaN).  Instantiated in pgps_het_inst.hip, pgps_site_inst.hip and (one workgroup per series)
// pgps_panel_inst.hip.
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T het_noise(T R, T r, T y) {
    return R + (is_nan(y) ? T(0) : r);
}

// filter_apply_step (pgps_kernels.hip.h) in its (E, g, L) form with the step's noise variance as an argument
template <typename T, int D, bool SMOOTH>
__device__ __forceinline__ void gp_apply_step_r(const ScanArgs<T>& a, long k, long k0, const T* F, const T* Qf, T y, const T* h,
                                                T R, MeanCov<T, D>& s, LogLik& ll, SmthElem<T, D>& sagg) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM;
    T Q[SYM];
    sym_from_full<T, D>(Qf, Q);
    T mp[D], Pp[SYM], FP[MAT];
    MeanCov<T, D> prev = s;
    kf_step(s, F, Q, y, h, R, (k == 0) && a.seg_first, ll, mp, Pp, FP);
    if (SMOOTH && k > k0) {                 // element of step k-1 from this step's predict
        SmthElem<T, D> e, r;
        smth_element(prev, mp, Pp, FP, e);
        smth_combine(sagg, e, r);
        sagg = r;
    }
}

// ---------------------------------------------------------------------------------------------
// predictive checks of a fitted model against its own data: two compile-time flavours, off by default --
// the other instantiations are what they were.  OSA (gp_apply_body): the Kalman pass stores the one-step-ahead law of y_k,
// (mu_k, S_k) = (H m_k^-, H P_k^- H^T + R), the pair it hands to the log-likelihood accumulator, at EVERY step (observed or
// not).  LOO (gp_smooth_body): the smoother projects at every step, reads y_k and removes the factor N(y_k | f_k, R) from the
// smoothed law of f_k = H x_k (Rasmussen & Williams eq. 5.10-5.12 in cavity form), stores the leave-one-out law of y_k and
// accumulates its log density; one partial per workgroup (lpd_part), summed afterwards in a fixed order.  Any of the four
// arrays of GpLooOut (pgps_internal.h) may be null: that store is skipped.  Instantiated in pgps_loo_inst.hip and, one
// workgroup per series, in pgps_panel_inst.hip (k_gpp_loo).
// Both flavours combine with per-observation noise, again at compile time and off by default: OSA + HET
// takes the step's variance R_k = het_noise(R, rs[k], y_k) into the recursion and stores S_k with R + rs[k] AS STORED (at a
// missing row a NaN there gives a NaN variance at that row and reaches nothing else); LHET (gp_smooth_body, with LOO) loads
// rs[k - 1] next to ys[k - 1], under the same guard, and the epilogue removes N(y_k | f_k, R + rs[k]).
// ---------------------------------------------------------------------------------------------
// gp_apply_step_r that also hands out (mu, S) of the step: kf_step's own expressions on the predicted moments it returns.
// R: the step's noise variance in the recursion; Rs: the one in the stored S (they differ at a missing row of HET alone)
template <typename T, int D, bool SMOOTH>
__device__ __forceinline__ void gp_apply_step_osa(const ScanArgs<T>& a, long k, long k0, const T* F, const T* Qf, T y, const T* h,
                                                  T R, T Rs, MeanCov<T, D>& s, LogLik& ll, SmthElem<T, D>& sagg, T& mu, T& S) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM;
    T Q[SYM];
    sym_from_full<T, D>(Qf, Q);
    T mp[D], Pp[SYM], FP[MAT], u[D];
    MeanCov<T, D> prev = s;
    kf_step(s, F, Q, y, h, R, (k == 0) && a.seg_first, ll, mp, Pp, FP);
    sym_vec<T, D, kPkStep>(Pp, h, u);
    S = dot_add<T, D, kPkStep>(h, u, Rs);
    mu = dot_add<T, D, kPkStep>(h, mp, T(0));
    if (SMOOTH && k > k0) {                 // element of step k-1 from this step's predict
        SmthElem<T, D> e, r;
        smth_element(prev, mp, Pp, FP, e);
        smth_combine(sagg, e, r);
        sagg = r;
    }
}

// mean and variance of f = H x under (m, P)
template <typename T, int D>
__device__ __forceinline__ void gp_project(const GpModel<T>& m, const MeanCov<T, D>& s, T& mu, T& var) {
    mu = T(0);
    var = T(0);
#pragma unroll
    for (int r = 0; r < D; ++r) {
        mu += m.H[r] * s.m[r];
#pragma unroll
        for (int c = 0; c < D; ++c) var += m.H[r] * m.H[c] * s.P[symi<D>(r < c ? r : c, r < c ? c : r)];
    }
}

// (m, v) the smoothed law of f_k given ALL observations, y its observation with noise variance R > 0: the law of y_k given
// the others is N((m R - y v) / (R - v), R^2 / (R - v)) (v < R: the posterior of f_k is narrower than the factor it contains).
// At a missing step nothing is left out: N(m, v + R), and no density.
template <typename T>
__device__ __forceinline__ void loo_step(T m, T v, T R, T y, T& mean, T& var, LogLik& lpd) {
    if (is_nan(y)) {
        mean = m;
        var = v + R;
        return;
    }
    const T c = R / (R - v);
    mean = c * (m - y * (v / R));
    var = c * R;
    lpd.add(ll_diff(y, mean), ll_wide(var));
}

// ---------------------------------------------------------------------------------------------
// one Newton step of a Laplace approximation: a compile-time flavour of the smoother, SITE, off by
// default -- the other instantiations are what they were.  The pass smooths Gaussian sites N(z_k | f_k, s_k) (the Kalman pass
// before it is the HET one over (zs, ss), R = 0); the smoother projects at every step as LOO does, and the epilogue site_step
// forms alpha_k, evaluates the likelihood at the new f_k (pgps_lik.h), stores the new iterate and the sites formed at it, and
// accumulates the pass's sums per lane; one set of partials per workgroup (GpSiteOut::part), summed afterwards in a fixed
// order.  sms / sPs are not written.  Instantiated in pgps_site_inst.hip only.
// ---------------------------------------------------------------------------------------------
struct SiteAcc {
    double lp = 0.0, fa = 0.0, corr = 0.0, dmax = 0.0, count = 0.0;
};

// a maximum that keeps a NaN once it has met one (fmax would drop it: a diverged iterate must not read as converged)
__device__ __forceinline__ double max_nan(double a, double b) {
    return (b > a || b != b) ? b : a;
}

// the workgroup's maximum (block_sum_double's shape: waves by shuffles, then one LDS word per wave)
__device__ __forceinline__ double block_max_nan(double x, double* lds) {
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) x = max_nan(x, __shfl_down(x, s, kWave));
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    if (lane == 0) lds[wave] = x;
    __syncthreads();
    double t = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t = max_nan(t, lds[w]);
    __syncthreads();
    return t;
}

// (f, v) the smoothed law of f_k; (z, s) the site the pass used there (z NaN: none); y the observation; fp the iterate the site
// was formed at
template <typename T>
__device__ __forceinline__ void site_step(const GpSiteOut<T>& so, long k, T f, T v, T z, T s, T y, T fp, bool have_prev,
                                          SiteAcc& acc) {
    const double fd = double(f);
    const double alpha = is_nan(z) ? 0.0 : (double(z) - fd) / double(s);
    double z_new = double(y), s_new = 1.0;           // (y is NaN at a missing row)
    if (!is_nan(y)) {
        const LikSite ls = lik_site(so.lik, so.par, double(y), fd);
        z_new = ls.z;
        s_new = ls.s;
        acc.lp += ls.lp;
        acc.corr += ls.corr;
        acc.count += 1.0;
    }
    acc.fa += fd * alpha;
    if (have_prev) acc.dmax = max_nan(acc.dmax, fabs(fd - double(fp)));
    so.f_out[k] = f;
    so.v_out[k] = v;
    so.alpha_out[k] = T(alpha);
    so.zs_out[k] = T(z_new);
    so.ss_out[k] = T(s_new);
}

// ---------------------------------------------------------------------------------------------
// reduce
// ---------------------------------------------------------------------------------------------
// LDS of the fused kernels: declared once per kernel and handed to the bodies, so that the one-launch kernel (below), which
// runs the three bodies one after the other, pays for the largest of them and not for their sum
template <typename T, int D>
struct GpLds {
    static constexpr int G = 4;
    using GF = StageGeom<D * D * (int)sizeof(T), G>;
    using GM = StageGeom<D * (int)sizeof(T), G>;
    T lds[kWaves * Dim<D>::NFILT];
    double lds_ll[kWaves];
    __attribute__((aligned(16))) char stage[kWaves][GF::BYTES + GM::BYTES];
};

template <typename T, int D, bool HET = false>
__device__ __forceinline__ void gp_reduce_body(const GpArgs<T>& g, T* lds, const T* rs = nullptr) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM;
    using FE = FiltElem<T, D>;
    const ScanArgs<T>& a = g.s;
    T h[D], P0[SYM];
    gp_prior<T, D>(g.m, h, P0);
    const long gt = (long)blockIdx.x * kBlock + threadIdx.x;
    const long k0 = gt * a.Lc;
    const long k1 = min(a.N, k0 + a.Lc);
    FE agg;
    filt_identity(agg);
    if (k0 < k1) {
        T tprev = (k0 > 0) ? g.m.ts[k0 - 1] : g.m.t_prev;
        T tn = g.m.ts[k0], yn = a.ys[k0];
        [[maybe_unused]] T rn = T(0);
        if constexpr (HET) rn = rs[k0];
        for (long k = k0; k < k1; ++k) {
            const T t = tn, y = yn;
            [[maybe_unused]] const T rk = rn;
            if (k + 1 < k1) {
                tn = g.m.ts[k + 1]; yn = a.ys[k + 1];
                if constexpr (HET) rn = rs[k + 1];
            }
            T Rk = a.R;
            if constexpr (HET) Rk = het_noise(a.R, rk, y);
            if (k == 0) {
                filt_first(agg, P0, y, h, Rk);
            } else {
                T F[MAT], Qf[MAT], Q[SYM];
                lti_step<T, D>(g.m, t - tprev, F, Qf);
                sym_from_full<T, D>(Qf, Q);
                filt_extend(agg, F, Q, y, h, Rk);
            }
            tprev = t;
        }
    }
    FE excl, total;
    block_scan_exclusive<FE, true>(agg, excl, total, lds);
    ws_store(a.lpre, a.nlanes, gt, excl);
    if (threadIdx.x == 0) rec_store(a.spine + (long)blockIdx.x * Dim<D>::NFILT, total);
}

template <typename T, int D>
__global__ __launch_bounds__(kBlock) void k_gp_reduce(const GpArgs<T> g) {
    __shared__ T lds[kWaves * Dim<D>::NFILT];
    gp_reduce_body<T, D>(g, lds);
}

// ---------------------------------------------------------------------------------------------
// apply (+ log-likelihood, + smoothing aggregates when SMOOTH); fms / fPs are written when non-null
// ---------------------------------------------------------------------------------------------
template <typename T, int D, bool SMOOTH, bool NT, bool HET = false, bool OSA = false>
__device__ __forceinline__ void gp_apply_body(const GpArgs<T>& g, GpLds<T, D>& sh, const T* rs = nullptr,
                                              const GpLooOut<T>& lo = GpLooOut<T>{}) {
    constexpr int MAT = D * D, SYM = Dim<D>::SYM, NF = Dim<D>::NFILT, G = 4;
    using FE = FiltElem<T, D>;
    using SE = SmthElem<T, D>;
    using MC = MeanCov<T, D>;
    using GF = StageGeom<MAT * (int)sizeof(T), G>;
    using GM = StageGeom<D * (int)sizeof(T), G>;
    const ScanArgs<T>& a = g.s;
    T* lds = sh.lds;
    double* lds_ll = sh.lds_ll;
    auto& stage = sh.stage;
    (void)NF;

    T h[D];
    MC s;
    gp_prior<T, D>(g.m, h, s.P);
#pragma unroll
    for (int i = 0; i < D; ++i) s.m[i] = T(0);

    const long gt = (long)blockIdx.x * kBlock + threadIdx.x;
    const long k0 = gt * a.Lc;
    const long k1 = min(a.N, k0 + a.Lc);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const long wbase = ((long)blockIdx.x * kBlock + wave * kWave) * a.Lc;
    const bool store = (a.fms != nullptr);
    const bool staged = store && (wbase + (long)kWave * a.Lc <= a.N) && (a.Lc % G == 0);

    FE left_part, lp;
    MC s_short;
    const bool shortcut = a.shortcut != 0 && blockIdx.x > 0 && carry_shortcut_filter<T, D>(a.spine, (int)blockIdx.x - 1, s_short);
    if (blockIdx.x > 0 && !shortcut) fold_spine_partial<FE>(a.spine, 0, (int)blockIdx.x, left_part);
    ws_load(a.lpre, a.nlanes, gt, lp);
    T tprev = T(0), tn = T(0), yn = T(0);
    [[maybe_unused]] T rn = T(0);
    if (k0 < k1) {
        tprev = (k0 > 0) ? g.m.ts[k0 - 1] : g.m.t_prev;
        tn = g.m.ts[k0];
        yn = a.ys[k0];
        if constexpr (HET) rn = rs[k0];
    }
    if (shortcut) {
        s = s_short;
    } else if (blockIdx.x > 0) {
        FE left;
        block_reduce_ordered(left_part, left, lds);
        filt_apply(s, left);
    }
    filt_apply(s, lp);

    LogLik ll;
    SE sagg;
    smth_identity(sagg);
    char* lP = stage[wave];
    char* lM = lP + GF::BYTES;
    const long pitchF = (long)a.Lc * MAT * sizeof(T), pitchM = (long)a.Lc * D * sizeof(T);
    char* gP = reinterpret_cast<char*>(a.fPs + wbase * MAT);
    char* gM = reinterpret_cast<char*>(a.fms + wbase * D);
    if (k0 < k1) {
        for (long k = k0; k < k1; ++k) {
            const T t = tn, y = yn;
            [[maybe_unused]] const T rk = rn;
            if (k + 1 < a.N && (k + 1 < k1 || SMOOTH)) tn = g.m.ts[k + 1];
            if (k + 1 < k1) {
                yn = a.ys[k + 1];
                if constexpr (HET) rn = rs[k + 1];
            }
            T F[MAT], Qf[MAT];
            lti_step<T, D>(g.m, t - tprev, F, Qf);
            tprev = t;
            if constexpr (OSA) {
                T mu, S, Rk = a.R, Rs = a.R;
                if constexpr (HET) {
                    Rk = het_noise(a.R, rk, y);
                    Rs = a.R + rk;
                }
                gp_apply_step_osa<T, D, SMOOTH>(a, k, k0, F, Qf, y, h, Rk, Rs, s, ll, sagg, mu, S);
                if (lo.osa_mean) lo.osa_mean[k] = mu;
                if (lo.osa_var) lo.osa_var[k] = S;
            } else if constexpr (HET) gp_apply_step_r<T, D, SMOOTH>(a, k, k0, F, Qf, y, h, het_noise(a.R, rk, y), s, ll, sagg);
            else filter_apply_step<T, D, SMOOTH>(a, k, k0, F, Qf, y, h, s, ll, sagg);
            if (store) {
                T Pf[MAT];
                full_from_sym<T, D>(s.P, Pf);
                if (staged) {
                    const int i = (int)((k - k0) % G);
                    if (i == 0) wave_lds_sync();
                    stage_put<GM, T, D>(lM, i, s.m);
                    stage_put<GF, T, MAT>(lP, i, Pf);
                    if (i == G - 1) {
                        const long sb = (k - k0) / G;
                        wave_lds_sync();
                        stage_drain<GM, NT>(gM + sb * GM::SEG, pitchM, lM);
                        stage_drain<GF, NT>(gP + sb * GF::SEG, pitchF, lP);
                    }
                } else {
                    store_rec<T, D>(a.fms + k * D, s.m);
                    store_rec<T, MAT>(a.fPs + k * MAT, Pf);
                }
            }
        }
        if (SMOOTH) {
            T F[MAT], Qf[MAT];
            const bool have_next = (k1 < a.N);
            if (have_next) lti_step<T, D>(g.m, tn - tprev, F, Qf);
            filter_tail_apply<T, D>(have_next, F, Qf, s, sagg);
        }
    }
    {
        const double v = ll.value();
        const double t = block_sum_double(v, lds_ll);
        if (threadIdx.x == 0) a.llpart[blockIdx.x] = t;
        if constexpr (!SMOOTH) {
            if (a.ll != nullptr && a.ll_in_apply) ll_finish(a.llpart, a.nblocks, a.ll, a.status + kLlTicketWord, lds_ll);
        }
    }
    if (SMOOTH) {
        SE excl, total;
        block_scan_exclusive<SE, false>(sagg, excl, total, lds);
        ws_store(a.lsuf, a.nlanes, gt, excl);
        if (threadIdx.x == 0) rec_store(a.sspine + (long)blockIdx.x * Dim<D>::NSMTH, total);
    }
    (void)lane;
}

template <typename T, int D, bool SMOOTH, bool NT>
__global__ __launch_bounds__(kBlock) void k_gp_apply(const GpArgs<T> g) {
    __shared__ GpLds<T, D> sh;
    gp_apply_body<T, D, SMOOTH, NT>(g, sh);
}

// ---------------------------------------------------------------------------------------------
// batched log-likelihood: B hyper-parameter settings over the same (ts, ys) in one pair of launches
// (HMC leapfrogs / grid search at the reference's realistic N of
// 1e3..1e5, where one series alone cannot fill the chip).  blockIdx.y selects the model; each model
// has its own slice of the scan scratch.  Same bodies, same arithmetic as the single-model launches.
// ---------------------------------------------------------------------------------------------
template <typename T, int D, bool PREDICT = false>
__device__ __forceinline__ GpArgs<T> gp_batch_select(const GpBatchArgs<T>& b) {
    const long m = blockIdx.y;
    const double* p = b.models + m * kGpModelStride;
    GpArgs<T> g{};
    g.s.N = b.N; g.s.Lc = b.Lc; g.s.nblocks = b.nblocks; g.s.nlanes = b.nlanes;
    g.s.seg_first = 1; g.s.seg_last = 1;
    g.s.ys = b.ys;
    g.s.R = T(p[31]);
    g.s.spine = b.spine + m * b.nblocks * Dim<D>::NFILT;
    g.s.lpre = b.lpre + m * b.nlanes * Dim<D>::NFILT;
    g.s.llpart = b.llpart + m * b.nblocks;
    g.m.lam = p[0];
#pragma unroll
    for (int i = 0; i < D * D; ++i) { g.m.N1[i] = p[1 + i]; g.m.N2[i] = p[10 + i]; g.m.Pinf[i] = p[19 + i]; }
#pragma unroll
    for (int i = 0; i < D; ++i) g.m.H[i] = T(p[28 + i]);
    g.m.ts = b.ts;
    g.m.t_prev = b.t_prev;
    if constexpr (PREDICT) {
        // predict (pgps_gp_predict_batch_*): the model's slices of the filtered moments and of the smoother's scan records,
        // its output rows and its log-likelihood; the merged series and its query slots are shared.  A compile-time flavour: the
        // log-likelihood kernels keep fms == nullptr a constant, so their store path is compiled out as it always was
        g.s.fms = b.fms + m * b.bs_fm;
        g.s.fPs = b.fPs + m * b.bs_fP;
        g.s.sspine = b.sspine + m * b.nblocks * Dim<D>::NSMTH;
        g.s.lsuf = b.lsuf + m * b.nlanes * Dim<D>::NSMTH;
        g.s.ll = b.ll + m;
        g.qslot = b.qslot;
        g.pmean = b.pmean + m * b.K;
        g.pvar = b.pvar + m * b.K;
    }
    return g;
}

template <typename T, int D>
__global__ __launch_bounds__(kBlock) void k_gpb_reduce(const GpBatchArgs<T> b) {
    const GpArgs<T> g = gp_batch_select<T, D>(b);
    __shared__ T lds[kWaves * Dim<D>::NFILT];
    gp_reduce_body<T, D>(g, lds);
}

template <typename T, int D, bool SMOOTH = false>
__global__ __launch_bounds__(kBlock) void k_gpb_apply(const GpBatchArgs<T> b) {
    const GpArgs<T> g = gp_batch_select<T, D, SMOOTH>(b);
    __shared__ GpLds<T, D> sh;
    gp_apply_body<T, D, SMOOTH, false>(g, sh);
}

// one workgroup per model: ll[m] = sum of its block partials
static __global__ __launch_bounds__(kBlock) void k_gpb_finalize(const double* llpart, int nblocks, double* ll) {
    __shared__ double lds_ll[kWaves];
    const double* p = llpart + (long)blockIdx.x * nblocks;
    double v = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kBlock) v += p[i];
    const double t = block_sum_double(v, lds_ll);
    if (threadIdx.x == 0) ll[blockIdx.x] = t;
}

// ---------------------------------------------------------------------------------------------
// smoother apply
// ---------------------------------------------------------------------------------------------
template <typename T, int D, bool NT, bool PROJ = false, bool LOO = false, bool SITE = false, bool LHET = false>
__device__ __forceinline__ void gp_smooth_body(const GpArgs<T>& g, GpLds<T, D>& sh, const GpLooOut<T>& lo = GpLooOut<T>{},
                                               const GpSiteOut<T>& so = GpSiteOut<T>{}, const T* rs = nullptr) {
    static_assert(!LHET || LOO, "LHET is a flavour of the leave-one-out epilogue");
    constexpr int MAT = D * D, SYM = Dim<D>::SYM, NS = Dim<D>::NSMTH, G = 4;
    using SE = SmthElem<T, D>;
    using MC = MeanCov<T, D>;
    using GF = StageGeom<MAT * (int)sizeof(T), G>;
    using GM = StageGeom<D * (int)sizeof(T), G>;
    const ScanArgs<T>& a = g.s;
    T* lds = sh.lds;                    // (NFILT >= NSMTH scalars per wave)
    double* lds_ll = sh.lds_ll;
    auto& stage = sh.stage;
    (void)NS;

    const long gt = (long)blockIdx.x * kBlock + threadIdx.x;
    const long k0 = gt * a.Lc;
    const long k1 = min(a.N, k0 + a.Lc);
    const int wave = threadIdx.x / kWave;
    const long wbase = ((long)blockIdx.x * kBlock + wave * kWave) * a.Lc;
    const bool staged = (wbase + (long)kWave * a.Lc <= a.N) && (a.Lc % G == 0);
    char* lP = stage[wave];
    char* lM = lP + GF::BYTES;
    const long pitchF = (long)a.Lc * MAT * sizeof(T), pitchM = (long)a.Lc * D * sizeof(T);
    const int S = a.Lc / G;

    SE right_part, ls;
    MC s_short;
    const bool has_right = (int)blockIdx.x + 1 < a.nblocks;
    const bool shortcut = a.shortcut != 0 && has_right && carry_shortcut_smoother<T, D>(a.sspine, (int)blockIdx.x + 1, s_short);
    if (has_right && !shortcut) fold_spine_partial<SE>(a.sspine, (int)blockIdx.x + 1, a.nblocks, right_part);
    ws_load(a.lsuf, a.nlanes, gt, ls);
    V4 rP[GF::NV], rM[GM::NV];
    const char* gP = reinterpret_cast<const char*>(a.fPs + wbase * MAT);
    const char* gM = reinterpret_cast<const char*>(a.fms + wbase * D);
    if (staged) {
        stage_issue<GF>(gP + (long)(S - 1) * GF::SEG, pitchF, rP);
        stage_issue<GM>(gM + (long)(S - 1) * GM::SEG, pitchM, rM);
    }
    T tnext = T(0), tcur = T(0);
    [[maybe_unused]] T ycur = T(0), rcur = T(0);         // (rcur: LHET, the step's given variance, loaded as ycur is)
    [[maybe_unused]] LogLik lpd;
    // SITE: the step's site (a.ys = zs, so.ss), its observation and the previous iterate, loaded a step ahead as ycur is
    [[maybe_unused]] T scur = T(0), ocur = T(0), pcur = T(0);
    [[maybe_unused]] SiteAcc sacc;
    [[maybe_unused]] bool have_prev = false;
    if constexpr (SITE) have_prev = so.f_prev != nullptr;
    if (k0 < k1) {
        tnext = (k1 < a.N) ? g.m.ts[k1] : T(0);
        tcur = g.m.ts[k1 - 1];
        if constexpr (LOO || SITE) ycur = a.ys[k1 - 1];
        if constexpr (LHET) rcur = rs[k1 - 1];
        if constexpr (SITE) {
            scur = so.ss[k1 - 1];
            ocur = so.ys[k1 - 1];
            if (have_prev) pcur = so.f_prev[k1 - 1];
        }
    }
    MC s;
#pragma unroll
    for (int i = 0; i < D; ++i) s.m[i] = T(0);
#pragma unroll
    for (int i = 0; i < SYM; ++i) s.P[i] = T(0);
    if (shortcut) {
        s = s_short;
    } else if ((int)blockIdx.x + 1 < a.nblocks) {
        SE right;
        block_reduce_ordered(right_part, right, lds);
        smth_apply(right, s);
    }
    smth_apply(ls, s);

    if (k0 < k1) {
        char* oP = reinterpret_cast<char*>(a.sPs + wbase * MAT);
        char* oM = reinterpret_cast<char*>(a.sms + wbase * D);
        for (long k = k1 - 1; k >= k0; --k) {
            const int i = (int)((k - k0) % G);
            const long sb = (k - k0) / G;
            if (staged && i == G - 1) {
                wave_lds_sync();
                stage_commit<GF>(lP, rP);
                stage_commit<GM>(lM, rM);
                if (sb > 0) {
                    stage_issue<GF>(gP + (sb - 1) * GF::SEG, pitchF, rP);
                    stage_issue<GM>(gM + (sb - 1) * GM::SEG, pitchM, rM);
                }
                wave_lds_sync();
            }
            T mk[D], Pk[MAT];
            if (staged) {
                stage_get<GM, T, D>(lM, i, mk);
                stage_get<GF, T, MAT>(lP, i, Pk);
            } else {
                load_rec<T, D>(a.fms + k * D, mk);
                load_rec<T, MAT>(a.fPs + k * MAT, Pk);
            }
            const T t = tcur;
            if (k > 0) tcur = g.m.ts[k - 1];
            [[maybe_unused]] const T y = ycur;
            [[maybe_unused]] const T rk = rcur;
            if constexpr (LOO || SITE) {
                if (k > k0) {
                    ycur = a.ys[k - 1];
                    if constexpr (LHET) rcur = rs[k - 1];
                }
            }
            [[maybe_unused]] const T sk = scur, ok = ocur, pk = pcur;
            if constexpr (SITE) {
                if (k > k0) {
                    scur = so.ss[k - 1];
                    ocur = so.ys[k - 1];
                    if (have_prev) pcur = so.f_prev[k - 1];
                }
            }
            const bool last = (k == a.N - 1);
            T F[MAT], Qf[MAT];
            if (!last) lti_step<T, D>(g.m, tnext - t, F, Qf);
            smoother_apply_step<T, D>(F, Qf, mk, Pk, last, s);
            tnext = t;
            if constexpr (LOO) {
                // the leave-one-out law of y_k at every step; sms / sPs are not written
                T m, v, mean, var;
                gp_project<T, D>(g.m, s, m, v);
                T Rk = a.R;
                if constexpr (LHET) Rk = a.R + rk;          // (as stored: a missing row's variance is v + R + rs[k])
                loo_step(m, v, Rk, y, mean, var, lpd);
                if (lo.loo_mean) lo.loo_mean[k] = mean;
                if (lo.loo_var) lo.loo_var[k] = var;
                continue;
            }
            if constexpr (SITE) {
                // the new iterate and the sites formed at it, at every step; sms / sPs are not written
                T m, v;
                gp_project<T, D>(g.m, s, m, v);
                site_step(so, k, m, v, y, sk, ok, pk, have_prev, sacc);
                continue;
            }
            if constexpr (PROJ) {
                // posterior of f = H x at the query rows only (pssgp/model.py:107-111)
                const int q = g.qslot[k];
                if (q >= 0) {
                    T mu, var;
                    gp_project<T, D>(g.m, s, mu, var);
                    g.pmean[q] = mu;
                    g.pvar[q] = var;
                }
                continue;
            }
            T Pf[MAT];
            full_from_sym<T, D>(s.P, Pf);
            if (staged) {
                stage_put<GM, T, D>(lM, i, s.m);
                stage_put<GF, T, MAT>(lP, i, Pf);
                if (i == 0) {
                    wave_lds_sync();
                    stage_drain<GM, NT>(oM + sb * GM::SEG, pitchM, lM);
                    stage_drain<GF, NT>(oP + sb * GF::SEG, pitchF, lP);
                }
            } else {
                store_rec<T, D>(a.sms + k * D, s.m);
                store_rec<T, MAT>(a.sPs + k * MAT, Pf);
            }
        }
    }
    if constexpr (LOO) {
        const double t = block_sum_double(lpd.value(), lds_ll);
        if (threadIdx.x == 0) lo.lpd_part[blockIdx.x] = t;
    }
    if constexpr (SITE) {
        const double vals[4] = {sacc.lp, sacc.fa, sacc.corr, sacc.count};
        const int slot[4] = {0, 1, 2, 4};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double t = block_sum_double(vals[i], lds_ll);
            if (threadIdx.x == 0) so.part[(long)slot[i] * a.nblocks + blockIdx.x] = t;
        }
        const double mx = block_max_nan(sacc.dmax, lds_ll);
        if (threadIdx.x == 0) so.part[3L * a.nblocks + blockIdx.x] = mx;
    }
    if (blockIdx.x == 0 && a.ll != nullptr) {
        double v = 0.0;
        for (int b = threadIdx.x; b < a.nblocks; b += kBlock) v += a.llpart[b];
        const double t = block_sum_double(v, lds_ll);
        if (threadIdx.x == 0) *a.ll = t;
    }
}

template <typename T, int D, bool NT, bool PROJ = false>
__global__ __launch_bounds__(kBlock) void k_gp_smooth(const GpArgs<T> g) {
    __shared__ GpLds<T, D> sh;
    gp_smooth_body<T, D, NT, PROJ>(g, sh);
}

// ---------------------------------------------------------------------------------------------
// ONE launch for a short series (round 3): the reference's own lengths are N = 200 .. 10^4 per call
// (pssgp/experiments/toy_models/mcmc.py:55, speed_and_stability.py:73), where three dependent launches of a few
// workgroups each cost more in launch gaps than in work.  A single workgroup runs the three bodies above one after
// the other -- its lanes own up to kOneLaunchSteps consecutive steps each, nblocks = 1, so there is no spine to fold and
// the "inter-workgroup" scratch (lpre, lsuf, the filtered moments) is written and read back by the same CU behind a
// workgroup barrier.  SMOOTH: 0 = log-likelihood (and filtered moments when asked for), 1 = + smoother, 2 = + smoother
// in projection mode (predict_f).
// ---------------------------------------------------------------------------------------------
template <typename T, int D, int SMOOTH>
__global__ __launch_bounds__(kBlock) void k_gp_one(const GpArgs<T> g) {
    __shared__ GpLds<T, D> sh;
    gp_reduce_body<T, D>(g, sh.lds);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    gp_apply_body<T, D, SMOOTH != 0, false>(g, sh);
    if constexpr (SMOOTH != 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        gp_smooth_body<T, D, false, SMOOTH == 2>(g, sh);
    } else {
        if (threadIdx.x == 0 && g.s.ll != nullptr) *g.s.ll = g.s.llpart[0];      // (this lane wrote the partial)
    }
}

// ---------------------------------------------------------------------------------------------
// batched predict_f (pgps_gp_predict_batch_*): B models over one merged series.  Two forms, the same three bodies:
//   k_gpb_reduce, k_gpb_apply<.., true>, k_gpb_smooth   three launches of (nblocks, B) workgroups;
//   k_gpb_one                                           ONE workgroup per model (grid (1, B): blockIdx.x stays the
//                                                       workgroup's index inside its series), the three bodies back to
//                                                       back as k_gp_one<.., 2> runs them: no spine, no second launch, and
//                                                       with B >= the number of CUs no CU idles as it does for a single model.
// Every model has its own slices of the scratch (gp_batch_select), so workgroups of different models share nothing but the
// read-only series.
// ---------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(kBlock) void k_gpb_smooth(const GpBatchArgs<T> b) {
    const GpArgs<T> g = gp_batch_select<T, D, true>(b);
    __shared__ GpLds<T, D> sh;
    gp_smooth_body<T, D, false, true>(g, sh);
}

template <typename T, int D>
__global__ __launch_bounds__(kBlock) void k_gpb_one(const GpBatchArgs<T> b) {
    const GpArgs<T> g = gp_batch_select<T, D, true>(b);
    __shared__ GpLds<T, D> sh;
    gp_reduce_body<T, D>(g, sh.lds);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    gp_apply_body<T, D, true, false>(g, sh);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    gp_smooth_body<T, D, false, true>(g, sh);
}

}  // namespace pgps
