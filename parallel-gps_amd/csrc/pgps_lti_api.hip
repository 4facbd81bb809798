// pgps_lti_api.hip -- general LTI models on the device (include/pgps.h, fp64, 2 <= d <= 32): log-likelihood, predict_f, the
// adjoint gradient, the batched log-likelihood and predict_f, and the array-path front the model-level sampler and joint
// covariance share.  The kernels are the row-, wave-cooperative and two-rows units'.
#include "pgps_host.h"
#include "pgps_gradlti.h"
#include "pgps_scratch.h"

using namespace pgps;

// ---------------------------------------------------------------------------------------------
// general LTI models on the device (fp64, 2 <= d <= 16): _get_ssm -> pkf / pkfs for any kernel, with
// nothing but the results leaving the GPU (row-cooperative kernels, pgps_rc.hip.h)
// ---------------------------------------------------------------------------------------------
// H sm and H sP H^T at the query rows of a merged series (the general-LTI predict path above d = 16, where the smoother
// writes whole moments): one thread per merged step
__global__ void k_project_rows(long m, int d, const int* __restrict__ qslot, const double* __restrict__ H,
                               const double* __restrict__ sms, const double* __restrict__ sPs, double* __restrict__ mean,
                               double* __restrict__ var) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int q = qslot[k];
    if (q < 0) return;
    const double* sm = sms + k * d;
    const double* sP = sPs + k * (long)d * d;
    double mu = 0.0, v = 0.0;
    for (int i = 0; i < d; ++i) {
        mu += H[i] * sm[i];
        double r = 0.0;
        for (int j = 0; j < d; ++j) r += sP[(long)i * d + j] * H[j];
        v += H[i] * r;
    }
    mean[q] = mu;
    var[q] = v;
}

// ... and its J-row sibling (pgps_lti_predict_lin_*): C sm (J) and C sP C^T (J, J) at the query rows, one thread per merged
// step.  One pass over the rows of sP: t_j = sP[a, :] c_j, then M[i][j] += c_i[a] t_j for i <= j; the mirror is a copy, so
// the block is symmetric bit for bit.  The loops over the functionals have compile-time bounds (the J x J accumulators stay
// in registers) and uniform guards; the rows of C are wave-uniform loads.
__global__ void k_project_rows_lin(long m, int d, int J, const int* __restrict__ qslot, const double* __restrict__ C,
                                   const double* __restrict__ sms, const double* __restrict__ sPs, double* __restrict__ mean,
                                   double* __restrict__ cov) {
    constexpr int JM = PGPS_MAX_FUNCTIONALS;
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int q = qslot[k];
    if (q < 0) return;
    const double* sm = sms + k * d;
    const double* sP = sPs + k * (long)d * d;
    double mu[JM], M[JM][JM];
#pragma unroll
    for (int i = 0; i < JM; ++i) {
        mu[i] = 0.0;
#pragma unroll
        for (int j = 0; j < JM; ++j) M[i][j] = 0.0;
    }
    for (int a = 0; a < d; ++a) {
        double t[JM];
#pragma unroll
        for (int j = 0; j < JM; ++j) t[j] = 0.0;
        for (int b = 0; b < d; ++b) {
            const double p = sP[(long)a * d + b];
#pragma unroll
            for (int j = 0; j < JM; ++j)
                if (j < J) t[j] += p * C[j * d + b];
        }
        const double s = sm[a];
#pragma unroll
        for (int i = 0; i < JM; ++i) {
            if (i < J) {
                const double ci = C[i * d + a];
                mu[i] += ci * s;
#pragma unroll
                for (int j = i; j < JM; ++j)
                    if (j < J) M[i][j] += ci * t[j];
            }
        }
    }
    double* mq = mean + (long)q * J;
    double* cq = cov + (long)q * J * J;
#pragma unroll
    for (int i = 0; i < JM; ++i) {
        if (i < J) {
            mq[i] = mu[i];
#pragma unroll
            for (int j = i; j < JM; ++j)
                if (j < J) { cq[i * J + j] = M[i][j]; cq[j * J + i] = M[i][j]; }
        }
    }
}

// Fs / Qs of a block-diagonal model from the per-block results: element (i, j) of block step k goes to
// (idx[i], idx[j]) of the big step k (the big arrays are zero elsewhere)
// (blockIdx.y = one of several blocks of the same size: their model records -- [F_b | P_b | indices] -- lie `mstride` doubles
// apart, their discretised arrays m db^2 apart)
__global__ void k_scatter_block(long m, int d, int db, const int* __restrict__ idx, const double* __restrict__ Fb,
                                const double* __restrict__ Qb, double* __restrict__ Fs, double* __restrict__ Qs, long mstride) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = (long)db * db;
    idx = reinterpret_cast<const int*>(reinterpret_cast<const double*>(idx) + (long)blockIdx.y * mstride);
    Fb += (long)blockIdx.y * m * per;
    Qb += (long)blockIdx.y * m * per;
    if (e >= m * per) return;
    const long k = e / per;
    const int r = (int)(e - k * per), i = r / db, j = r - i * db;
    const long dst = k * (long)d * d + (long)idx[i] * d + idx[j];
    Fs[dst] = Fb[e];
    Qs[dst] = Qb[e];
}

// Sum kernels give block-diagonal F and Pinf (pssgp/kernels/base.py:133-141), so expm(F dt) and Q are block-diagonal
// too: connected components of the sparsity pattern of |F| + |F^T| + |Pinf|, single states attached to the smallest
// block.  Returns the components (each sorted) when there are at least two and none is larger than `cap`.
// An entry counts as a coupling when it exceeds 1e-14 of its matrix's largest entry: a Pinf that came out of a Lyapunov
// solve carries rounding residue of that size between independent blocks, and dropping it moves the discretised
// operands by the same relative amount -- five orders below the parity tolerance.
static bool diagonal_blocks(int d, const double* F, const double* P, int cap, std::vector<std::vector<int>>& blocks) {
    std::vector<int> comp(d);
    for (int i = 0; i < d; ++i) comp[i] = i;
    auto find = [&](int x) { while (comp[x] != x) x = comp[x] = comp[comp[x]]; return x; };
    double fmax = 0.0, pmax = 0.0;
    for (int i = 0; i < d * d; ++i) { fmax = std::max(fmax, std::fabs(F[i])); pmax = std::max(pmax, std::fabs(P[i])); }
    const double ftol = 1e-14 * fmax, ptol = 1e-14 * pmax;
    auto coupled = [&](int i, int j) { return std::fabs(F[i * d + j]) > ftol || std::fabs(P[i * d + j]) > ptol; };
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j)
            if (i != j && (coupled(i, j) || coupled(j, i))) {
                const int a = find(i), b = find(j);
                if (a != b) comp[a] = b;
            }
    blocks.clear();
    std::vector<int> slot(d, -1);
    for (int i = 0; i < d; ++i) {
        const int r = find(i);
        if (slot[r] < 0) { slot[r] = (int)blocks.size(); blocks.emplace_back(); }
        blocks[slot[r]].push_back(i);
    }
    // single states: the row-cooperative discretisation starts at d = 2
    for (size_t b = 0; b < blocks.size();) {
        if (blocks[b].size() == 1 && blocks.size() > 1) {
            size_t best = blocks.size();
            for (size_t o = 0; o < blocks.size(); ++o)
                if (o != b && (best == blocks.size() || blocks[o].size() < blocks[best].size())) best = o;
            blocks[best].push_back(blocks[b][0]);
            std::sort(blocks[best].begin(), blocks[best].end());
            blocks.erase(blocks.begin() + (long)b);
            b = 0;
        } else {
            ++b;
        }
    }
    if (blocks.size() < 2) return false;
    for (auto& bl : blocks)
        if ((int)bl.size() > cap || bl.size() < 2) return false;
    return true;
}

// 16 < d <= 32: the same chain on the wave-cooperative kernels -- discretisation with Qs written out, whole filtered (and
// smoothed) moments into scratch, projection at the query rows by k_project_rows.  Everything stays on the device.
// discretisation of the d <= 32 road into the context's scratch: Fs, Qs (m, d, d)
static int lti_disc_wc(pgps_ctx* ctx, size_t m, int d, const double* model, const double* F_host, const double* P_host,
                       const double* ts_m, double t0, double** Fs_out, double** Qs_out) {
    const size_t dd = (size_t)d * d;
    double *Fs, *Qs;
    TRY(stage_in<double>(ctx, ctx->lti[4], nullptr, m * dd, &Fs));
    TRY(stage_in<double>(ctx, ctx->lti[5], nullptr, m * dd, &Qs));
    std::vector<std::vector<int>> blocks;
    if (diagonal_blocks(d, F_host, P_host, rc::kDimMax, blocks)) {
        // block-diagonal model (a sum kernel): every block through the row-cooperative discretisation (Pade in
        // registers, ~20x the rate of wc_discretise), scattered into zeroed Fs / Qs
        HIPCHK(ctx, hipMemsetAsync(Fs, 0, m * dd * sizeof(double), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(Qs, 0, m * dd * sizeof(double), ctx->stream));
        // blocks of the same size go together: one batched discretisation launch and one scatter launch per SIZE (the CO2
        // kernel's six blocks -- 4, 4, 4, 2, 2, 2 -- are two launches of each instead of six: a launch is ~8 us of a 0.6 ms
        // evaluation at the experiment's 3192 points)
        std::stable_sort(blocks.begin(), blocks.end(), [](const std::vector<int>& a, const std::vector<int>& b) { return a.size() < b.size(); });
        size_t small = 0, big = 0;
        for (size_t b = 0; b < blocks.size();) {
            size_t e = b;
            while (e < blocks.size() && blocks[e].size() == blocks[b].size()) ++e;
            const size_t db = blocks[b].size();
            small += (e - b) * (2 * db * db + (db + 1) / 2 * 2);                // F_b, P_b, indices (ints, padded)
            big = std::max(big, (e - b) * db * db);
            b = e;
        }
        double *bm, *Fb, *Qb;
        TRY(stage_in<double>(ctx, ctx->lti[10], nullptr, small, &bm));
        TRY(stage_in<double>(ctx, ctx->lti[11], nullptr, 2 * m * big, &Fb));
        Qb = Fb + m * big;
        std::vector<double> hb(small);
        size_t off = 0;
        std::vector<size_t> offs;
        for (auto& bl : blocks) {
            const size_t db = bl.size();
            offs.push_back(off);
            for (size_t i = 0; i < db; ++i)
                for (size_t j = 0; j < db; ++j) {
                    hb[off + i * db + j] = F_host[bl[i] * d + bl[j]];
                    hb[off + db * db + i * db + j] = P_host[bl[i] * d + bl[j]];
                }
            int* ip = reinterpret_cast<int*>(&hb[off + 2 * db * db]);
            for (size_t i = 0; i < db; ++i) ip[i] = bl[i];
            off += 2 * db * db + (db + 1) / 2 * 2;
        }
        HIPCHK(ctx, hipMemcpyAsync(bm, hb.data(), small * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        // (pageable source: staged by the runtime before the call returns, as for the model in lti_dev)
        for (size_t b = 0; b < blocks.size();) {
            size_t e = b;
            while (e < blocks.size() && blocks[e].size() == blocks[b].size()) ++e;
            const int db = (int)blocks[b].size(), nb = (int)(e - b);
            const long mstride = 2L * db * db + (db + 1) / 2 * 2;
            const double* Fd = bm + offs[b];
            TRY(launch_disc_rc(ctx, (long)m, db, Fd, Fd + db * db, ts_m, t0, Fb, Qb, nb, mstride));
            const long total = (long)m * db * db;
            hipLaunchKernelGGL(k_scatter_block, dim3((unsigned)((total + 255) / 256), (unsigned)nb), dim3(256), 0, ctx->stream,
                               (long)m, d, db, reinterpret_cast<const int*>(Fd + 2 * db * db), (const double*)Fb,
                               (const double*)Qb, Fs, Qs, mstride);
            HIPCHK(ctx, hipGetLastError());
            b = e;
        }
    } else {
        TRY(launch_disc_wc<double>(ctx, (long)m, d, model, model + dd, ts_m, t0, Fs, Qs));
    }
    *Fs_out = Fs;
    *Qs_out = Qs;
    return PGPS_OK;
}

static int lti_dev_wc(pgps_ctx* ctx, size_t m, int d, const double* model, const double* F_host, const double* P_host,
                      double R, const double* ts_m, const double* ys_m, double t0, const int* qslot, double* mean,
                      double* var, double* ll, const LtiLin* lin) {
    const size_t dd = (size_t)d * d;
    double *Fs, *Qs, *fms, *fPs;
    TRY(lti_disc_wc(ctx, m, d, model, F_host, P_host, ts_m, t0, &Fs, &Qs));
    ScanArgs<double> a{};
    a.N = (long)m; a.seg_first = 1; a.seg_last = 1;
    a.P0 = model + dd; a.H = model + 2 * dd; a.R = R; a.Fs = Fs; a.Qs = Qs; a.ys = ys_m;
    a.ll = ll;
    TRY(stage_in<double>(ctx, ctx->lti[6], nullptr, m * dd, &fPs));
    TRY(stage_in<double>(ctx, ctx->lti[7], nullptr, m * d, &fms));
    a.fms = fms; a.fPs = fPs;
    if (!qslot) return launch_scan_wc<double>(ctx, a, d, MODE_PKF);
    // smoothed moments in place of the filtered ones is not possible (the smoother reads both): two more buffers
    double *sms, *sPs;
    TRY(stage_in<double>(ctx, ctx->lti[8], nullptr, m * dd, &sPs));
    TRY(stage_in<double>(ctx, ctx->lti[9], nullptr, m * d, &sms));
    a.sms = sms; a.sPs = sPs;
    TRY(launch_scan_wc<double>(ctx, a, d, MODE_PKFS));
    const int block = 256;
    if (lin) {      // (the rows of C follow H in the model block: lti_model_in; a thread's step is J d^2 products: small blocks)
        hipLaunchKernelGGL(k_project_rows_lin, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, ctx->stream, (long)m, d, lin->J, qslot,
                           a.H + d, (const double*)sms, (const double*)sPs, mean, lin->cov);
        HIPCHK(ctx, hipGetLastError());
        return PGPS_OK;
    }
    hipLaunchKernelGGL(k_project_rows, dim3((unsigned)((m + block - 1) / block)), dim3(block), 0, ctx->stream, (long)m, d,
                       qslot, a.H, (const double*)sms, (const double*)sPs, mean, var);
    HIPCHK(ctx, hipGetLastError());
    return PGPS_OK;
}

// the small model [F | Pinf | H] from host memory, in ONE copy (three pageable copies were 15 us of a short series' call;
// the source is staged by the runtime before the call returns, so it may change afterwards)
int pgps::lti_model_in(pgps_ctx* ctx, int d, const double* F, const double* Pinf, const double* H, double** model,
                       const double* C, int J) {
    const size_t dd = (size_t)d * d, nc = C ? (size_t)J * d : 0;
    if (C && (J < 1 || J > PGPS_MAX_FUNCTIONALS)) return PGPS_E_INVALID;
    TRY(ensure(ctx, ctx->lti[0], (2 * dd + d + nc) * sizeof(double)));
    *model = (double*)ctx->lti[0].p;
    double host[2 * PGPS_MAX_DIM * PGPS_MAX_DIM + PGPS_MAX_DIM + PGPS_MAX_FUNCTIONALS * PGPS_MAX_DIM];
    std::memcpy(host, F, dd * sizeof(double));
    std::memcpy(host + dd, Pinf, dd * sizeof(double));
    std::memcpy(host + 2 * dd, H, (size_t)d * sizeof(double));
    if (C) std::memcpy(host + 2 * dd + d, C, nc * sizeof(double));
    HIPCHK(ctx, hipMemcpyAsync(*model, host, (2 * dd + d + nc) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return PGPS_OK;
}

// m steps (training and query rows merged: qslot != nullptr marks the query rows and asks for the posterior there),
// everything on the device except the model
int pgps::lti_core(pgps_ctx* ctx, size_t m, int d, const double* F, const double* Pinf, const double* H, double R,
                    const double* ts_m, const double* ys_m, double t0, const int* qslot, double* mean, double* var,
                    double* ll, const LtiLin* lin) {
    const size_t dd = (size_t)d * d;
    double* model;
    if (lin && !qslot) return PGPS_E_INVALID;
    TRY(lti_model_in(ctx, d, F, Pinf, H, &model, lin ? lin->C : nullptr, lin ? lin->J : 0));
    double *Fs, *Qs = nullptr, *dll;
    TRY(stage_in<double>(ctx, ctx->st[11], nullptr, 2, &dll));
    if (d > rc::kDimMax) return lti_dev_wc(ctx, m, d, model, F, Pinf, R, ts_m, ys_m, t0, qslot, mean, var, ll ? ll : dll, lin);
    TRY(stage_in<double>(ctx, ctx->lti[4], nullptr, m * dd, &Fs));
    // the process noise stays implicit in both calls (Q_k = Pinf - F_k Pinf F_k^T inside the predict step): Qs is
    // never formed
    TRY(launch_disc_rc(ctx, (long)m, d, model, model + dd, ts_m, t0, Fs, Qs));
    ScanArgs<double> a{};
    a.N = (long)m; a.seg_first = 1; a.seg_last = 1;
    a.P0 = model + dd; a.H = model + 2 * dd; a.R = R; a.Fs = Fs; a.Qs = Qs; a.ys = ys_m;
    a.ll = ll ? ll : dll;
    if (!qslot) return launch_scan_rc_proj(ctx, a, d, MODE_PKF, nullptr, nullptr, nullptr);
    // scratch for the smoothing elements (E, g) where pkfs would have sPs, sms
    TRY(stage_in<double>(ctx, ctx->lti[6], nullptr, m * dd, &a.sPs));
    TRY(stage_in<double>(ctx, ctx->lti[7], nullptr, m * d, &a.sms));
    if (lin) return launch_scan_rc_proj(ctx, a, d, MODE_PKFS, qslot, mean, nullptr, lin->J, model + 2 * dd + d, lin->cov);
    return launch_scan_rc_proj(ctx, a, d, MODE_PKFS, qslot, mean, var);
}

// The array-path front of the model-level sampler and joint covariance (pgps_post_api.hip): explicit Fs, Qs and whole
// filtered (smoothed) moments, where lti_core keeps the process noise implicit and writes nothing per step
int pgps::lti_filter_front(pgps_ctx* ctx, size_t m, int d, const double* F, const double* Pinf, const double* H, double R,
                           const double* ts_m, const double* ys_m, double t0, bool smooth, double* ll, LtiFront* o) {
    const size_t dd = (size_t)d * d;
    double* dll;
    TRY(lti_model_in(ctx, d, F, Pinf, H, &o->model));
    TRY(stage_in<double>(ctx, ctx->lti[4], nullptr, m * dd, &o->Fs));
    TRY(stage_in<double>(ctx, ctx->lti[5], nullptr, m * dd, &o->Qs));
    TRY(stage_in<double>(ctx, ctx->lti[6], nullptr, m * dd, &o->fPs));
    TRY(stage_in<double>(ctx, ctx->lti[7], nullptr, m * d, &o->fms));
    o->sPs = o->sms = nullptr;
    if (smooth) {
        TRY(stage_in<double>(ctx, ctx->lti[8], nullptr, m * dd, &o->sPs));
        TRY(stage_in<double>(ctx, ctx->lti[9], nullptr, m * d, &o->sms));
    }
    TRY(stage_in<double>(ctx, ctx->st[11], nullptr, 2, &dll));
    const double *P0 = o->model + dd, *Hd = o->model + 2 * dd;
    TRY(disc_dev<double>(ctx, (long)m, d, o->model, P0, ts_m, t0, o->Fs, o->Qs));
    if (!smooth) return pkf_dev<double>(ctx, (long)m, d, P0, o->Fs, o->Qs, Hd, R, ys_m, o->fms, o->fPs, ll ? ll : dll);
    return pkfs_dev<double>(ctx, (long)m, d, P0, o->Fs, o->Qs, Hd, R, ys_m, o->fms, o->fPs, o->sms, o->sPs, ll ? ll : dll);
}

static int lti_dev(pgps_ctx* ctx, long N, long K, int d, const double* F, const double* Pinf, const double* H, double R,
                   const double* ts, const double* ys, double t0, const double* tq, double* mean, double* var,
                   double* ll, const LtiLin* lin = nullptr) {
    if (!ctx || N < 1 || K < 0 || !F || !Pinf || !H || !ts || !ys) return PGPS_E_INVALID;
    if (K > 0 && (!tq || !mean || (!var && !lin))) return PGPS_E_INVALID;
    if (K == 0 && !ll) return PGPS_E_INVALID;
    if (lin && (K < 1 || !lin->C || !lin->cov || lin->J < 1 || lin->J > PGPS_MAX_FUNCTIONALS)) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    if (N + K > 0x7fffffffL) return PGPS_E_INVALID;
    // (the functionals flavour of the row-cooperative smoother addresses mean and cov with 32-bit byte offsets)
    if (lin && d <= rc::kDimMax && (size_t)K * lin->J * lin->J * sizeof(double) > 0x7fff0000u) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t m = (size_t)(N + K);
    const double *ts_m = ts, *ys_m = ys;
    int* qslot = nullptr;
    if (K > 0) {
        Merged<double> mg;
        TRY(merged_front<double>(ctx, ctx->lti + 1, N, K, ts, ys, tq, &mg));
        ts_m = mg.ts; ys_m = mg.ys; qslot = mg.qslot;
    }
    return lti_core(ctx, m, d, F, Pinf, H, R, ts_m, ys_m, t0, qslot, mean, var, ll, lin);
}

// host arrays in and out, staged once for both flavours (lin: mean (K, J) and lin->cov (K, J, J) on the HOST in place of var)
static int lti_host(pgps_ctx* ctx, long N, long K, int d, const double* F, const double* Pinf, const double* H, double R,
                    const double* ts, const double* ys, double t0, const double* tq, double* mean, double* var,
                    double* ll, const LtiLin* lin = nullptr) {
    if (!ctx || N < 1 || K < 0 || !ts || !ys) return PGPS_E_INVALID;
    if (lin && (K < 1 || !lin->C || !lin->cov || lin->J < 1 || lin->J > PGPS_MAX_FUNCTIONALS)) return PGPS_E_INVALID;
    if (lin) var = lin->cov;
    if (K > 0 && (!tq || !mean || !var)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t J = lin ? (size_t)lin->J : 1, nm = (size_t)K * J, nv = lin ? nm * J : (size_t)K;
    // the device call of either flavour: var is the block's place when there are functionals
    auto run = [&](double* dts, double* dys, double* dtq, double* dmean, double* dvar, double* dll) {
        if (!lin) return lti_dev(ctx, N, K, d, F, Pinf, H, R, dts, dys, t0, dtq, dmean, dvar, dll);
        const LtiLin dl{lin->C, lin->J, dvar};
        return lti_dev(ctx, N, K, d, F, Pinf, H, R, dts, dys, t0, dtq, dmean, nullptr, dll, &dl);
    };
    {
        SmallStage st(ctx, 2 * SmallStage::up((size_t)N * 8) + SmallStage::up((size_t)K * 8),
                      SmallStage::up(nm * 8) + SmallStage::up(nv * 8) + 16);
        if (st.ok) {
            double llh = 0.0;
            double* dts_ = st.in(ts, (size_t)N);
            double* dys_ = st.in(ys, (size_t)N);
            double* dtq_ = K > 0 ? st.in(tq, (size_t)K) : nullptr;
            double* dll_ = st.out(&llh, 1);
            double* dmean_ = K > 0 ? st.out(mean, nm) : nullptr;
            double* dvar_ = K > 0 ? st.out(var, nv) : nullptr;
            TRY(st.send());
            TRY(run(dts_, dys_, dtq_, dmean_, dvar_, dll_));
            TRY(st.finish());
            if (ll) *ll = llh;
            return std::isfinite(llh) ? PGPS_OK : PGPS_E_NUMERIC;
        }
    }
    double *dts, *dys, *dtq = nullptr, *dmean = nullptr, *dvar = nullptr, *dll;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    if (K > 0) {
        TRY(stage_in(ctx, ctx->st[3], tq, (size_t)K, &dtq));
        TRY(stage_in<double>(ctx, ctx->st[7], nullptr, nm, &dmean));
        TRY(stage_in<double>(ctx, ctx->st[8], nullptr, nv, &dvar));
    }
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, 2, &dll));
    TRY(run(dts, dys, dtq, dmean, dvar, dll));
    if (K > 0) {
        TRY(stage_out(ctx, mean, dmean, nm));
        TRY(stage_out(ctx, var, dvar, nv));
    }
    double llh = 0.0;
    TRY(stage_out(ctx, &llh, dll, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ll) *ll = llh;
    if (!std::isfinite(llh)) return PGPS_E_NUMERIC;
    return PGPS_OK;
}

// B models over one series: table = B x [F | Pinf | H | R] from host memory
int pgps::lti_ll_batch_dev(pgps_ctx* ctx, int B, long N, int d, const double* models, const double* ts, const double* ys,
                            double t0, double* ll) {
    if (!ctx || B < 1 || N < 1 || !models || !ts || !ys || !ll) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > rc::kDimMax) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t dd = (size_t)d * d, ms = 2 * dd + d + 1;
    double *table, *Fs;
    TRY(stage_in<double>(ctx, ctx->lti[0], models, (size_t)B * ms, &table));
    TRY(stage_in<double>(ctx, ctx->lti[4], nullptr, (size_t)B * (size_t)N * dd, &Fs));
    TRY(launch_disc_rc(ctx, N, d, table, table + dd, ts, t0, Fs, nullptr, B, (long)ms));     // implicit process noise
    return launch_ll_batch_rc(ctx, N, d, B, table, (long)ms, Fs, nullptr, ys, ll);
}

static int lti_ll_batch_host(pgps_ctx* ctx, int B, long N, int d, const double* models, const double* ts, const double* ys,
                             double t0, double* ll) {
    if (!ctx || B < 1 || N < 1 || !models || !ts || !ys || !ll) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double *dts, *dys, *dll;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)B, &dll));
    TRY(lti_ll_batch_dev(ctx, B, N, d, models, dts, dys, t0, dll));
    TRY(stage_out(ctx, ll, dll, (size_t)B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGPS_OK;
}

extern "C" int pgps_lti_ll_batch_f64(pgps_ctx* c, int B, long N, int d, const double* models, const double* ts,
                                     const double* ys, double t0, double* ll) {
    return lti_ll_batch_host(c, B, N, d, models, ts, ys, t0, ll);
}
extern "C" int pgps_lti_ll_batch_dev_f64(pgps_ctx* c, int B, long N, int d, const double* models, const double* ts,
                                         const double* ys, double t0, double* ll) {
    return lti_ll_batch_dev(c, B, N, d, models, ts, ys, t0, ll);
}
// log-likelihood and the model's adjoints (pgps_gradlti.h): [ll | Abar | Ubar | Hbar | Rbar]
int pgps::lti_grad_dev(pgps_ctx* ctx, long N, int d, const double* F, const double* Pinf, const double* H, double R,
                        const double* ts, const double* ys, double t0, double* out) {
    if (!ctx || N < 1 || !F || !Pinf || !H || !ts || !ys || !out) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double* model;
    TRY(lti_model_in(ctx, d, F, Pinf, H, &model));
    // row-cooperative kernels up to d = 16; above that (and wherever the wave-cooperative family is forced: the tests'
    // cross-check) the wave-cooperative ones, from discretised arrays
    if (d <= rc::kDimMax && ctx->family != 2) return launch_ll_grad_lti(ctx, N, d, model, R, ts, t0, ys, out);
    double *Fs, *Qs;
    TRY(lti_disc_wc(ctx, (size_t)N, d, model, F, Pinf, ts, t0, &Fs, &Qs));
    return launch_ll_grad_lti_wc(ctx, N, d, model, R, Fs, Qs, ts, t0, ys, out);
}
extern "C" int pgps_lti_ll_grad_dev_f64(pgps_ctx* c, long N, int d, const double* F, const double* Pinf, const double* H,
                                        double R, const double* ts, const double* ys, double t0, double* out) {
    return lti_grad_dev(c, N, d, F, Pinf, H, R, ts, ys, t0, out);
}
extern "C" int pgps_lti_ll_grad_f64(pgps_ctx* ctx, long N, int d, const double* F, const double* Pinf, const double* H,
                                    double R, const double* ts, const double* ys, double t0, double* out) {
    if (!ctx || N < 1 || !ts || !ys || !out) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nout = 1 + (size_t)grad_lti_nstat(d);
    double *dts, *dys, *dout;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, nout, &dout));
    TRY(lti_grad_dev(ctx, N, d, F, Pinf, H, R, dts, dys, t0, dout));
    TRY(stage_out(ctx, out, dout, nout));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return std::isfinite(out[0]) ? PGPS_OK : PGPS_E_NUMERIC;
}
// ... of B models over one series on the row-cooperative kernels (2 <= d <= 16): models = B rows [F | Pinf | H | R] from host
// memory, out (B, 1 + d d + 2 d + 1) on the device
int pgps::lti_grad_batch_dev(pgps_ctx* ctx, int B, long N, int d, const double* models, const double* ts, const double* ys,
                              double t0, double* out) {
    if (!ctx || B < 1 || N < 1 || !models || !ts || !ys || !out) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > rc::kDimMax) return PGPS_E_UNSUPPORTED_DIM;
    const size_t dd = (size_t)d * d, ms = 2 * dd + d + 1;
    for (int b = 0; b < B; ++b)
        if (!(models[(size_t)b * ms + ms - 1] > 0.0)) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double* table;
    TRY(stage_in<double>(ctx, ctx->lti[0], models, (size_t)B * ms, &table));
    return launch_ll_grad_lti_batch(ctx, N, d, B, table, (long)ms, ts, t0, ys, out);
}
extern "C" int pgps_lti_ll_grad_batch_dev_f64(pgps_ctx* c, int B, long N, int d, const double* models, const double* ts,
                                              const double* ys, double t0, double* out) {
    return lti_grad_batch_dev(c, B, N, d, models, ts, ys, t0, out);
}
extern "C" int pgps_lti_ll_grad_batch_f64(pgps_ctx* ctx, int B, long N, int d, const double* models, const double* ts,
                                          const double* ys, double t0, double* out) {
    if (!ctx || B < 1 || N < 1 || !models || !ts || !ys || !out) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > rc::kDimMax) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int nout = 1 + grad_lti_nstat(d);
    double *dts, *dys, *dout;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)B * nout, &dout));
    TRY(lti_grad_batch_dev(ctx, B, N, d, models, dts, dys, t0, dout));
    TRY(stage_out(ctx, out, dout, (size_t)B * nout));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return adj_batch_result(B, nout, out);
}
extern "C" int pgps_lti_ll_f64(pgps_ctx* c, long N, int d, const double* F, const double* Pinf, const double* H, double R,
                               const double* ts, const double* ys, double t0, double* ll) {
    if (!ll) return PGPS_E_INVALID;
    return lti_host(c, N, 0, d, F, Pinf, H, R, ts, ys, t0, nullptr, nullptr, nullptr, ll);
}
extern "C" int pgps_lti_ll_dev_f64(pgps_ctx* c, long N, int d, const double* F, const double* Pinf, const double* H,
                                   double R, const double* ts, const double* ys, double t0, double* ll) {
    return lti_dev(c, N, 0, d, F, Pinf, H, R, ts, ys, t0, nullptr, nullptr, nullptr, ll);
}
extern "C" int pgps_lti_predict_f64(pgps_ctx* c, long N, long K, int d, const double* F, const double* Pinf,
                                    const double* H, double R, const double* ts, const double* ys, double t0,
                                    const double* tq, double* mean, double* var, double* ll) {
    if (K < 1) return PGPS_E_INVALID;
    return lti_host(c, N, K, d, F, Pinf, H, R, ts, ys, t0, tq, mean, var, ll);
}
extern "C" int pgps_lti_predict_dev_f64(pgps_ctx* c, long N, long K, int d, const double* F, const double* Pinf,
                                        const double* H, double R, const double* ts, const double* ys, double t0,
                                        const double* tq, double* mean, double* var, double* ll) {
    if (K < 1) return PGPS_E_INVALID;
    return lti_dev(c, N, K, d, F, Pinf, H, R, ts, ys, t0, tq, mean, var, ll);
}
extern "C" int pgps_lti_predict_lin_f64(pgps_ctx* c, long N, long K, int d, int J, const double* F, const double* Pinf,
                                        const double* H, const double* C, double R, const double* ts, const double* ys,
                                        double t0, const double* tq, double* mean, double* cov, double* ll) {
    if (K < 1) return PGPS_E_INVALID;
    const LtiLin lin{C, J, cov};
    return lti_host(c, N, K, d, F, Pinf, H, R, ts, ys, t0, tq, mean, nullptr, ll, &lin);
}
extern "C" int pgps_lti_predict_lin_dev_f64(pgps_ctx* c, long N, long K, int d, int J, const double* F, const double* Pinf,
                                            const double* H, const double* C, double R, const double* ts, const double* ys,
                                            double t0, const double* tq, double* mean, double* cov, double* ll) {
    if (K < 1) return PGPS_E_INVALID;
    const LtiLin lin{C, J, cov};
    return lti_dev(c, N, K, d, F, Pinf, H, R, ts, ys, t0, tq, mean, nullptr, ll, &lin);
}
// ---------------------------------------------------------------------------------------------
// batched predict_f for ANY kernel's LTI model (fp64, 2 <= d <= 16): B models [F | Pinf | H | R] over one series and one
// query grid.  ONE merge, one batched discretisation, then the row-cooperative filter + smoother + projection of all
// models of a group side by side (blockIdx.y = model: model_view, pgps_rc.hip.h) -- the launches of ONE predict, whatever B.
// ---------------------------------------------------------------------------------------------
int pgps::lti_predict_batch_merged(pgps_ctx* ctx, int B, size_t m, long K, int d, const double* models, const double* ts_m,
                                    const double* ys_m, double t0, const int* qslot, double* mean, double* var, double* ll) {
    const size_t dd = (size_t)d * d, ms = 2 * dd + d + 1;
    for (int b = 0; b < B; ++b)
        if (!(models[(size_t)b * ms + ms - 1] > 0.0)) return PGPS_E_INVALID;
    // per model: Fs, the stored smoothing elements E (as much again) and g, plus L and the chain records inside the scan's
    // own workspace -- about 3 m d^2 doubles; the models run in groups that fit the context's batch budget
    const size_t group = batch_group(batch_budget_lti(ctx), 0, (3 * m * dd + m * d) * sizeof(double), (size_t)B);
    double *table, *Fs, *Es, *gs;
    TRY(stage_in<double>(ctx, ctx->lti[0], models, (size_t)B * ms, &table));
    TRY(stage_in<double>(ctx, ctx->lti[4], nullptr, group * m * dd, &Fs));
    TRY(stage_in<double>(ctx, ctx->lti[6], nullptr, group * m * dd, &Es));
    TRY(stage_in<double>(ctx, ctx->lti[7], nullptr, group * m * d, &gs));
    for (size_t g0 = 0; g0 < (size_t)B; g0 += group) {
        const int G = (int)((size_t)B - g0 < group ? (size_t)B - g0 : group);
        const double* tab = table + g0 * ms;
        TRY(launch_disc_rc(ctx, (long)m, d, tab, tab + dd, ts_m, t0, Fs, nullptr, G, (long)ms));     // implicit process noise
        TRY(launch_predict_batch_rc(ctx, (long)m, K, d, G, B, tab, (long)ms, Fs, ys_m, qslot, Es, gs, mean + g0 * (size_t)K,
                                    var + g0 * (size_t)K, ll + g0));
    }
    return PGPS_OK;
}

static int lti_predict_batch_dev(pgps_ctx* ctx, int B, long N, long K, int d, const double* models, const double* ts,
                                 const double* ys, double t0, const double* tq, double* mean, double* var, double* ll) {
    if (!ctx || B < 1 || N < 1 || K < 1 || !models || !ts || !ys || !tq || !mean || !var) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > rc::kDimMax) return PGPS_E_UNSUPPORTED_DIM;
    if (N + K > 0x7fffffffL) return PGPS_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t m = (size_t)(N + K);
    Merged<double> mg;
    double* dll = ll;
    TRY(merged_front<double>(ctx, ctx->lti + 1, N, K, ts, ys, tq, &mg));
    if (!dll) TRY(stage_in<double>(ctx, ctx->st[6], nullptr, (size_t)B, &dll));
    return lti_predict_batch_merged(ctx, B, m, K, d, models, mg.ts, mg.ys, t0, mg.qslot, mean, var, dll);
}

extern "C" int pgps_lti_predict_batch_dev_f64(pgps_ctx* c, int B, long N, long K, int d, const double* models, const double* ts,
                                              const double* ys, double t0, const double* tq, double* mean, double* var,
                                              double* ll) {
    return lti_predict_batch_dev(c, B, N, K, d, models, ts, ys, t0, tq, mean, var, ll);
}

extern "C" int pgps_lti_predict_batch_f64(pgps_ctx* ctx, int B, long N, long K, int d, const double* models, const double* ts,
                                          const double* ys, double t0, const double* tq, double* mean, double* var, double* ll) {
    if (!ctx || B < 1 || N < 1 || K < 1 || !models || !ts || !ys || !tq || !mean || !var) return PGPS_E_INVALID;
    if (d < rc::kDimMin || d > rc::kDimMax) return PGPS_E_UNSUPPORTED_DIM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t bk = (size_t)B * (size_t)K;
    double *dts, *dys, *dtq, *dmean, *dvar, *dll;
    TRY(stage_in(ctx, ctx->st[10], ts, (size_t)N, &dts));
    TRY(stage_in(ctx, ctx->st[4], ys, (size_t)N, &dys));
    TRY(stage_in(ctx, ctx->st[3], tq, (size_t)K, &dtq));
    TRY(stage_in<double>(ctx, ctx->st[7], nullptr, bk, &dmean));
    TRY(stage_in<double>(ctx, ctx->st[8], nullptr, bk, &dvar));
    TRY(stage_in<double>(ctx, ctx->st[9], nullptr, (size_t)B, &dll));
    TRY(lti_predict_batch_dev(ctx, B, N, K, d, models, dts, dys, t0, dtq, dmean, dvar, dll));
    return copy_out_batch(ctx, B, {mean, dmean, bk * 8}, {var, dvar, bk * 8}, dll, ll);
}
