// pgps_host.h -- what the host units of the C ABI share (pgps_ctx.hip, pgps_scan_api.hip, pgps_gp_api.hip, pgps_series.hip,
// pgps_lti_api.hip, pgps_post_api.hip): staging of host arrays, dimension dispatch, the float32 promotion path, the merged
// front of the model-level calls and the functions that cross those units.  No kernel unit includes it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "pgps_internal.h"

#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

namespace pgps {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// f(std::integral_constant<int, D>{}) for the D in [Lo, Hi] that equals d: the ONE ladder over the compiled state dimensions
//   return for_dim<1, 6>(d, [&](auto D) { return launch_scan<T, D()>(ctx, a, mode); });
template <int Lo, int Hi, typename F>
int for_dim(int d, F&& f) {
    if constexpr (Lo > Hi) {
        return PGPS_E_UNSUPPORTED_DIM;
    } else {
        if (d == Lo) return f(std::integral_constant<int, Lo>{});
        return for_dim<Lo + 1, Hi>(d, std::forward<F>(f));
    }
}

// ---------------------------------------------------------------------------------------------
// host-pointer entry points (stage -> run -> copy back)
// ---------------------------------------------------------------------------------------------
template <typename T>
int stage_in(pgps_ctx* ctx, DevBuf& b, const T* host, size_t n, T** dev) {
    int rc = ensure(ctx, b, n * sizeof(T));
    if (rc) return rc;
    *dev = (T*)b.p;
    if (host) HIPCHK(ctx, hipMemcpyAsync(b.p, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return PGPS_OK;
}
template <typename T>
int stage_out(pgps_ctx* ctx, T* host, const T* dev, size_t n) {
    if (host) HIPCHK(ctx, hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return PGPS_OK;
}

// A call whose host arrays are small -- the first evaluation of a model at the reference's series lengths, the whole of its
// speed protocol (experiments/toy_models/speed_and_stability.py:73-87) -- pays for every hipMemcpy from pageable memory (a
// staged, host-synchronous copy of ~10 us whatever its size).  SmallStage lays the call's inputs out in one pinned arena
// (plain memcpy), sends them with ONE asynchronous copy, and brings the outputs back with ONE: three inputs and three
// outputs of pgps_gp_predict_f64 at N = K = 4096 were six such copies (model + predict_f 178 -> 140 us).
constexpr size_t kPinArena = 2u << 20;
struct SmallStage {
    pgps_ctx* ctx;
    size_t in_bytes = 0, out_bytes = 0, in_cap, out_off;
    bool ok = false;
    bool in_flight = false;         // send() has queued a copy out of the pinned arena and finish() has not synchronised yet
    struct Out { void* host; size_t off, bytes; } outs[4];
    int nout = 0;
    // in_total / out_total: bytes of all inputs / outputs (each rounded up to 16)
    SmallStage(pgps_ctx* c, size_t in_total, size_t out_total) : ctx(c), in_cap(in_total), out_off(in_total) {
        if (in_total + out_total > kPinArena) return;
        if (!ctx->pin_h && hipHostMalloc((void**)&ctx->pin_h, kPinArena, hipHostMallocDefault) != hipSuccess) { ctx->pin_h = nullptr; return; }
        if (ensure(ctx, ctx->pin_d, kPinArena) != PGPS_OK) return;
        ok = true;
    }
    // an error return between send() and finish() (TRY leaves the function) must not leave the arena's host-to-device copy
    // in flight: the next small call would memcpy its inputs into the same pinned bytes underneath it
    ~SmallStage() {
        if (in_flight) (void)hipStreamSynchronize(ctx->stream);
    }
    SmallStage(const SmallStage&) = delete;
    SmallStage& operator=(const SmallStage&) = delete;
    static size_t up(size_t b) { return (b + 15) / 16 * 16; }
    template <typename T> T* in(const T* host, size_t n) {          // -> device pointer of the staged copy
        T* dev = (T*)((char*)ctx->pin_d.p + in_bytes);
        memcpy(ctx->pin_h + in_bytes, host, n * sizeof(T));
        in_bytes += up(n * sizeof(T));
        return dev;
    }
    template <typename T> T* out(T* host, size_t n) {               // -> device pointer the call writes, copied back by finish()
        T* dev = (T*)((char*)ctx->pin_d.p + out_off + out_bytes);
        outs[nout++] = {(void*)host, out_off + out_bytes, n * sizeof(T)};
        out_bytes += up(n * sizeof(T));
        return dev;
    }
    int send() {
        in_flight = true;
        HIPCHK(ctx, hipMemcpyAsync(ctx->pin_d.p, ctx->pin_h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
        return PGPS_OK;
    }
    int finish() {                                                  // one copy back, the synchronisation, the scatter
        HIPCHK(ctx, hipMemcpyAsync(ctx->pin_h + out_off, (char*)ctx->pin_d.p + out_off, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        in_flight = false;
        for (int i = 0; i < nout; ++i)
            if (outs[i].host) memcpy(outs[i].host, ctx->pin_h + outs[i].off, outs[i].bytes);
        return PGPS_OK;
    }
};

// device results -> pageable host arrays through the context's pinned buffer; synchronises the stream (pgps_ctx.hip)
struct OutPart { void* host; const void* dev; size_t bytes; };
int copy_out(pgps_ctx* ctx, const OutPart* parts, int n);
// the tail of a batched host call: mean, var and the B log-likelihoods [device] come back in one copy_out; ll (may be null)
// takes the log-likelihoods.  PGPS_E_NUMERIC unless all B are finite.
int copy_out_batch(pgps_ctx* ctx, int B, OutPart mean, OutPart var, const double* dll, double* ll);
// ... its last step alone, for log-likelihoods already on the host
int batch_ll_result(int B, const double* llh, double* ll);

// which of the two builds of the lane-chunk scan a call (or a rank's segment) of N steps at state dimension d takes
bool lane_narrow(const pgps_ctx* ctx, int d, long N);

// ---------------------------------------------------------------------------------------------
// float32 calls in fp64 arithmetic (pgps_scan_api.hip)
// ---------------------------------------------------------------------------------------------
// The plain probe sequence of a float32 call that reads smoothing gains off the grid Fs (N, d, d): *wide = 1 when the call
// is to run in fp64 arithmetic (policy 2, d > 16, or the probe found the grid dense), 0 for the float32 kernels.  Waits for
// the probe's verdict; the context's memory of the last probed call moves only when the probe decided.
int f32_wants_promotion(pgps_ctx* ctx, long N, int d, const float* Fs, int* wide);

// up to eight arrays in one launch (blockIdx.y selects the array): the promoted float32 calls convert seven inputs and four
// outputs, and a launch costs the host more than converting a short series does
struct ConvJobs {
    const void* src[8];
    void* dst[8];
    long n[8];
};
// The conversions of one promoted call.  add() collects arrays (a null or empty one is skipped), widen() / narrow() convert
// what was collected in ONE launch sized for the longest of them and start a new collection; finish() checks the launches
// and raises PGPS_STATUS_F32_PROMOTED.
class WideConv {
public:
    explicit WideConv(pgps_ctx* c) : ctx_(c) {}
    void add(const void* src, void* dst, size_t n);
    void widen();                                               // float -> double
    void narrow();                                              // double -> float
    void narrow_one(const double* src, float* dst, size_t n);   // a single array
    int finish(bool promoted = true);                           // (false: the discretisation, fp64 arithmetic in every family by design)
private:
    dim3 grid(size_t longest, int arrays) const { return dim3((unsigned)std::min<size_t>(4096, (longest + 255) / 256), (unsigned)arrays); }
    pgps_ctx* ctx_;
    ConvJobs jobs_{};
    int nj_ = 0;
    size_t most_ = 0;
};

// device-pointer entry points of the array path; pgps_scan_api.hip instantiates them for double and float
template <typename T>
int pkf_dev(pgps_ctx* ctx, long N, int d, const T* P0, const T* Fs, const T* Qs, const T* H, T R, const T* ys, T* fms, T* fPs,
            double* ll);
template <typename T>
int pkfs_dev(pgps_ctx* ctx, long N, int d, const T* P0, const T* Fs, const T* Qs, const T* H, T R, const T* ys, T* fms, T* fPs,
             T* sms, T* sPs, double* ll);
template <typename T>
int disc_dev(pgps_ctx* ctx, long N, int d, const T* F, const T* Pinf, const T* ts, T t0, T* Fs, T* Qs);

// ---------------------------------------------------------------------------------------------
// the merged series of the model-level calls
// ---------------------------------------------------------------------------------------------
template <typename T>
struct Merged {
    T* ts;          // (N + K,) merged times
    T* ys;          // (N + K,) observations, NaN at the query rows
    int* qslot;     // (N + K,) slot of a query row, -1 at the training rows
};
// training series and query grid merged on the device (launch_merge) into three consecutive buffers of the context:
// b = ctx->lti + 1 or ctx->st
template <typename T>
int merged_front(pgps_ctx* ctx, DevBuf* b, long N, long K, const T* ts, const T* ys, const T* tq, Merged<T>* m) {
    const size_t n = (size_t)(N + K);
    TRY(stage_in<T>(ctx, b[0], nullptr, n, &m->ts));
    TRY(stage_in<T>(ctx, b[1], nullptr, n, &m->ys));
    TRY(stage_in<int>(ctx, b[2], nullptr, n, &m->qslot));
    return launch_merge<T>(ctx, N, K, ts, ys, tq, m->ts, m->ys, m->qslot);
}

// general LTI models (pgps_lti_api.hip)
// the small model [F | Pinf | H] from host memory into ctx->lti[0], in one copy
// (with C: the J rows of the functionals follow, [F | Pinf | H | C], the same copy)
int lti_model_in(pgps_ctx* ctx, int d, const double* F, const double* Pinf, const double* H, double** model,
                 const double* C = nullptr, int J = 0);
// the functionals of a pgps_lti_predict_lin_* call: C (J, d) HOST; lti_core then writes mean (K, J) and cov (K, J, J) [device]
struct LtiLin {
    const double* C;
    int J;
    double* cov;
};
// The array-path front of a model-level call over m (merged) steps: model in, Fs / Qs / fPs / fms (with `smooth`: sPs / sms
// too) in ctx->lti[4..9], discretisation, then the filter (or filter + smoother).  ll [device] may be null.
struct LtiFront {
    double* model;              // [F | Pinf | H]
    double *Fs, *Qs, *fms, *fPs, *sms, *sPs;
};
int lti_filter_front(pgps_ctx* ctx, size_t m, int d, const double* F, const double* Pinf, const double* H, double R,
                     const double* ts_m, const double* ys_m, double t0, bool smooth, double* ll, LtiFront* o);
int lti_core(pgps_ctx* ctx, size_t m, int d, const double* F, const double* Pinf, const double* H, double R, const double* ts_m,
             const double* ys_m, double t0, const int* qslot, double* mean, double* var, double* ll, const LtiLin* lin = nullptr);
int lti_ll_batch_dev(pgps_ctx* ctx, int B, long N, int d, const double* models, const double* ts, const double* ys, double t0,
                     double* ll);
int lti_grad_dev(pgps_ctx* ctx, long N, int d, const double* F, const double* Pinf, const double* H, double R, const double* ts,
                 const double* ys, double t0, double* out);
int lti_grad_batch_dev(pgps_ctx* ctx, int B, long N, int d, const double* models, const double* ts, const double* ys, double t0,
                       double* out);
int lti_predict_batch_merged(pgps_ctx* ctx, int B, size_t m, long K, int d, const double* models, const double* ts_m,
                             const double* ys_m, double t0, const int* qslot, double* mean, double* var, double* ll);

// fused Matern path (pgps_gp_api.hip); instantiated for double and float
template <typename T>
int gp_dev(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf, const double* H,
           double R, const T* ts, double t0, const T* ys, T* fms, T* fPs, T* sms, T* sPs, double* ll);
int gp_adj_dev(pgps_ctx* ctx, long N, int d, double lam, const double* N1, const double* N2, const double* Pinf, const double* H,
               double R, const double* ts, double t0, const double* ys, double* out);
// ... of B models (host table of rows [lam | N1 | N2 | Pinf | H | R]) over one series: out (B, 1 + d d + 2 d + 1) [device]
int gp_adj_batch_dev(pgps_ctx* ctx, int B, long N, int d, const double* models_host, const double* ts, double t0, const double* ys,
                     double* out);
// B result rows of nout doubles on the host: PGPS_E_NUMERIC when a row's log-likelihood (its first entry) is not finite
int adj_batch_result(int B, int nout, const double* rows);
template <typename T>
int gp_predict_batch_merged(pgps_ctx* ctx, int B, size_t m, long K, int d, const double* models_host, const T* ts_m,
                            const T* ys_m, double t0, const int* qslot, T* mean, T* var, double* ll);

// a panel of series (pgps_panel_api.hip), shared with pgps_panel_gram_api.hip
// everything a panel call can be refused for before anything is staged (ys: the array whose presence is required)
int panel_check(pgps_ctx* ctx, long S, const long* offs, const long* qoffs, bool predict, int d, int nmodels, const double* models,
                const double* ts, const double* ys, bool het);
// the caller's rows [lam | N1 | N2 | Pinf | H | R] re-packed to the fixed device stride (kGpModelStride)
void panel_pack_models(int nmodels, int d, const double* models, std::vector<double>& packed);
// the Gram calls' checks (pgps_panel_gram_api.hip), shared with pgps_panel_trend_api.hip: panel_check on V, C in 1 .. kPanelGramMax
// and a non-null out; and the host forms' one pass over V (a row is NaN in all columns or in none) and rs (the rule of
// pgps_gp_panel_ll_f64 at the observed rows)
int panel_gram_check(pgps_ctx* ctx, long S, const long* offs, int d, int nmodels, const double* models, int C, const double* ts,
                     const double* V, bool het, const double* out);
bool panel_gram_rows_valid(long S, const long* offs, int d, int nmodels, const double* models, int C, const double* V,
                           const double* rs);

// moments of the mixture of B Gaussians per query column (pgps_post_api.hip)
int mix_moments_dev(pgps_ctx* ctx, int B, long K, const double* mean, const double* var, const double* w, double* mean_out,
                    double* var_out);

}  // namespace pgps
