"""Any kernel's LTI model (F, Pinf, H), fp64, 2 <= d <= 32: likelihood, adjoint gradient, predict, draws, and the streams
that enqueue one asynchronous evaluation per model."""
import numpy as np

from .arrays import _prep, _ptr, _scalar_out, _series_inputs
from .context import Context, get_context
from .library import _require, c_double, c_int, c_long, c_void_p

# state dimensions of the general-LTI device path: row-cooperative kernels up to 16 (batched evaluation only there),
# wave-cooperative kernels from 17 to 32
LTI_DIM_MIN, LTI_DIM_MAX, LTI_BATCH_DIM_MAX = 2, 32, 16
LTI_FUNCTIONALS_MAX = 8         # PGPS_MAX_FUNCTIONALS: rows of C in one pgps_lti_predict_lin_* call


def _lti_model(F, Pinf, H):
    F = _prep(F, np.float64)
    d = F.shape[0]
    if not (LTI_DIM_MIN <= d <= LTI_DIM_MAX):
        raise ValueError(f"the general-LTI device path covers state dimensions {LTI_DIM_MIN}..{LTI_DIM_MAX}, got {d}")
    return F, _prep(Pinf, np.float64, (d, d)), _prep(H, np.float64, (d,)), d


def lti_ll(F, Pinf, H, R, ts, ys, t0=0.0, device=0):
    """Log-likelihood of any LTI state-space GP on the device (pgps_lti_ll_f64): discretisation, parallel filter
    and the likelihood terms with nothing written per step.  `Pinf` must be the stationary covariance of the SDE
    (it is every kernel's P0)."""
    F, Pinf, H, d = _lti_model(F, Pinf, H)
    ts_a, ys_a, N = _series_inputs(ts, ys)
    ll, llp = _scalar_out()
    get_context(device).call("pgps_lti_ll_f64", N, d, _ptr(F), _ptr(Pinf), _ptr(H), float(R), _ptr(ts_a), _ptr(ys_a),
                             float(t0), llp)
    return ll.value


def split_grad_stats(out, d, M=None):
    """[ll | Abar | Ubar | Hbar | Rbar] of pgps_lti_ll_grad_* -> (ll, Abar (d, d), Ubar (d,), Hbar (d,), Rbar); given M, the
    statistics follow M log-likelihoods (pgps_gp_ll_grad_multi_*) and ll comes back as an (M,) array.  Copies."""
    dd = d * d
    ll, st = (float(out[0]), out[1:]) if M is None else (out[:M].copy(), out[M:])
    return ll, st[:dd].reshape(d, d).copy(), st[dd:dd + d].copy(), st[dd + d:dd + 2 * d].copy(), float(st[dd + 2 * d])


def contract_grad_stats(stats, H, grads):
    """d ll / d theta for the kernel's parameters (grads: [(dF, dPinf, dH)] of pssgp.kernels.sde_grads, every dF
    commuting with F) followed by d ll / d R -- the host half of the adjoint gradient (include/pgps.h,
    pgps_lti_ll_grad_f64)."""
    _, Abar, Ubar, Hbar, Rbar = stats
    h = np.asarray(H, np.float64).reshape(-1)
    g = [float(np.sum(Abar * dF) + Ubar @ (np.asarray(dP, np.float64) @ h) + Hbar @ np.asarray(dH, np.float64).reshape(-1))
         for dF, dP, dH in grads]
    return np.array(g + [Rbar], np.float64)


def lti_ll_grad(F, Pinf, H, R, ts, ys, t0=0.0, device=0):
    """Log-likelihood and the model's adjoints of any LTI state-space GP (pgps_lti_ll_grad_f64): one filter pass and one
    reverse pass on the device, whatever the number of hyper-parameters.  Returns (ll, Abar, Ubar, Hbar, Rbar)."""
    F, Pinf, H, d = _lti_model(F, Pinf, H)
    ts_a, ys_a, N = _series_inputs(ts, ys)
    ctx = _require(get_context(device), "pgps_lti_ll_grad_f64", "pgps_lti_ll_grad_*")
    out = np.zeros(2 + d * d + 2 * d, np.float64)
    ctx.call("pgps_lti_ll_grad_f64", N, d, _ptr(F), _ptr(Pinf), _ptr(H), float(R), _ptr(ts_a), _ptr(ys_a), float(t0), _ptr(out))
    return split_grad_stats(out, d)


def lti_predict(F, Pinf, H, R, ts, ys, tq, t0=0.0, device=0):
    """predict_f of any LTI state-space GP on the device (pgps_lti_predict_f64): merge of the sorted `ts` (N) and
    `tq` (K), discretisation, filter + smoother over the N + K steps, posterior mean / variance of f = H x at the K
    query times.  Returns (mean (K,), var (K,), ll of the training series)."""
    F, Pinf, H, d = _lti_model(F, Pinf, H)
    ts_a, ys_a, tq_a, N = _series_inputs(ts, ys, tq)
    K = tq_a.shape[0]
    mean, var = np.empty(K, np.float64), np.empty(K, np.float64)
    ll, llp = _scalar_out()
    get_context(device).call("pgps_lti_predict_f64", N, K, d, _ptr(F), _ptr(Pinf), _ptr(H), float(R), _ptr(ts_a), _ptr(ys_a),
                             float(t0), _ptr(tq_a), _ptr(mean), _ptr(var), llp)
    return mean, var, ll.value


def lti_predict_lin(F, Pinf, H, C, R, ts, ys, tq, t0=0.0, device=0):
    """The posterior of J linear functionals C x of the state at the query times (pgps_lti_predict_lin_f64): the chain of
    lti_predict -- merge, discretisation, filter + smoother over the N + K steps, H the observation row -- with
    mean (K, J) = C sm and cov (K, J, J) = C sP C^T of every query step, each block symmetric bit for bit.  C (J, d),
    1 <= J <= LTI_FUNCTIONALS_MAX.  Returns (mean, cov, ll of the training series)."""
    F, Pinf, H, d = _lti_model(F, Pinf, H)
    C = _prep(C, np.float64, (-1, d))
    J = C.shape[0]
    ts_a, ys_a, tq_a, N = _series_inputs(ts, ys, tq)
    K = tq_a.shape[0]
    mean, cov = np.empty((K, J), np.float64), np.empty((K, J, J), np.float64)
    ll, llp = _scalar_out()
    ctx = _require(get_context(device), "pgps_lti_predict_lin_f64", "pgps_lti_predict_lin_*")
    ctx.call("pgps_lti_predict_lin_f64", N, K, d, J, _ptr(F), _ptr(Pinf), _ptr(H), _ptr(C), float(R), _ptr(ts_a), _ptr(ys_a),
             float(t0), _ptr(tq_a), _ptr(mean), _ptr(cov), llp)
    return mean, cov, ll.value


def _small_lti_model(F, Pinf, H):
    """(F, Pinf, H, d) of the calls that run on the lane-chunk kernels (d <= 6: the library refuses a larger one)."""
    F = _prep(F, np.float64)
    d = F.shape[0]
    return F, _prep(Pinf, np.float64, (d, d)), _prep(H, np.float64, (d,)), d


def lti_sample(F, Pinf, H, R, ts, ys, tq, num_samples, seed, t0=0.0, first_sample=0, device=0):
    """Joint posterior draws of f = H x at the sorted query times `tq` (K) of any LTI state-space GP with d <= 6
    (pgps_lti_sample_f64): merge with the sorted training times `ts`, discretisation, filter with the query rows
    missing, backward sampling -- the (S, K) projected draws come back, nothing per step.  Larger d raises
    PgpsError (PGPS_E_UNSUPPORTED_DIM)."""
    F, Pinf, H, d = _small_lti_model(F, Pinf, H)
    ts_a, ys_a, tq_a, N = _series_inputs(ts, ys, tq)
    K, S = tq_a.shape[0], int(num_samples)
    out = np.empty((S, K), np.float64)
    get_context(device).call("pgps_lti_sample_f64", N, K, d, _ptr(F), _ptr(Pinf), _ptr(H), float(R), _ptr(ts_a), _ptr(ys_a),
                             float(t0), _ptr(tq_a), S, int(first_sample), int(seed) & (2 ** 64 - 1), _ptr(out), None)
    return out


def lti_predict_cov(F, Pinf, H, R, ts, ys, tq, t0=0.0, device=0):
    """predict_f(full_cov=True) of any LTI state-space GP with d <= 6 on the device (pgps_lti_predict_cov_f64): merge of
    the sorted `ts` (N) and `tq` (K), discretisation, filter + smoother over the N + K steps, gain products between the
    query rows, fill.  Returns (mean (K,), cov (K, K) symmetric bit for bit, ll of the training series).  Larger d raises
    PgpsError (PGPS_E_UNSUPPORTED_DIM)."""
    F, Pinf, H, d = _small_lti_model(F, Pinf, H)
    ts_a, ys_a, tq_a, N = _series_inputs(ts, ys, tq)
    K = tq_a.shape[0]
    mean, cov = np.empty(K, np.float64), np.empty((K, K), np.float64)
    ll, llp = _scalar_out()
    get_context(device).call("pgps_lti_predict_cov_f64", N, K, d, _ptr(F), _ptr(Pinf), _ptr(H), float(R), _ptr(ts_a), _ptr(ys_a),
                             float(t0), _ptr(tq_a), _ptr(mean), _ptr(cov), llp)
    return mean, cov, ll.value


class LtiLlStream:
    """Log-likelihoods of several general LTI models over one series, one ASYNCHRONOUS device evaluation each
    (pgps_lti_ll_dev_f64): the series is uploaded once, the results are read once at the end, and the host prepares
    model i + 1 (its get_sde()) while the device runs model i.  For the state dimensions above the batch kernels'
    (17..32, e.g. the reference's CO2 kernel, d = 18)."""

    def __init__(self, ts, ys, capacity, t0=0.0, device=0):
        ts_a, ys_a, self.n = _series_inputs(ts, ys)
        self.t0, self.capacity, self.count = float(t0), int(capacity), 0
        self.d_ts = self.d_ys = self.d_ll = None
        # A context of its own: the asynchronous evaluations keep their scratch in the context between push() and
        # finish(), so the stream must own one -- and with a private context it never holds the shared default
        # context's lock (a stream dropped without finish() / close() used to leave that lock held for ever).
        self.ctx = Context(device)
        try:
            self.d_ts = self.ctx.malloc(ts_a.nbytes)
            self.d_ys = self.ctx.malloc(ys_a.nbytes)
            self.d_ll = self.ctx.malloc(8 * max(self.capacity, 1))
            self.ctx.h2d(self.d_ts, ts_a)
            self.ctx.h2d(self.d_ys, ys_a)
        except Exception:
            self.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass

    def push(self, F, Pinf, H, R):
        if self.count >= self.capacity:
            raise ValueError("LtiLlStream is full")
        F, Pinf, H, d = _lti_model(F, Pinf, H)
        self.ctx.call("pgps_lti_ll_dev_f64", c_long(self.n), c_int(d), _ptr(F), _ptr(Pinf), _ptr(H), c_double(float(R)),
                      c_void_p(self.d_ts), c_void_p(self.d_ys), c_double(self.t0), c_void_p(self.d_ll + 8 * self.count))
        self.count += 1

    def finish(self):
        """The log-likelihoods pushed so far (waits for the device); releases the device buffers."""
        out = np.empty(self.count, np.float64)
        try:
            if self.count:
                self.ctx.d2h(out, self.d_ll)
        finally:
            self.close()
        return out

    def close(self):
        ctx = getattr(self, "ctx", None)
        if ctx is None:
            return
        self.ctx = None
        try:
            for name in ("d_ts", "d_ys", "d_ll"):
                p = getattr(self, name, None)
                setattr(self, name, None)
                if p:
                    ctx.free(p)
        finally:
            ctx.close()


class LtiGradStream(LtiLlStream):
    """The same for the adjoint gradient (pgps_lti_ll_grad_dev_f64): one asynchronous evaluation per model of state dimension
    d, rows [ll | Abar | Ubar | Hbar | Rbar] read once at the end -- the road of d = 17..32, which no batched kernel covers.
    (Every evaluation's model is uploaded by a copy on the context's stream, so it is ordered behind the kernels of the
    evaluation before it.)"""

    def __init__(self, ts, ys, capacity, d, t0=0.0, device=0):
        self.d, self.nout = int(d), 2 + int(d) * int(d) + 2 * int(d)
        super().__init__(ts, ys, int(capacity) * self.nout, t0=t0, device=device)
        self.rows = int(capacity)

    def push(self, F, Pinf, H, R):
        if self.count >= self.rows:
            raise ValueError("LtiGradStream is full")
        F, Pinf, H, d = _lti_model(F, Pinf, H)
        if d != self.d:
            raise ValueError("all models of a batch must have the same state dimension")
        self.ctx.call("pgps_lti_ll_grad_dev_f64", c_long(self.n), c_int(d), _ptr(F), _ptr(Pinf), _ptr(H), c_double(float(R)),
                      c_void_p(self.d_ts), c_void_p(self.d_ys), c_double(self.t0), c_void_p(self.d_ll + 8 * self.nout * self.count))
        self.count += 1

    def finish(self):
        """The (count, 1 + d d + 2 d + 1) rows pushed so far (waits for the device); releases the device buffers."""
        out = np.empty((self.count, self.nout), np.float64)
        try:
            if self.count:
                self.ctx.d2h(out, self.d_ll)
        finally:
            self.close()
        return out


def lti_predict_stream(models, ts, ys, tq, t0=0.0, device=0):
    """predict_f of several general LTI models of ANY supported dimension (2 .. 32; the way for 17 .. 32, e.g. the
    reference's CO2 kernel), one ASYNCHRONOUS device predict each (pgps_lti_predict_dev_f64), enqueued as LtiLlStream
    enqueues likelihoods: series and query grid uploaded once, results read once.  (mean (B, K), var (B, K), ll (B,))."""
    ts_a = _prep(ts, np.float64, (-1,))
    ys_a = _prep(ys, np.float64, (-1,))
    tq_a = _prep(tq, np.float64, (-1,))
    N, K, B = ts_a.shape[0], tq_a.shape[0], len(models)
    mean, var, ll = np.empty((B, K), np.float64), np.empty((B, K), np.float64), np.empty(B, np.float64)
    ctx = Context(device)               # (a context of its own, as LtiLlStream: the evaluations keep scratch between calls)
    bufs = []
    try:
        for nbytes in (8 * N, 8 * N, 8 * K, 8 * B * K, 8 * B * K, 8 * B):
            bufs.append(ctx.malloc(nbytes))
        ctx.h2d(bufs[0], ts_a)
        ctx.h2d(bufs[1], ys_a)
        ctx.h2d(bufs[2], tq_a)
        for b, (F, Pinf, H, R) in enumerate(models):
            F, Pinf, H, d = _lti_model(F, Pinf, H)
            ctx.call("pgps_lti_predict_dev_f64", c_long(N), c_long(K), c_int(d), _ptr(F), _ptr(Pinf), _ptr(H), c_double(float(R)),
                     c_void_p(bufs[0]), c_void_p(bufs[1]), c_double(float(t0)), c_void_p(bufs[2]),
                     c_void_p(bufs[3] + 8 * K * b), c_void_p(bufs[4] + 8 * K * b), c_void_p(bufs[5] + 8 * b))
        ctx.d2h(mean, bufs[3])
        ctx.d2h(var, bufs[4])
        ctx.d2h(ll, bufs[5])
    finally:
        try:
            for p in bufs:
                ctx.free(p)
        finally:
            ctx.close()
    return mean, var, ll
