"""B models over one series in one set of launches: the model tables, the batched calls, the mixture moments."""
import numpy as np

from .arrays import _prep, _ptr, _series_inputs, _suffix
from .context import get_context
from .library import E_NUMERIC, PgpsError, _require, c_double, c_int, c_long, c_void_p
from .lti import LTI_BATCH_DIM_MAX, LTI_DIM_MAX, LTI_DIM_MIN, LtiGradStream, _lti_model


def _lti_table(models):
    """(B x [F | Pinf | H | R] float64 table, d) of a list of (F, Pinf, H, R), all of one state dimension."""
    if isinstance(models, np.ndarray):          # already a table: 2 d^2 + d + 1 columns
        cols = models.shape[1] if models.ndim == 2 else -1
        d = next((k for k in range(LTI_DIM_MIN, LTI_BATCH_DIM_MAX + 1) if 2 * k * k + k + 1 == cols), None)
        if d is None:
            raise ValueError(f"a general-LTI model table has 2 d^2 + d + 1 columns (d = {LTI_DIM_MIN}..{LTI_BATCH_DIM_MAX}), got shape {models.shape}")
        return np.ascontiguousarray(models, dtype=np.float64), d
    d, table = None, None
    for b, (F, Pinf, H, R) in enumerate(models):
        F, Pinf, H, dm = _lti_model(F, Pinf, H)
        if dm > LTI_BATCH_DIM_MAX:
            raise ValueError(f"batched general-LTI evaluation covers state dimensions up to {LTI_BATCH_DIM_MAX}, got {dm}")
        if d is None:
            d = dm
            table = np.empty((len(models), 2 * d * d + d + 1), np.float64)
        if dm != d:
            raise ValueError("all models of a batch must have the same state dimension")
        row = table[b]
        row[:d * d] = F.reshape(-1)
        row[d * d:2 * d * d] = Pinf.reshape(-1)
        row[2 * d * d:2 * d * d + d] = H.reshape(-1)
        row[-1] = R
    return table, d


def _gp_rows(models):
    """(B x [lam | N1 | N2 | Pinf | H | R] float64 table, d) of a list of (form=(lam, N1, N2), Pinf, H, R), one state dimension."""
    if isinstance(models, np.ndarray):          # already a table (StateSpaceGP._matern_table): 6, 16, 32 columns at d = 1, 2, 3
        d = {6: 1, 16: 2, 32: 3}.get(models.shape[1] if models.ndim == 2 else -1)
        if d is None:
            raise ValueError(f"a model table has 6, 16 or 32 columns (d = 1, 2, 3), got shape {models.shape}")
        return np.ascontiguousarray(models, dtype=np.float64), d
    d = np.asarray(models[0][0][1]).shape[0]
    rows = []
    for (lam, N1, N2), Pinf, H, R in models:
        if np.asarray(N1).shape[0] != d:
            raise ValueError("all models of a batch must have the same state dimension")
        rows.append(np.concatenate([[float(lam)], np.asarray(N1, np.float64).reshape(-1), np.asarray(N2, np.float64).reshape(-1),
                                    np.asarray(Pinf, np.float64).reshape(-1), np.asarray(H, np.float64).reshape(-1),
                                    [float(R)]]))
    return np.ascontiguousarray(np.stack(rows), dtype=np.float64), d


def lti_ll_batch(models, ts, ys, t0=0.0, device=0):
    """Log-likelihoods of B general LTI models over one series in one set of launches (pgps_lti_ll_batch_f64).

    `models`: list of (F, Pinf, H, R) -- what lti_ll() takes, once per model; all of one state dimension."""
    packed, d = _lti_table(models)
    ts_a, ys_a, N = _series_inputs(ts, ys)
    out = np.zeros(len(models), np.float64)
    get_context(device).call("pgps_lti_ll_batch_f64", len(models), N, d, _ptr(packed), _ptr(ts_a), _ptr(ys_a), float(t0), _ptr(out))
    return out


def gp_ll_batch(models, ts, ys, t0=0.0, device=0):
    """Log-likelihoods of B models over one series (pgps_gp_ll_batch_*).

    `models`: list of (form=(lam, N1, N2), Pinf, H, R) -- what gp() takes, once per model."""
    ts_a, ys_a, N = _series_inputs(ts, ys, keep_f32=True)
    packed, d = _gp_rows(models)
    out = np.zeros(len(models), np.float64)
    get_context(device).call(f"pgps_gp_ll_batch_{_suffix(ts_a.dtype)[0]}", len(models), N, d, _ptr(packed), _ptr(ts_a), float(t0),
                             _ptr(ys_a), _ptr(out))
    return out


def gp_ll_grad_adj_batch(models, ts, ys, t0=0.0, device=0):
    """Log-likelihood and the model's adjoints of B fused (Matern-family, d <= 3) models over one float64 series in one set
    of launches (pgps_gp_ll_grad_adj_batch_f64).  `models` as gp_ll_batch takes them, or a table.  Returns a
    (B, 1 + d d + 2 d + 1) array, row b = [ll | Abar | Ubar | Hbar | Rbar] of model b (split_grad_stats)."""
    ts_a, ys_a, N = _series_inputs(ts, ys)
    packed, d = _gp_rows(models)
    ctx = _require(get_context(device), "pgps_gp_ll_grad_adj_batch_f64", "pgps_gp_ll_grad_adj_batch_*")
    out = np.empty((packed.shape[0], 2 + d * d + 2 * d), np.float64)
    ctx.call("pgps_gp_ll_grad_adj_batch_f64", packed.shape[0], N, d, _ptr(packed), _ptr(ts_a), float(t0), _ptr(ys_a), _ptr(out))
    return out


def lti_ll_grad_batch(models, ts, ys, t0=0.0, device=0):
    """Log-likelihood and the model's adjoints of B general LTI models [(F, Pinf, H, R)] of one state dimension over one
    series: a (B, 1 + d d + 2 d + 1) array, row b = [ll | Abar | Ubar | Hbar | Rbar] of model b (split_grad_stats).
    d = 2 .. 16: one set of launches on the row-cooperative kernels (pgps_lti_ll_grad_batch_f64); d = 17 .. 32: one
    asynchronous pgps_lti_ll_grad_dev_f64 per model on a private context, read once (LtiGradStream)."""
    d = 0 if isinstance(models, np.ndarray) else np.asarray(models[0][0]).shape[0]
    if LTI_BATCH_DIM_MAX < d <= LTI_DIM_MAX:
        with LtiGradStream(ts, ys, len(models), d, t0=t0, device=device) as stream:
            for F, Pinf, H, R in models:
                stream.push(F, Pinf, H, R)
            out = stream.finish()
        if not np.all(np.isfinite(out[:, 0])):
            raise PgpsError(E_NUMERIC, "pgps_lti_ll_grad_dev_f64: a log-likelihood of the batch is not finite")
        return out
    table, d = _lti_table(models)
    ts_a, ys_a, N = _series_inputs(ts, ys)
    ctx = _require(get_context(device), "pgps_lti_ll_grad_batch_f64", "pgps_lti_ll_grad_batch_*")
    out = np.empty((table.shape[0], 2 + d * d + 2 * d), np.float64)
    ctx.call("pgps_lti_ll_grad_batch_f64", table.shape[0], N, d, _ptr(table), _ptr(ts_a), _ptr(ys_a), float(t0), _ptr(out))
    return out


def gp_predict_batch(models, ts, ys, tq, t0=0.0, device=0, mix=None):
    """predict_f of B fused (Matern-family, d <= 3) models over one series and one query grid in one set of launches
    (pgps_gp_predict_batch_*): one merge of the sorted `ts` (N) and `tq` (K), B filters + smoothers + projections.
    `models` as gp_ll_batch takes them.  Returns (mean (B, K), var (B, K), ll (B,), None).  With `mix` (B normalised
    weights; float64 series) the (B, K) results stay on the device, k_mix_moments reduces them there and
    (None, None, ll, (mixture mean (K,), mixture variance (K,))) comes back."""
    ts_a, ys_a, tq_a, N = _series_inputs(ts, ys, tq, keep_f32=True)
    dtype, K = ts_a.dtype, tq_a.shape[0]
    packed, d = _gp_rows(models)
    B = packed.shape[0]
    ctx = get_context(device)
    ll = np.zeros(B, np.float64)
    if mix is None or dtype != np.float64:
        mean, var = np.empty((B, K), dtype), np.empty((B, K), dtype)
        ctx.call(f"pgps_gp_predict_batch_{_suffix(dtype)[0]}", B, N, K, d, _ptr(packed), _ptr(ts_a), _ptr(ys_a), float(t0),
                 _ptr(tq_a), _ptr(mean), _ptr(var), _ptr(ll))
        if mix is None:
            return mean, var, ll, None
        return None, None, ll, mix_moments(mean, var, mix, device=device)
    wv = _prep(mix, np.float64, (B,))
    mm, mv = np.empty(K, np.float64), np.empty(K, np.float64)
    bufs = []
    with ctx.lock:
        try:
            for nbytes in (8 * N, 8 * N, 8 * K, 8 * B * K, 8 * B * K, 8 * B, 8 * B, 8 * K, 8 * K):
                bufs.append(ctx.malloc(max(nbytes, 8)))
            dts, dys, dtq, dmean, dvar, dll, dw, dmm, dmv = (c_void_p(b) for b in bufs)
            ctx.h2d(bufs[0], ts_a)
            ctx.h2d(bufs[1], ys_a)
            ctx.h2d(bufs[2], tq_a)
            ctx.h2d(bufs[6], wv)
            ctx.call("pgps_gp_predict_batch_dev_f64", c_int(B), c_long(N), c_long(K), c_int(d), _ptr(packed), dts, dys,
                     c_double(float(t0)), dtq, dmean, dvar, dll)
            ctx.call("pgps_mix_moments_dev_f64", c_int(B), c_long(K), dmean, dvar, dw, dmm, dmv)
            ctx.d2h(mm, bufs[7])
            ctx.d2h(mv, bufs[8])
            ctx.d2h(ll, bufs[5])
        finally:
            for b in bufs:
                ctx.free(b)
    return None, None, ll, (mm, mv)


def lti_predict_batch(models, ts, ys, tq, t0=0.0, device=0, mix=None):
    """predict_f of B general LTI models [(F, Pinf, H, R)] (one state dimension, 2 .. 16) over one series and one query grid
    (pgps_lti_predict_batch_f64): one merge, the models side by side on the row-cooperative kernels, one copy back.  Returns
    (mean (B, K), var (B, K), ll (B,), None), or with `mix` (None, None, ll, mixture moments) reduced by mix_moments."""
    table, d = _lti_table(models)
    ts_a, ys_a, tq_a, N = _series_inputs(ts, ys, tq)
    K, B = tq_a.shape[0], table.shape[0]
    mean, var, ll = np.empty((B, K), np.float64), np.empty((B, K), np.float64), np.zeros(B, np.float64)
    get_context(device).call("pgps_lti_predict_batch_f64", B, N, K, d, _ptr(table), _ptr(ts_a), _ptr(ys_a), float(t0), _ptr(tq_a),
                             _ptr(mean), _ptr(var), _ptr(ll))
    if mix is None:
        return mean, var, ll, None
    return None, None, ll, mix_moments(mean, var, mix, device=device)


def mix_moments(mean, var, weights=None, device=0):
    """Moments of the mixture sum_b w_b N(mean_b, var_b) on the device (pgps_mix_moments_dev_f64, fp64): mean, var (B, K)
    host arrays, `weights` (B,) used as given (None: 1 / B each).  mix = sum_b w_b mean_b, then
    var = sum_b w_b (var_b + (mean_b - mix)^2): two passes, every term of the variance non-negative."""
    mean_a = _prep(mean, np.float64)
    var_a = _prep(var, np.float64, mean_a.shape)
    if mean_a.ndim != 2:
        raise ValueError(f"mean must be (B, K), got {mean_a.shape}")
    B, K = mean_a.shape
    wv = None if weights is None else _prep(weights, np.float64, (B,))
    mm, mv = np.empty(K, np.float64), np.empty(K, np.float64)
    if K == 0:
        return mm, mv
    ctx = get_context(device)
    bufs = []
    with ctx.lock:
        try:
            for nbytes in (8 * B * K, 8 * B * K, 8 * B, 8 * K, 8 * K):
                bufs.append(ctx.malloc(nbytes))
            ctx.h2d(bufs[0], mean_a)
            ctx.h2d(bufs[1], var_a)
            if wv is not None:
                ctx.h2d(bufs[2], wv)
            ctx.call("pgps_mix_moments_dev_f64", c_int(B), c_long(K), c_void_p(bufs[0]), c_void_p(bufs[1]),
                     c_void_p(bufs[2]) if wv is not None else None, c_void_p(bufs[3]), c_void_p(bufs[4]))
            ctx.d2h(mm, bufs[3])
            ctx.d2h(mv, bufs[4])
        finally:
            for b in bufs:
                ctx.free(b)
    return mm, mv
