"""The fused path: discretisation inside the scan kernels (SDEs with F = -lam I + N, N nilpotent, d <= 3), and the
forward-mode gradient calls of the same models and of their block-diagonal composites."""
import ctypes

import numpy as np

from .arrays import _prep, _ptr, _scalar_out, _series_inputs, _suffix
from .context import get_context
from .library import _require
from .lti import split_grad_stats


def nilpotent_form(F, tol=1e-9):
    """(lam, N1, N2) with F = -lam I + N, N^d = 0, N1 = N, N2 = N^2 / 2 -- or None if F is not of
    that form (it is for every Matern kernel, balanced or not) or d > 3."""
    F = np.asarray(F, dtype=np.float64)
    d = F.shape[0]
    if d > 3:
        return None
    lam = -float(np.trace(F)) / d
    N = F + lam * np.eye(d)
    Np = np.linalg.matrix_power(N, d)
    scale = max(1.0, float(np.max(np.abs(F)))) ** d
    if not np.all(np.abs(Np) <= tol * scale) or lam <= 0:
        return None
    return lam, np.ascontiguousarray(N), np.ascontiguousarray(0.5 * (N @ N))


def _fused_model(form, Pinf, H):
    """(d, the arguments (lam, N1, N2, Pinf, H)) of the fused model, as every pgps_gp_* entry point takes them."""
    lam, N1, N2 = form
    d = N1.shape[0]
    return d, (float(lam), _ptr(_prep(N1, np.float64)), _ptr(_prep(N2, np.float64)), _ptr(_prep(Pinf, np.float64, (d, d))),
               _ptr(_prep(H, np.float64, (d,))))


def gp(form, Pinf, H, R, ts, ys, t0=0.0, want_filtered=False, want_smoothed=False, device=0):
    """Fused filter (+ smoother) + log-likelihood straight from times and observations.

    Returns a dict with "ll" and, on request, "fms", "fPs", "sms", "sPs" (host numpy arrays)."""
    ts_a, ys_a, N = _series_inputs(ts, ys, keep_f32=True)
    dtype = ts_a.dtype
    d, model = _fused_model(form, Pinf, H)
    want_filtered = want_filtered or want_smoothed
    out = {}
    fms = np.empty((N, d), dtype) if want_filtered else None
    fPs = np.empty((N, d, d), dtype) if want_filtered else None
    sms = np.empty((N, d), dtype) if want_smoothed else None
    sPs = np.empty((N, d, d), dtype) if want_smoothed else None
    ll, llp = _scalar_out()
    get_context(device).call(f"pgps_gp_{_suffix(dtype)[0]}", N, d, *model, float(R), _ptr(ts_a), float(t0), _ptr(ys_a),
                             _ptr(fms), _ptr(fPs), _ptr(sms), _ptr(sPs), llp)
    out["ll"] = np.asarray(ll.value, dtype=dtype)
    if want_filtered:
        out["fms"], out["fPs"] = fms, fPs
    if want_smoothed:
        out["sms"], out["sPs"] = sms, sPs
    return out


def gp_predict(form, Pinf, H, R, ts, ys, tq, t0=0.0, device=0):
    """predict_f on the device (pgps_gp_predict_*): merge of the sorted `ts` (N) and `tq` (K), fused
    filter + smoother over the N + K steps, posterior mean / variance of f = H x at the K query
    times.  Returns (mean (K,), var (K,), ll of the training series)."""
    ts_a, ys_a, tq_a, N = _series_inputs(ts, ys, tq, keep_f32=True)
    dtype, K = ts_a.dtype, tq_a.shape[0]
    d, model = _fused_model(form, Pinf, H)
    mean, var = np.empty(K, dtype), np.empty(K, dtype)
    ll, llp = _scalar_out()
    get_context(device).call(f"pgps_gp_predict_{_suffix(dtype)[0]}", N, K, d, *model, float(R), _ptr(ts_a), _ptr(ys_a),
                             float(t0), _ptr(tq_a), _ptr(mean), _ptr(var), llp)
    return mean, var, ll.value


def gp_ll_multi(form, Pinf, H, R, ts, Y, t0=0.0, device=0):
    """Log-likelihoods of the M columns of Y (N, M) -- M independent GPs that share the kernel, the noise and the inputs
    -- in one covariance pass (pgps_gp_ll_multi_f64): (M,).  Every row of Y is observed in all columns or NaN in all
    columns (a mixed row raises PgpsError with PGPS_E_INVALID)."""
    ts_a, Y_a, N = _series_inputs(ts, Y, columns=True)
    d, model = _fused_model(form, Pinf, H)
    M = Y_a.shape[1]
    ll = np.empty(M, np.float64)
    get_context(device).call("pgps_gp_ll_multi_f64", N, M, d, *model, float(R), _ptr(ts_a), _ptr(Y_a), float(t0), _ptr(ll))
    return ll


def gp_predict_multi(form, Pinf, H, R, ts, Y, tq, t0=0.0, device=0):
    """predict_f for the M columns of Y (N, M) in one covariance pass (pgps_gp_predict_multi_f64): the merge of the sorted
    `ts` (N) and `tq` (K), the column-tiled fused filter + smoother over the N + K steps, the projection at the K query
    times.  Returns (mean (K, M), var (K,) -- the same for every column --, ll (M,))."""
    ts_a, Y_a, tq_a, N = _series_inputs(ts, Y, tq, columns=True)
    d, model = _fused_model(form, Pinf, H)
    M, K = Y_a.shape[1], tq_a.shape[0]
    mean, var, ll = np.empty((K, M), np.float64), np.empty(K, np.float64), np.empty(M, np.float64)
    get_context(device).call("pgps_gp_predict_multi_f64", N, K, M, d, *model, float(R), _ptr(ts_a), _ptr(Y_a), float(t0),
                             _ptr(tq_a), _ptr(mean), _ptr(var), _ptr(ll))
    return mean, var, ll


def gp_ll_grad_multi(form, Pinf, H, R, ts, Y, t0=0.0, device=0):
    """Log-likelihoods of the M columns of Y (N, M) and the model's adjoints SUMMED over the columns, in one filter pass and one
    reverse pass on column tiles (pgps_gp_ll_grad_multi_f64): (ll (M,), Abar (d, d), Ubar (d,), Hbar (d,), Rbar) -- the
    statistics of sum_j ll[j], contracted by contract_grad_stats().  Rows of Y as gp_ll_multi takes them."""
    ts_a, Y_a, N = _series_inputs(ts, Y, columns=True)
    d, model = _fused_model(form, Pinf, H)
    M = Y_a.shape[1]
    ctx = _require(get_context(device), "pgps_gp_ll_grad_multi_f64", "pgps_gp_ll_grad_multi_*")
    out = np.zeros(M + d * d + 2 * d + 1, np.float64)
    ctx.call("pgps_gp_ll_grad_multi_f64", N, M, d, *model, float(R), _ptr(ts_a), _ptr(Y_a), float(t0), _ptr(out))
    return split_grad_stats(out, d, M)


GRAM_COLUMNS_MAX = 16           # pgps_gp_gram_multi_*: columns of V


def _whiten_call(name, form, Pinf, H, R, ts, V, out, t0, device):
    """pgps_gp_whiten_multi_f64 / pgps_gp_gram_multi_f64 on V (N, M): fills `out`, returns (logdet, n_obs)."""
    ts_a, V_a, N = _series_inputs(ts, V, columns=True)
    d, model = _fused_model(form, Pinf, H)
    ctx = _require(get_context(device), name, "pgps_gp_whiten_multi_* / pgps_gp_gram_multi_*")
    logdet, n_obs = ctypes.c_double(0.0), ctypes.c_long(0)
    ctx.call(name, N, V_a.shape[1], d, *model, float(R), _ptr(ts_a), _ptr(V_a), float(t0), _ptr(out), ctypes.byref(logdet),
             ctypes.byref(n_obs))
    return float(logdet.value), int(n_obs.value)


def gp_whiten_multi(form, Pinf, H, R, ts, V, t0=0.0, device=0):
    """The whitened columns of V (N, M), any M >= 1, in one covariance pass (pgps_gp_whiten_multi_f64): W = L^-1 V with
    K + R I = L L^T on the observed rows in time order -- the standardised innovations (V[k, c] - mu_c[k]) / sqrt(S_k) of the
    Kalman pass, exact 0.0 at the rows that are not observed.  Returns (W (N, M), logdet = sum log S_k, n_obs).  Rows of V as
    gp_ll_multi takes them."""
    V = np.asarray(V, np.float64)
    V = V[:, None] if V.ndim == 1 else V
    W = np.empty(V.shape, np.float64)
    return (W,) + _whiten_call("pgps_gp_whiten_multi_f64", form, Pinf, H, R, ts, V, W, t0, device)


def gp_gram_multi(form, Pinf, H, R, ts, V, t0=0.0, device=0):
    """G = W^T W = V^T (K + R I)^-1 V (M, M) for the M <= GRAM_COLUMNS_MAX columns of V (N, M), W as gp_whiten_multi returns
    it but kept on the device (pgps_gp_gram_multi_f64): symmetric bit for bit, equal bits from call to call.  Returns
    (G, logdet, n_obs).  More columns raise PgpsError (PGPS_E_INVALID)."""
    V = np.asarray(V, np.float64)
    V = V[:, None] if V.ndim == 1 else V
    G = np.empty((V.shape[1], V.shape[1]), np.float64)
    return (G,) + _whiten_call("pgps_gp_gram_multi_f64", form, Pinf, H, R, ts, V, G, t0, device)


def _het_context(device):
    return _require(get_context(device), "pgps_gp_ll_het_f64", "pgps_gp_*_het_*")


def gp_ll_het(form, Pinf, H, R, ts, ys, rs, t0=0.0, device=0):
    """Log-likelihood of a series whose observation k has noise variance R + rs[k] (pgps_gp_ll_het_f64): `rs` (N,) given
    per-observation variances, finite and >= 0 at the observed rows (ignored where ys is NaN), R >= 0 the shared jitter,
    R + rs[k] > 0.  fp64, d <= 3."""
    ts_a, ys_a, rs_a, N = _series_inputs(ts, ys, rs=rs)
    d, model = _fused_model(form, Pinf, H)
    ll, llp = _scalar_out()
    _het_context(device).call("pgps_gp_ll_het_f64", N, d, *model, float(R), _ptr(ts_a), _ptr(ys_a), _ptr(rs_a), float(t0), llp)
    return ll.value


def gp_predict_het(form, Pinf, H, R, ts, ys, rs, tq, t0=0.0, device=0):
    """predict_f under per-observation noise variances R + rs[k] (pgps_gp_predict_het_f64): the merge of the sorted `ts` (N)
    and `tq` (K) carries ys and rs, the fused filter + smoother runs over the N + K steps.  Returns (mean (K,), var (K,) of
    f, ll of the training series)."""
    ts_a, ys_a, tq_a, rs_a, N = _series_inputs(ts, ys, tq, rs)
    d, model = _fused_model(form, Pinf, H)
    K = tq_a.shape[0]
    mean, var = np.empty(K, np.float64), np.empty(K, np.float64)
    ll, llp = _scalar_out()
    _het_context(device).call("pgps_gp_predict_het_f64", N, K, d, *model, float(R), _ptr(ts_a), _ptr(ys_a), _ptr(rs_a),
                              float(t0), _ptr(tq_a), _ptr(mean), _ptr(var), llp)
    return mean, var, ll.value


def gp_ll_grad_adj_het(form, Pinf, H, R, ts, ys, rs, t0=0.0, device=0):
    """Log-likelihood and the model's adjoints under per-observation noise variances R + rs[k]
    (pgps_gp_ll_grad_adj_het_f64): (ll, Abar (d, d), Ubar (d,), Hbar (d,), Rbar), Rbar = d ll / d R = sum_k d ll / d (R + rs[k]);
    contracted by contract_grad_stats()."""
    ts_a, ys_a, rs_a, N = _series_inputs(ts, ys, rs=rs)
    d, model = _fused_model(form, Pinf, H)
    out = np.zeros(1 + d * d + 2 * d + 1, np.float64)
    _het_context(device).call("pgps_gp_ll_grad_adj_het_f64", N, d, *model, float(R), _ptr(ts_a), float(t0), _ptr(ys_a),
                              _ptr(rs_a), _ptr(out))
    return split_grad_stats(out, d)


def normal_log_density(y, mean, var):
    """log N(y | mean, var) elementwise in fp64; NaN where y is."""
    y, mean, var = (np.asarray(a, np.float64) for a in (y, mean, var))
    return -0.5 * (np.log(2.0 * np.pi) + np.log(var) + (y - mean) ** 2 / var)


def gp_loo(form, Pinf, H, R, ts, ys, t0=0.0, osa=True, loo=True, device=0):
    """The predictive checks of a fitted model against its own data in one filter and one smoother pass over the N training
    steps (pgps_gp_loo_f64; fp64, d <= 3, R > 0).  Returns a dict with "ll" (the log-likelihood) and "loo_lpd" (the sum over the
    observed rows of the leave-one-out log densities); with `osa`: "osa_mean", "osa_var" (N,), the law of y_k given the
    observations before it, and "osa_log_density"; with `loo`: "loo_mean", "loo_var", the law of y_k given all other
    observations, and "loo_log_density".  Variances include R; a log density is NaN where ys is (formed here from
    (ys, mean, var): the library stores none).  osa = loo = False: no per-step array is stored or copied back."""
    ts_a, ys_a, N = _series_inputs(ts, ys)
    d, model = _fused_model(form, Pinf, H)
    out = {}
    for want, name in ((osa, "osa"), (loo, "loo")):
        for part in ("mean", "var"):
            out[f"{name}_{part}"] = np.empty(N, np.float64) if want else None
    sums = np.zeros(2, np.float64)
    ctx = _require(get_context(device), "pgps_gp_loo_f64", "pgps_gp_loo_*")
    ctx.call("pgps_gp_loo_f64", N, d, *model, float(R), _ptr(ts_a), _ptr(ys_a), float(t0),
             _ptr(out["osa_mean"]), _ptr(out["osa_var"]), _ptr(out["loo_mean"]), _ptr(out["loo_var"]), _ptr(sums))
    for want, name in ((osa, "osa"), (loo, "loo")):
        if want:
            out[f"{name}_log_density"] = normal_log_density(ys_a, out[f"{name}_mean"], out[f"{name}_var"])
    out = {k: v for k, v in out.items() if v is not None}
    out["ll"], out["loo_lpd"] = float(sums[0]), float(sums[1])
    return out


# ----------------------------------------------------------------------------------------------
# forward-mode gradients: the model and its partial derivatives ride through the filter together
# ----------------------------------------------------------------------------------------------
def pack_grad_model(blocks):
    """(1 + np, 1 + 2 d^2 + d + 1) array [lam | N1 | Pinf | H | R] per block, as pgps_gp_ll_grad_* reads it."""
    d = np.asarray(blocks[0][1]).shape[0]
    dd = d * d
    model = np.empty((len(blocks), 2 + 2 * dd + d), np.float64)
    for r, (lam, N1, Pinf, H, R) in enumerate(blocks):
        row = model[r]
        row[0] = lam
        row[1:1 + dd] = np.asarray(N1, np.float64).reshape(-1)          # (a shape mismatch raises here)
        row[1 + dd:1 + 2 * dd] = np.asarray(Pinf, np.float64).reshape(-1)
        row[1 + 2 * dd:1 + 2 * dd + d] = np.asarray(H, np.float64).reshape(-1)
        row[-1] = R
    return model, d, len(blocks) - 1


def gp_ll_grad(blocks, ts, ys, t0=0.0, device=0):
    """Log-likelihood and its gradient on the fused path (pgps_gp_ll_grad_f64, fp64, d <= 3).

    `blocks`: list of 1 + np tuples (lam, N1, Pinf, H, R) -- the model, then its partial derivative
    with respect to each hyper-parameter.  Returns (ll, grad[np])."""
    model, d, npar = pack_grad_model(blocks)
    ts_a, ys_a, N = _series_inputs(ts, ys)
    out = np.zeros(1 + npar, np.float64)
    get_context(device).call("pgps_gp_ll_grad_f64", N, d, npar, _ptr(model), _ptr(ts_a), float(t0), _ptr(ys_a), _ptr(out))
    return out[0], out[1:]


GRAD_BLOCKS_DIM_MAX = 6        # pgps_gp_ll_grad_blocks_*: state dimension, blocks
GRAD_BLOCKS_MAX = 4


def nilpotent_blocks(F, tol=1e-9):
    """[(start, size, lam, N)] when F is block diagonal (contiguous blocks) with every block -lam I + N, N nilpotent --
    sums and products of Matern kernels, balanced or not -- else None.  Blocks = connected components of F's pattern."""
    F = np.asarray(F, np.float64)
    d = F.shape[0]
    scale = max(1.0, float(np.max(np.abs(F))))
    adj = (np.abs(F) > tol * scale) | (np.abs(F.T) > tol * scale) | np.eye(d, dtype=bool)
    comp = -np.ones(d, int)
    ncomp = 0
    for i in range(d):
        if comp[i] >= 0:
            continue
        stack, comp[i] = [i], ncomp
        while stack:
            u = stack.pop()
            for v in np.nonzero(adj[u])[0]:
                if comp[v] < 0:
                    comp[v] = ncomp
                    stack.append(v)
        ncomp += 1
    if np.any(np.diff(comp) < 0) or np.any(np.diff(comp) > 1):
        return None                                 # components must be contiguous index ranges, in order
    blocks = []
    for b in range(ncomp):
        idx = np.nonzero(comp == b)[0]
        lo, n = int(idx[0]), int(idx.size)
        Fb = F[lo:lo + n, lo:lo + n]
        lam = -float(np.trace(Fb)) / n              # all eigenvalues of a Matern block equal -lam (companion form)
        Nb = Fb + lam * np.eye(n)
        if not np.all(np.isfinite(Nb)) or np.max(np.abs(np.linalg.matrix_power(Nb, 4))) > tol * scale ** 4:
            return None                             # not nilpotent, or beyond the device series (it stops at N^3 / 6)
        blocks.append((lo, n, lam, Nb))
    return blocks


def gp_ll_grad_blocks(rows, bsizes, ts, ys, t0=0.0, device=0):
    """Log-likelihood and its exact gradient for a block-nilpotent composite model (pgps_gp_ll_grad_blocks_f64, fp64,
    2 <= d <= 6).  `rows`: 1 + np tuples (lams [nblk], N (d, d), Pinf (d, d), H (d,), R) -- the model, then its partial
    derivative with respect to each hyper-parameter; `bsizes`: the block sizes.  Returns (ll, grad[np])."""
    d = int(np.asarray(rows[0][1]).shape[0])
    nblk = len(bsizes)
    packed = []
    for lams, Nm, Pinf, H, R in rows:
        lam4 = np.zeros(GRAD_BLOCKS_MAX)
        lam4[:nblk] = np.asarray(lams, np.float64).reshape(-1)
        packed.append(np.concatenate([lam4, np.asarray(Nm, np.float64).reshape(-1), np.asarray(Pinf, np.float64).reshape(-1),
                                      np.asarray(H, np.float64).reshape(-1), [float(R)]]))
    model = np.ascontiguousarray(np.stack(packed), dtype=np.float64)
    npar = len(rows) - 1
    ts_a, ys_a, N = _series_inputs(ts, ys)
    bs = np.ascontiguousarray(bsizes, dtype=np.int32)
    out = np.zeros(1 + npar, np.float64)
    get_context(device).call("pgps_gp_ll_grad_blocks_f64", N, d, nblk, _ptr(bs), npar, _ptr(model), _ptr(ts_a), float(t0),
                             _ptr(ys_a), _ptr(out))
    return out[0], out[1:]
