"""The array path: a discretised model (P0, Fs, Qs, H, R) through the parallel filter, smoother, draws and joint covariance."""
import numpy as np

from .arrays import _check_rows, _float_dtype, _prep, _ptr, _scalar_out, _suffix
from .context import get_context


def discretise(F, Pinf, ts, t0=0.0, device=0):
    """Fs, Qs = expm(dt F), Pinf - Fs Pinf Fs^T on the GPU (host arrays in and out)."""
    dtype = _float_dtype(ts)
    suf, _ = _suffix(dtype)
    F = _prep(F, dtype)
    d = F.shape[0]
    Pinf = _prep(Pinf, dtype, (d, d))
    ts = _prep(ts, dtype, (-1,))
    N = ts.shape[0]
    Fs = np.empty((N, d, d), dtype)
    Qs = np.empty((N, d, d), dtype)
    get_context(device).call(f"pgps_discretise_{suf}", N, d, _ptr(F), _ptr(Pinf), _ptr(ts), float(t0), _ptr(Fs), _ptr(Qs))
    return Fs, Qs


def _unpack_lgssm(lgssm, dtype):
    P0, Fs, Qs, H, R = lgssm
    Fs = _prep(Fs, dtype)
    N, d = Fs.shape[0], Fs.shape[1]
    return (_prep(P0, dtype, (d, d)), Fs, _prep(Qs, dtype, (N, d, d)), _prep(H, dtype, (d,)),
            float(np.asarray(R).reshape(())), N, d)


def _dtype_of(lgssm):
    return _float_dtype(lgssm[1])


def pkf(lgssm, observations, return_loglikelihood=False, device=0):
    dtype = _dtype_of(lgssm)
    suf, _ = _suffix(dtype)
    P0, Fs, Qs, H, R, N, d = _unpack_lgssm(lgssm, dtype)
    ys = _prep(observations, dtype, (-1,))
    _check_rows(ys, N, "model")
    fms = np.empty((N, d), dtype)
    fPs = np.empty((N, d, d), dtype)
    ll, llp = _scalar_out()
    get_context(device).call(f"pgps_pkf_{suf}", N, d, _ptr(P0), _ptr(Fs), _ptr(Qs), _ptr(H), R, _ptr(ys), _ptr(fms), _ptr(fPs),
                             llp if return_loglikelihood else None)
    if return_loglikelihood:
        return fms, fPs, np.asarray(ll.value, dtype=dtype)
    return fms, fPs


def pks(lgssm, ms, Ps, device=0):
    dtype = _dtype_of(lgssm)
    suf, _ = _suffix(dtype)
    _, Fs, Qs, *_ = lgssm
    Fs = _prep(Fs, dtype)
    N, d = Fs.shape[0], Fs.shape[1]
    Qs = _prep(Qs, dtype, (N, d, d))
    ms = _prep(ms, dtype, (N, d))
    Ps = _prep(Ps, dtype, (N, d, d))
    sms = np.empty((N, d), dtype)
    sPs = np.empty((N, d, d), dtype)
    get_context(device).call(f"pgps_pks_{suf}", N, d, _ptr(Fs), _ptr(Qs), _ptr(ms), _ptr(Ps), _ptr(sms), _ptr(sPs))
    return sms, sPs


def pkfs(lgssm, observations, return_filtered=False, return_loglikelihood=False, device=0):
    dtype = _dtype_of(lgssm)
    suf, _ = _suffix(dtype)
    P0, Fs, Qs, H, R, N, d = _unpack_lgssm(lgssm, dtype)
    ys = _prep(observations, dtype, (-1,))
    _check_rows(ys, N, "model")
    fms = np.empty((N, d), dtype) if return_filtered else None
    fPs = np.empty((N, d, d), dtype) if return_filtered else None
    sms = np.empty((N, d), dtype)
    sPs = np.empty((N, d, d), dtype)
    ll, llp = _scalar_out()
    get_context(device).call(f"pgps_pkfs_{suf}", N, d, _ptr(P0), _ptr(Fs), _ptr(Qs), _ptr(H), R, _ptr(ys), _ptr(fms), _ptr(fPs),
                             _ptr(sms), _ptr(sPs), llp)
    out = (sms, sPs)
    if return_filtered:
        out += (fms, fPs)
    if return_loglikelihood:
        out += (np.asarray(ll.value, dtype=dtype),)
    return out


def _sample_inputs(lgssm, ms, Ps, num_samples, first_sample, z, H):
    dtype = _dtype_of(lgssm)
    _, Fs, Qs, *_ = lgssm
    Fs = _prep(Fs, dtype)
    N, d = Fs.shape[0], Fs.shape[1]
    S = int(num_samples)
    if S < 1 or int(first_sample) < 0:
        raise ValueError(f"num_samples must be >= 1 and first_sample >= 0, got {num_samples}, {first_sample}")
    z = None if z is None else _prep(z, dtype, (S, N, d))
    H = None if H is None else _prep(H, dtype, (d,))
    return (dtype, N, d, S, Fs, _prep(Qs, dtype, (N, d, d)), _prep(ms, dtype, (N, d)), _prep(Ps, dtype, (N, d, d)), z, H)


def pks_sample(lgssm, ms, Ps, num_samples, seed, first_sample=0, z=None, H=None, device=0):
    """Joint posterior draws of x_0 .. x_{N-1} by parallel backward sampling (pgps_pks_sample_*): Fs, Qs of `lgssm` and
    the filtered moments ms (N, d), Ps (N, d, d) -> (S, N, d), or (S, N) of H x_k when H (d,) is given.  z (S, N, d):
    the standard normals to use; None = the library's draws of samples first_sample .. first_sample + S - 1 under
    `seed` (a fixed function of (seed, sample, step, component): the host twin ks_sample draws the same)."""
    dtype, N, d, S, Fs, Qs, ms, Ps, z, H = _sample_inputs(lgssm, ms, Ps, num_samples, first_sample, z, H)
    suf, _ = _suffix(dtype)
    out = np.empty((S, N) if H is not None else (S, N, d), dtype)
    get_context(device).call(f"pgps_pks_sample_{suf}", N, d, _ptr(Fs), _ptr(Qs), _ptr(ms), _ptr(Ps), S, int(first_sample),
                             int(seed) & (2 ** 64 - 1), _ptr(z), _ptr(H), _ptr(out))
    return out


def _cov_inputs(lgssm, Ps, sPs, steps, H):
    dtype = _dtype_of(lgssm)
    _, Fs, Qs, *_ = lgssm
    Fs = _prep(Fs, dtype)
    N, d = Fs.shape[0], Fs.shape[1]
    sel = np.ascontiguousarray(np.asarray(steps).reshape(-1), dtype=np.int64)
    n = sel.shape[0]
    if n < 1 or sel[0] < 0 or sel[-1] >= N or np.any(np.diff(sel) <= 0):
        raise ValueError(f"steps must be a non-empty, strictly increasing selection of 0..{N - 1}")
    H = None if H is None else _prep(H, dtype, (d,))
    out = np.empty((n, n) if H is not None else (n, n, d, d), dtype)
    return dtype, N, d, n, Fs, _prep(Qs, dtype, (N, d, d)), _prep(Ps, dtype, (N, d, d)), _prep(sPs, dtype, (N, d, d)), sel, H, out


def pks_cov(lgssm, Ps, sPs, steps, H=None, device=0):
    """Joint posterior covariance of the states at the selected `steps` (strictly increasing indices) on the GPU
    (pgps_pks_cov_*): Fs, Qs of `lgssm`, the filtered covariances Ps (N, d, d) and the smoothed ones sPs (N, d, d) ->
    (n, n, d, d) blocks out[a, b] = Cov(x_steps[a], x_steps[b] | ys), or (n, n) of H Cov H^T when H (d,) is given.  The
    products of the smoother gains between consecutive selected steps by a segmented scan, then the fill: no dense
    algebra over the N steps.  d <= 6 (larger: PgpsError, PGPS_E_UNSUPPORTED_DIM); the host twin is sequential.ks_cov."""
    dtype, N, d, n, Fs, Qs, Ps, sPs, sel, H, out = _cov_inputs(lgssm, Ps, sPs, steps, H)
    suf, _ = _suffix(dtype)
    get_context(device).call(f"pgps_pks_cov_{suf}", N, d, _ptr(Fs), _ptr(Qs), _ptr(Ps), _ptr(sPs), n, _ptr(sel), _ptr(H), _ptr(out))
    return out
