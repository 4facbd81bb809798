"""Sequential Kalman filter / RTS smoother: the reference's `kf / ks / kfs`
(pssgp/kalman/sequential.py:11-73), the `parallel=False` mode of StateSpaceGP.

Runs on the host like the reference's (`tf.scan` on `/cpu:0`), through the C++ twins in
libpgps.so (`pgps_seq_kf_* / pgps_seq_ks_*`, csrc/pgps_seq_host.cpp).
"""
import numpy as np

from .. import _backend

__all__ = ["kf", "ks", "kfs", "ks_sample", "sample_normals", "ks_cov"]

_ptr = _backend._ptr


def kf(lgssm, observations, return_loglikelihood=False, return_predicted=False, observation_variances=None):
    """observation_variances (N,): the noise variance of EVERY step (pgps_seq_kf_het_*), in place of the model's R -- read
    where the observation is not NaN only.  None: the model's R at every step."""
    lib = _backend.load_library()
    dtype = _backend._dtype_of(lgssm)
    suf, _ = _backend._suffix(dtype)
    P0, Fs, Qs, H, R, N, d = _backend._unpack_lgssm(lgssm, dtype)
    ys = _backend._prep(observations, dtype, (-1,))
    fms, fPs = np.empty((N, d), dtype), np.empty((N, d, d), dtype)
    mps = np.empty((N, d), dtype) if return_predicted else None
    Pps = np.empty((N, d, d), dtype) if return_predicted else None
    ll, llp = _backend._scalar_out()
    if observation_variances is not None:
        noise = _backend._prep(observation_variances, dtype, (-1,))
        if noise.shape[0] != N:
            raise ValueError(f"observation_variances has {noise.shape[0]} entries, the series {N} steps")
        name, noise = "pgps_seq_kf_het", _ptr(noise)
    else:
        name, noise = "pgps_seq_kf", R
    code = getattr(lib, f"{name}_{suf}")(N, d, _ptr(P0), _ptr(Fs), _ptr(Qs), _ptr(H), noise, _ptr(ys), _ptr(fms), _ptr(fPs), llp,
                                         _ptr(mps), _ptr(Pps))
    _backend.check(None, code, name)
    out = (fms, fPs)
    if return_loglikelihood:
        out += (np.asarray(ll.value, dtype=dtype),)
    if return_predicted:
        out += (mps, Pps)
    return out


def ks(lgssm, ms, Ps, mps, Pps):
    lib = _backend.load_library()
    dtype = _backend._dtype_of(lgssm)
    suf, _ = _backend._suffix(dtype)
    Fs = _backend._prep(lgssm[1], dtype)
    N, d = Fs.shape[0], Fs.shape[1]
    ms, mps = _backend._prep(ms, dtype, (N, d)), _backend._prep(mps, dtype, (N, d))
    Ps, Pps = _backend._prep(Ps, dtype, (N, d, d)), _backend._prep(Pps, dtype, (N, d, d))
    sms, sPs = np.empty((N, d), dtype), np.empty((N, d, d), dtype)
    code = getattr(lib, f"pgps_seq_ks_{suf}")(N, d, _ptr(Fs), _ptr(ms), _ptr(Ps), _ptr(mps), _ptr(Pps),
                                              _ptr(sms), _ptr(sPs))
    _backend.check(None, code, "pgps_seq_ks")
    return sms, sPs


def kfs(model, observations, observation_variances=None):
    fms, fPs, mps, Pps = kf(model, observations, return_predicted=True, observation_variances=observation_variances)
    return ks(model, fms, fPs, mps, Pps)


def ks_sample(lgssm, ms, Ps, num_samples=1, seed=0, first_sample=0, z=None, H=None):
    """Host twin of parallel.pks_sample (pgps_seq_ks_sample_*): the same backward-sampling recursion and the same
    draws, any d.  (S, N, d), or (S, N) of H x_k when H is given."""
    lib = _backend.load_library()
    dtype, N, d, S, Fs, Qs, ms, Ps, z, H = _backend._sample_inputs(lgssm, ms, Ps, num_samples, first_sample, z, H)
    suf, _ = _backend._suffix(dtype)
    out = np.empty((S, N) if H is not None else (S, N, d), dtype)
    code = getattr(lib, f"pgps_seq_ks_sample_{suf}")(N, d, _ptr(Fs), _ptr(Qs), _ptr(ms), _ptr(Ps), S, int(first_sample),
                                                     int(seed) & (2 ** 64 - 1), _ptr(z), _ptr(H), _ptr(out))
    _backend.check(None, code, "pgps_seq_ks_sample")
    return out


def ks_cov(lgssm, Ps, sPs, steps, H=None):
    """Host twin of parallel.pks_cov (pgps_seq_ks_cov_*): the same definition, any d.  (n, n, d, d), or (n, n) of
    H Cov H^T when H is given."""
    lib = _backend.load_library()
    dtype, N, d, n, Fs, Qs, Ps, sPs, sel, H, out = _backend._cov_inputs(lgssm, Ps, sPs, steps, H)
    suf, _ = _backend._suffix(dtype)
    code = getattr(lib, f"pgps_seq_ks_cov_{suf}")(N, d, _ptr(Fs), _ptr(Qs), _ptr(Ps), _ptr(sPs), n, _ptr(sel), _ptr(H),
                                                  _ptr(out))
    _backend.check(None, code, "pgps_seq_ks_cov")
    return out


def sample_normals(N, d, num_samples, seed, first_sample=0, dtype=np.float64):
    """The library's standard normal draws (S, N, d) of samples first_sample .. first_sample + S - 1 (host)."""
    lib = _backend.load_library()
    suf, _ = _backend._suffix(dtype)
    z = np.empty((int(num_samples), int(N), int(d)), dtype)
    code = getattr(lib, f"pgps_seq_sample_normals_{suf}")(int(N), int(d), int(num_samples), int(first_sample),
                                                         int(seed) & (2 ** 64 - 1), _ptr(z))
    _backend.check(None, code, "pgps_seq_sample_normals")
    return z
