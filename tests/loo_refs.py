"""References and data of the predictive-check tests (test_loo_host.py, test_gpu_loo.py): the one-step-ahead law
y_k | y_1..k-1 and the leave-one-out law y_k | y_-k of a fitted model.  None of the three is the code under test:
  ss_checks     a numpy sequential Kalman filter + RTS smoother with a per-step R on O.get_ssm's Fs, Qs (any kernel), then the
                cavity formula  var = R^2 / (R - v),  mean = (m R - y v) / (R - v);
  dense_checks  dense algebra over the observed rows with O.dense_K (exact for the Matern family): leave-one-out by
                mu_i = y_i - [K_y^-1 y]_i / [K_y^-1]_ii,  var_i = 1 / [K_y^-1]_ii  (Rasmussen & Williams eq. 5.12), one step
                ahead from the Cholesky factor of K_y in time order (S_k = L_kk^2, y_k - mu_k = L_kk [L^-1 y]_k);
  brute_force   row i set to NaN and the EXISTING predict_f asked at t_i (test_loo_host.py).
"""
import functools
import math

import numpy as np
import scipy.linalg as sla

from het_refs import MATERNS, R, matern, rel, sde_of, series  # noqa: F401  (re-exported to the tests)
from oracle import np_oracle as O

LOG2PI = math.log(2.0 * math.pi)
TOL = 1e-9                      # the project's: max norm relative to the largest entry
FIELDS = ("osa_mean", "osa_var", "loo_mean", "loo_var")


def log_density(y, mean, var):
    return -0.5 * (LOG2PI + np.log(var) + (y - mean) ** 2 / var)


def ss_checks(sde, t, y, Rk, ssm=None):
    """dict of FIELDS (N,), "osa_log_density", "loo_log_density" (NaN at the NaN rows of y), "ll", "loo_lpd" from the
    state-space form; Rk scalar or (N,).  `ssm`: O.get_ssm(sde, t, .) where the caller has it already."""
    t, y = (np.asarray(a, np.float64).reshape(-1) for a in (t, y))
    Rk = np.broadcast_to(np.asarray(Rk, np.float64), t.shape)
    P0, Fs, Qs, H, _ = O.get_ssm(sde, t, 1.0) if ssm is None else ssm
    h = H.reshape(-1)
    n, d = t.size, h.size
    m, P = np.zeros(d), P0.copy()
    fm, fP, pm, pP = np.empty((n, d)), np.empty((n, d, d)), np.empty((n, d)), np.empty((n, d, d))
    for k in range(n):
        m = Fs[k] @ m
        P = Fs[k] @ P @ Fs[k].T + Qs[k]
        P = 0.5 * (P + P.T)
        pm[k], pP[k] = m, P
        if not np.isnan(y[k]):
            S = float(h @ P @ h) + Rk[k]
            u = P @ h
            m = m + u * ((y[k] - float(h @ m)) / S)
            P = P - np.outer(u, u) / S
            P = 0.5 * (P + P.T)
        fm[k], fP[k] = m, P
    sm, sP = fm.copy(), fP.copy()
    for k in range(n - 2, -1, -1):
        G = np.linalg.solve(pP[k + 1], Fs[k + 1] @ fP[k]).T
        sm[k] = fm[k] + G @ (sm[k + 1] - pm[k + 1])
        sP[k] = fP[k] + G @ (sP[k + 1] - pP[k + 1]) @ G.T
    out = {"osa_mean": pm @ h, "osa_var": np.einsum("i,nij,j->n", h, pP, h) + Rk}
    mf, vf = sm @ h, np.einsum("i,nij,j->n", h, sP, h)
    obs = ~np.isnan(y)
    out["loo_mean"], out["loo_var"] = mf.copy(), vf + Rk
    out["loo_mean"][obs] = (mf[obs] * Rk[obs] - y[obs] * vf[obs]) / (Rk[obs] - vf[obs])
    out["loo_var"][obs] = Rk[obs] ** 2 / (Rk[obs] - vf[obs])
    out["gap"] = float(np.min((Rk[obs] - vf[obs]) / Rk[obs]))           # (how benign the subtraction is)
    for name in ("osa", "loo"):
        out[f"{name}_log_density"] = log_density(y, out[f"{name}_mean"], out[f"{name}_var"])
    out["ll"] = float(np.sum(out["osa_log_density"][obs]))
    out["loo_lpd"] = float(np.sum(out["loo_log_density"][obs]))
    return out


def dense_checks(spec, t, y, Rk):
    """The same at the OBSERVED rows only (arrays of length obs.sum(), in row order) from dense algebra, plus "ll", "loo_lpd"."""
    t, y = (np.asarray(a, np.float64).reshape(-1) for a in (t, y))
    Rk = np.broadcast_to(np.asarray(Rk, np.float64), t.shape)
    o = ~np.isnan(y)
    to, yo = t[o], y[o]
    Ky = O.dense_K(spec, to, to) + np.diag(Rk[o])
    Ki = np.linalg.inv(Ky)
    out = {"loo_mean": yo - (Ki @ yo) / np.diag(Ki), "loo_var": 1.0 / np.diag(Ki)}
    L = np.linalg.cholesky(Ky)                      # (rows in time order: column k conditions on the rows before k)
    z = sla.solve_triangular(L, yo, lower=True)
    out["osa_var"] = np.diag(L) ** 2
    out["osa_mean"] = yo - np.diag(L) * z
    out["ll"] = float(np.sum(log_density(yo, out["osa_mean"], out["osa_var"])))
    out["loo_lpd"] = float(np.sum(log_density(yo, out["loo_mean"], out["loo_var"])))
    return out


def repeated_times(n=300, repeats=5):
    """series(n) with `repeats` pairs of equal consecutive times (dt = 0), observed rows on both sides of at least one."""
    t, y, s = series(n)
    t = t.copy()
    for i in np.linspace(20, n - 20, repeats).astype(int):
        t[i + 1] = t[i]
    assert np.all(np.diff(t) >= 0) and int(np.sum(np.diff(t) == 0)) == repeats
    return t, y, s


@functools.lru_cache(maxsize=None)
def case(n, run=None, repeated=False):
    t, y, s = repeated_times(n) if repeated else series(n, run=run)
    for a in (t, y, s):
        a.setflags(write=False)
    return t, y, s


@functools.lru_cache(maxsize=None)
def refs(kname, n, run=None, repeated=False):
    """(state-space reference, dense reference) of the scalar-noise model on case(n, run, repeated): computed once, shared."""
    t, y, _ = case(n, run, repeated)
    return ss_checks(sde_of(kname), t, y, R), dense_checks(MATERNS[kname][1], t, y, R)


def err(got, want):
    """rel(); a reference with no entry above rel()'s floor of 1e-6 -- the N = 1 means, zero up to the rounding of a difference
    of terms of order y R -- is compared absolutely."""
    want = np.asarray(want, np.float64)
    if float(np.max(np.abs(want))) < 1e-6:
        return float(np.max(np.abs(np.asarray(got, np.float64) - want)))
    return rel(got, want)


def gaps(got, kname, n, run=None, repeated=False):
    """(largest error of the four arrays and the two sums against the state-space reference; against the dense one at the
    observed rows).  `got`: a dict with FIELDS, "ll", "loo_lpd"."""
    ss, dn = refs(kname, n, run, repeated)
    obs = ~np.isnan(case(n, run, repeated)[1])
    e_ss = [err(got[f], ss[f]) for f in FIELDS] + [abs(got[s] - ss[s]) / abs(ss[s]) for s in ("ll", "loo_lpd")]
    e_dn = [err(np.asarray(got[f])[obs], dn[f]) for f in FIELDS] + [abs(got[s] - dn[s]) / abs(dn[s]) for s in ("ll", "loo_lpd")]
    return max(e_ss), max(e_dn)
