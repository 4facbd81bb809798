"""References and data of the panel's mean-function tests (test_panel_trend_host.py, test_gpu_panel_trend.py).  Neither
reference is the code under test:
  np_gram      the multi-column loop of test_gpu_whiten._np_whiten with a per-step R + s_k on O.get_ssm's Fs, Qs: (G, logdet, n_obs)
               of V = [y, Phi] of ONE series;
  dense_gls    dense generalised least squares through het_refs.dense_het's covariance O.dense_K + diag(R + s) on the observed
               rows: (beta_hat, cov, profile ll, flat-mean marginal).
Data: het_refs.series(n, seed=i) with a different seed per series and 20 % missing, kernels het_refs.matern (variance 1,
lengthscale 0.5), R = 0.1.  Bases: Constant, Linear, Polynomial(2 / 3, center=0.55, scale=0.3).
well_posed() asserts, from the reference alone, the two conditions every case rests on: the unit-diagonal A has condition
number <= 100 and the trend leaves (g_yy - b^T A^-1 b) / g_yy >= 0.25 of y's whitened norm."""
import functools
import math

import numpy as np
import scipy.linalg as sla

from het_refs import LOG2PI, MATERNS, R, sde_of, series
from oracle import np_oracle as O

KNAMES = ("m12", "m32", "m52")
COND_MAX, GAP_MIN = 100.0, 0.25


def bases():
    from pssgp.mean_functions import Constant, Linear, Polynomial
    return {"constant": Constant(), "linear": Linear(), "quadratic": Polynomial(2, center=0.55, scale=0.3),
            "cubic": Polynomial(3, center=0.55, scale=0.3)}


def design(name, t):
    """Phi (n, p) of basis `name`, written out here (not the package's design())."""
    t = np.asarray(t, np.float64).reshape(-1)
    if name == "constant":
        return np.ones((t.size, 1))
    if name == "linear":
        return np.stack([np.ones(t.size), t], axis=1)
    u = (t - 0.55) / 0.3
    deg = {"quadratic": 2, "cubic": 3}[name]
    return np.stack([u ** j for j in range(deg + 1)], axis=1)


def columns(t, y, Phi):
    """V = [y, Phi] with the rows where y is NaN set to NaN in all columns."""
    V = np.concatenate([np.asarray(y, np.float64).reshape(-1, 1), np.asarray(Phi, np.float64)], axis=1)
    V[np.isnan(V[:, 0])] = np.nan
    return V


def wide_columns(t, y, C):
    """C columns for the kernel-level tests, where C goes beyond the four bases: y, then the cosine basis 1, cos(j pi x),
    x = t - 0.05 on about [0, 1] (orthogonal under a flat weight: the reference's condition number stays below 6 at C = 8,
    where 1, u, u^2, u^3 and sines reach 1300)."""
    t = np.asarray(t, np.float64).reshape(-1)
    cols = [np.ones(t.size)] + [np.cos(j * np.pi * (t - 0.05)) for j in range(1, 7)]
    return columns(t, y, np.stack(cols[:C - 1], axis=1) if C > 1 else np.zeros((t.size, 0)))


def np_gram(sde, t, V, Rv, s=None):
    """(G (C, C), logdet, n_obs): the sequential filter of all columns at once (one covariance, a (d, C) matrix of means),
    W[k] = r / sqrt(S_k) at the observed rows with S_k = h^T P h + Rv + s_k, G = W^T W."""
    t, V = np.asarray(t, np.float64).reshape(-1), np.asarray(V, np.float64)
    s = np.zeros(t.size) if s is None else np.asarray(s, np.float64).reshape(-1)
    seen = ~np.isnan(V[:, 0])
    P0, Fs, Qs, H, _ = O.get_ssm(sde, t, Rv)
    h = H.reshape(-1)
    m, P = np.zeros((h.size, V.shape[1])), P0.copy()
    W, logdet = np.zeros(V.shape), 0.0
    for k in range(t.size):
        m = Fs[k] @ m
        P = Fs[k] @ P @ Fs[k].T + Qs[k]
        P = 0.5 * (P + P.T)
        if seen[k]:
            S = float(h @ P @ h) + Rv + s[k]
            r = V[k] - h @ m
            W[k] = r / math.sqrt(S)
            logdet += math.log(S)
            u = P @ h
            m = m + np.outer(u, r / S)
            P = P - np.outer(u, u) / S
            P = 0.5 * (P + P.T)
    return W.T @ W, logdet, int(seen.sum())


def gls_from_gram(G, logdet, n_obs):
    """(beta_hat, cov, profile ll, flat-mean marginal, condition number of the unit-diagonal A, gap) from a Gram record."""
    g_yy, b, A = float(G[0, 0]), G[1:, 0], G[1:, 1:]
    p = A.shape[0]
    sc = 1.0 / np.sqrt(np.diag(A))
    Au = A * sc[:, None] * sc[None, :]
    cov = np.linalg.inv(Au) * sc[:, None] * sc[None, :]
    beta = cov @ b
    profile = -0.5 * (n_obs * LOG2PI + logdet + g_yy - float(b @ beta))
    flat = profile - 0.5 * float(np.linalg.slogdet(A)[1]) + 0.5 * p * LOG2PI
    return beta, cov, profile, flat, float(np.linalg.cond(Au)), (g_yy - float(b @ beta)) / g_yy


def dense_gls(spec, t, y, Phi, Rv, s=None):
    """(beta_hat, cov, profile ll, flat-mean marginal) of the dense GP with noise covariance diag(Rv + s) on the observed rows."""
    t, y = np.asarray(t, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    s = np.zeros(t.size) if s is None else np.asarray(s, np.float64).reshape(-1)
    o = ~np.isnan(y)
    L = np.linalg.cholesky(O.dense_K(spec, t[o], t[o]) + np.diag(Rv + s[o]))
    Wv = sla.solve_triangular(L, np.concatenate([y[o, None], np.asarray(Phi, np.float64)[o]], axis=1), lower=True)
    G = Wv.T @ Wv
    return gls_from_gram(G, 2.0 * float(np.sum(np.log(np.diag(L)))), int(o.sum()))[:4]


def well_posed(G, logdet, n_obs, what=""):
    """The two conditions of the module docstring, from a REFERENCE record; returns the condition number."""
    if G.shape[0] == 1:
        return 1.0
    *_, cond, gap = gls_from_gram(G, logdet, n_obs)
    assert cond <= COND_MAX, (what, "condition number of the unit-diagonal A", cond)
    assert gap >= GAP_MIN, (what, "(g_yy - b^T A^-1 b) / g_yy", gap)
    return cond


@functools.lru_cache(maxsize=None)
def panel(lengths):
    """[(t, y, s)] of the panel's series, read-only; series i has seed i."""
    out = []
    for i, n in enumerate(lengths):
        t, y, s = series(n, seed=i)
        for a in (t, y, s):
            a.setflags(write=False)
        out.append((t, y, s))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ref_gram(kname, lengths, i, het, basis=None, C=None):
    """The reference record of series i for basis `basis` (or the C wide columns): computed once, read-only."""
    t, y, s = panel(lengths)[i]
    V = columns(t, y, design(basis, t)) if basis is not None else wide_columns(t, y, C)
    G, logdet, n_obs = np_gram(sde_of(kname), t, V, R, s if het else None)
    G.setflags(write=False)
    return G, logdet, n_obs


def spec_of(kname):
    return MATERNS[kname][1]
