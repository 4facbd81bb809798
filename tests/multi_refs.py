"""Data and the plain reference of the multi-output tests at realistic launch geometries (test_multi_refs_host.py,
test_gpu_multi_geometries.py): Y (N, M) is M independent GPs that share the kernel, the noise variance R and the inputs; a row
of Y is observed in all columns or in none.
  multi_series   times with steps spacing x U(0.5, 1.5) (het_refs.spaced_series' clock), M noisy sums of two slow sines;
  merged_rows    the series a predict call filters: het_refs.merged with the source ROW of every merged step as its payload;
  ss_multi       a numpy sequential Kalman filter + RTS smoother over that series which carries ONE covariance and a (d, M)
                 matrix of means, on O.get_ssm's Fs, Qs -- as het_refs.ss_het does it for one column.
Neither is the code under test.  Kernels and noise are het_refs': sde_of("m12" | "m32" | "m52") (variance 1, lengthscale 0.5),
R = 0.1.  The gradient's reference stays oracle.np_grad.ll_grad_stats per column, summed over the columns."""
import math

import numpy as np

from het_refs import LOG2PI, R, merged
from oracle import np_oracle as O


def multi_series(n, m, spacing, seed=0, extra_missing=()):
    """(t (n,), Y (n, m)).  20 % of the rows are NaN in every column, rows 0 and n - 1 among them; row n // 2 is observed;
    the rows of `extra_missing` are NaN too."""
    rng = np.random.RandomState(6000 + n + m + seed)
    t = 0.05 + np.cumsum(spacing * rng.uniform(0.5, 1.5, n))
    Y = (np.sin(0.7 * t)[:, None] * rng.uniform(0.5, 2.0, (1, m)) + 0.5 * np.sin(0.13 * t + 1.0)[:, None]
         + np.sqrt(R) * rng.randn(n, m))
    miss = rng.rand(n) < 0.2
    miss[[0, n - 1]] = True
    miss[n // 2] = False
    miss[list(extra_missing)] = True
    Y[miss] = np.nan
    return t, Y


def merged_rows(t, Y, tq):
    """(t (n + k,), Y (n + k, M), is-a-query) of the merge of the sorted queries into the training rows (a query before a
    training row of the same time): Y is NaN in every column at the query rows."""
    t, tq = (np.asarray(a, np.float64).reshape(-1) for a in (t, tq))
    Y = np.asarray(Y, np.float64)
    tm, row, _, isq = merged(t, np.arange(t.size, dtype=np.float64), np.zeros(t.size), tq)
    Ym = np.full((tm.size, Y.shape[1]), np.nan)
    Ym[~isq] = Y[row[~isq].astype(np.int64)]
    return tm, Ym, isq


def ss_multi(sde, t, Y, R, tq=None, ssm=None):
    """ll (M,) of the columns of Y (and, with tq, mean (K, M) and var (K,) of f at tq) from the state-space form.
    `ssm`: O.get_ssm(sde, t', .) of the series t' that is filtered (t, or t merged with tq), where the caller has it already."""
    t = np.asarray(t, np.float64).reshape(-1)
    Y = np.asarray(Y, np.float64)
    assert Y.ndim == 2 and Y.shape[0] == t.size
    if tq is not None:
        t, Y, isq = merged_rows(t, Y, tq)
    nan = np.isnan(Y)
    assert np.array_equal(nan.any(axis=1), nan.all(axis=1)), "a row is observed in all columns or in none"
    seen = ~nan[:, 0]
    P0, Fs, Qs, H, _ = O.get_ssm(sde, t, R) if ssm is None else ssm
    h = H.reshape(-1)
    n, d, M = t.size, h.size, Y.shape[1]
    m, P, ll = np.zeros((d, M)), P0.copy(), np.zeros(M)
    fm, fP, pm, pP = np.empty((n, d, M)), np.empty((n, d, d)), np.empty((n, d, M)), np.empty((n, d, d))
    for k in range(n):
        m = Fs[k] @ m
        P = Fs[k] @ P @ Fs[k].T + Qs[k]
        P = 0.5 * (P + P.T)
        pm[k], pP[k] = m, P
        if seen[k]:
            S = float(h @ P @ h) + R
            r = Y[k] - h @ m
            ll += -0.5 * (LOG2PI + math.log(S) + r * r / S)
            u = P @ h
            m = m + np.outer(u, r / S)
            P = P - np.outer(u, u) / S
            P = 0.5 * (P + P.T)
        fm[k], fP[k] = m, P
    if tq is None:
        return ll
    sm, sP = fm.copy(), fP.copy()
    for k in range(n - 2, -1, -1):
        G = np.linalg.solve(pP[k + 1], Fs[k + 1] @ fP[k]).T
        sm[k] = fm[k] + G @ (sm[k + 1] - pm[k + 1])
        sP[k] = fP[k] + G @ (sP[k + 1] - pP[k + 1]) @ G.T
    q = np.flatnonzero(isq)
    return ll, np.einsum("i,nim->nm", h, sm[q]), np.einsum("i,nij,j->n", h, sP[q], h)
