"""References and data of the per-observation-noise tests (test_het_noise_host.py, test_gpu_het_noise.py):
y_k = f(t_k) + e_k, e_k ~ N(0, R + s_k).  Neither reference is the code under test:
  dense_het   dense conditioning with O.dense_K(spec, t, t) + diag(R + s) over the observed rows (exact for the Matern family);
  ss_het      a numpy sequential Kalman filter + RTS smoother with a per-step R on O.get_ssm's Fs, Qs (any kernel).
"""
import functools
import math

import numpy as np
import scipy.linalg as sla

from oracle import np_oracle as O

LOG2PI = math.log(2.0 * math.pi)
R = 0.1
# (kernel class name, dense spec, tolerance against the dense GP: kernel_zoo's, tests/conftest.py)
MATERNS = {"m12": ("Matern12", ("matern12", 1., 0.5), 1e-6), "m32": ("Matern32", ("matern32", 1., 0.5), 1e-6),
           "m52": ("Matern52", ("matern52", 1., 0.5), 1e-6)}


def matern(kname):
    import pssgp.kernels as Kn
    return getattr(Kn, MATERNS[kname][0])(variance=1., lengthscales=0.5)


def dense_het(spec, t, y, R, s, tq=None):
    """ll (and mean, var of f at tq) of the dense GP with noise covariance diag(R + s); NaN rows of y carry no observation."""
    t, y, s = (np.asarray(a, np.float64).reshape(-1) for a in (t, y, s))
    o = ~np.isnan(y)
    C = O.dense_K(spec, t[o], t[o]) + np.diag(R + s[o])
    L = np.linalg.cholesky(C)
    alpha = sla.solve_triangular(L, y[o], lower=True)
    ll = -0.5 * float(alpha @ alpha) - float(np.sum(np.log(np.diag(L)))) - 0.5 * int(o.sum()) * LOG2PI
    if tq is None:
        return ll
    tq = np.asarray(tq, np.float64).reshape(-1)
    A = sla.solve_triangular(L, O.dense_K(spec, t[o], tq), lower=True)
    return ll, A.T @ alpha, np.diag(O.dense_K(spec, tq, tq)) - np.sum(A * A, axis=0)


def merged(t, y, Rk, tq):
    """(t, y, Rk, is-a-query) of the series the predict calls filter: the sorted queries merged into the training rows (a query
    before a training row of the same time), y and Rk NaN at the query rows."""
    t, y, Rk, tq = (np.asarray(a, np.float64).reshape(-1) for a in (t, y, Rk, tq))
    nanq = np.full(tq.size, np.nan)
    return O.merge_sorted(t, tq, (y, nanq), (Rk, nanq), (np.zeros(t.size, bool), np.ones(tq.size, bool)))


def ss_het(sde, t, y, R, s, tq=None, ssm=None):
    """The same from the state-space form: sequential Kalman filter (+ RTS smoother over the merged series) with R_k = R + s_k.
    `ssm`: O.get_ssm(sde, t', .) of the series t' that is filtered (t, or t merged with tq), where the caller has it already."""
    t, y, s = (np.asarray(a, np.float64).reshape(-1) for a in (t, y, s))
    Rk = R + s
    if tq is not None:
        t, y, Rk, isq = merged(t, y, Rk, tq)
    P0, Fs, Qs, H, _ = O.get_ssm(sde, t, R) if ssm is None else ssm
    h = H.reshape(-1)
    n, d = t.size, h.size
    m, P, ll = np.zeros(d), P0.copy(), 0.0
    fm, fP, pm, pP = np.empty((n, d)), np.empty((n, d, d)), np.empty((n, d)), np.empty((n, d, d))
    for k in range(n):
        m = Fs[k] @ m
        P = Fs[k] @ P @ Fs[k].T + Qs[k]
        P = 0.5 * (P + P.T)
        pm[k], pP[k] = m, P
        if not np.isnan(y[k]):
            S = float(h @ P @ h) + Rk[k]
            r = y[k] - float(h @ m)
            ll += -0.5 * (LOG2PI + math.log(S) + r * r / S)
            u = P @ h
            m = m + u * (r / S)
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
    return ll, sm[q] @ h, np.einsum("i,nij,j->n", h, sP[q], h)


def series(n, seed=0, missing=0.2, run=None):
    """Sorted times on about [0, 1] (the zoo's lengthscale is 0.5), a noisy sum of sines, `missing` of the rows NaN (from 10
    rows on; `run` = (first, length): these rows too), s log-uniform over two decades [0.01, 1] x R."""
    rng = np.random.RandomState(1000 + 13 * n + seed)
    t = np.sort(rng.rand(n)) + 0.05
    s = R * 10.0 ** rng.uniform(-2.0, 0.0, n)
    y = np.sin(np.pi * t) + np.sin(2 * np.pi * t) + np.cos(3 * np.pi * t) + np.sqrt(R + s) * rng.randn(n)
    if n >= 10:
        y[rng.rand(n) < missing] = np.nan
        y[n // 2] = 0.3                                             # (never all missing)
    if run is not None:
        y[run[0]:run[0] + run[1]] = np.nan
    return t, y, s


def spaced_series(n, spacing, seed=0):
    """Sorted times with steps `spacing` (a scalar or (n,)) x U(0.5, 1.5): at spacing 0.05 thousands of rows span hundreds of
    lengthscales, which series() -- n rows packed into [0, 1] -- never does.  Two slow sines plus noise of variance R + s, s
    log-uniform over two decades [0.01, 1] x R, 20 % of the rows NaN."""
    rng = np.random.RandomState(4000 + n + seed)
    t = 0.05 + np.cumsum(spacing * rng.uniform(0.5, 1.5, n))
    s = R * 10.0 ** rng.uniform(-2.0, 0.0, n)
    y = np.sin(0.7 * t) + 0.5 * np.sin(0.13 * t + 1.0) + np.sqrt(R + s) * rng.randn(n)
    y[rng.rand(n) < 0.2] = np.nan
    y[n // 2] = 0.3
    return t, y, s


def workgroup_forgetting(sde, t, y, Rk, span, ssm=None):
    """(blocks, 2): per block of `span` consecutive steps, log2 max |A| and log2 max |E| of the block's total in the parallel
    scans -- what the device compares with 2^-120 before it takes a neighbour's record for the whole carry.
      A  the product of (I - K_k h^T) F_k over the block, K_k the gains of a filter started at the block's first step with
         P = 0: the derivative of the filtered mean at the block's end with respect to the mean handed to the block;
      E  the product G_a G_a+1 ... of the RTS smoother's gains over the block (filter from the start of the series; the last
         step of the series has no gain: E = 0 there, -inf here).
    These are properties of the data.  The device's total of the FIRST block has A = 0 exactly instead (its first element
    carries the prior), as its total of the last block has E = 0.
    Both products are renormalised at every step, so hundreds of binades do not underflow.  Rk scalar or (n,); NaN rows of y
    carry no observation."""
    t, y = (np.asarray(a, np.float64).reshape(-1) for a in (t, y))
    Rk = np.broadcast_to(np.asarray(Rk, np.float64), t.shape)
    P0, Fs, Qs, H, _ = O.get_ssm(sde, t, 1.0) if ssm is None else ssm
    h = H.reshape(-1)
    n, d = t.size, h.size
    seen = ~np.isnan(y)

    def update(P, k):
        """(I - K h^T, filtered P) of step k from its predicted P"""
        if not seen[k]:
            return np.eye(d), P
        u = P @ h
        S = float(h @ u) + Rk[k]
        P = P - np.outer(u, u) / S
        return np.eye(d) - np.outer(u / S, h), 0.5 * (P + P.T)

    def scaled(M, log):
        top = float(np.max(np.abs(M)))
        return (M, -np.inf) if top == 0.0 else (M / top, log + math.log2(top))

    G = np.zeros((n, d, d))
    P = P0.copy()
    for k in range(n):
        if k > 0:
            FP = Fs[k] @ P
            pP = FP @ Fs[k].T + Qs[k]
            G[k - 1] = np.linalg.solve(0.5 * (pP + pP.T), FP).T
            P = 0.5 * (pP + pP.T)
        else:
            P = Fs[0] @ P @ Fs[0].T + Qs[0]
        P = update(P, k)[1]
    out = np.empty(((n + span - 1) // span, 2))
    for b in range(out.shape[0]):
        A, E, la, le = np.eye(d), np.eye(d), 0.0, 0.0
        P = np.zeros((d, d))
        for k in range(b * span, min(n, (b + 1) * span)):
            P = Fs[k] @ P @ Fs[k].T + Qs[k]
            IKh, P = update(0.5 * (P + P.T), k)
            if la > -np.inf:
                A, la = scaled(IKh @ Fs[k] @ A, la)
            if le > -np.inf:
                E, le = scaled(E @ G[k], le)
        out[b] = la, le
    return out


def queries(t, k, seed=0):
    """k sorted queries: before the first training time, after the last, ties on training times (from k >= 4 on)."""
    rng = np.random.RandomState(77 + k + seed)
    tq = rng.uniform(t[0], t[-1], k)
    if k >= 4:
        tq[0], tq[1] = t[0] - 0.07, t[-1] + 0.11
        nt = min(k // 4, t.size)
        tq[2:2 + nt] = t[rng.choice(t.size, nt, replace=False)]
    return np.sort(tq)


@functools.lru_cache(maxsize=None)
def sde_of(kname):
    return matern(kname).get_sde()


def rel(a, b):
    """Max-norm error relative to the largest entry (the project's, tests/test_gpu_multi_grad.py)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))
