"""References and data of the Laplace-inference tests (test_laplace_host.py, test_gpu_laplace.py).  None
of this is the code under test:
  lik_derivs      numpy formulas of (lp, g, W, d3) of the three likelihoods, written from the textbook forms (not the stable
                  ones of csrc/pgps_lik.h and pssgp/likelihoods.py);
  dense_laplace   Rasmussen & Williams Algorithm 3.1 in dense algebra over the observed rows, with the damping on the (f, alpha)
                  segment, the evidence by eq. 3.32, and the gradient by section 5.5.1 (dense_gradient);
  ss_newton       ONE Newton pass in state-space form: a numpy Kalman filter with a per-step variance + RTS smoother (as
                  het_refs.ss_het / loo_refs.ss_checks run them) over given sites, then the site update and the six sums.
"""
import functools
import math

import numpy as np
from scipy.special import gammaln

from het_refs import MATERNS, matern, rel, sde_of, series, spaced_series  # noqa: F401  (re-exported to the tests)
from oracle import np_oracle as O

LOG2PI = math.log(2.0 * math.pi)
W_MIN = 1e-10                   # kLikWMin of csrc/pgps_lik.h
TOL = 1e-9                      # the project's: max norm relative to the largest entry
LIKS = {"gaussian": 0, "bernoulli": 1, "poisson": 2}            # PGPS_LIK_*
ARRAYS = ("f", "v", "alpha", "zs", "ss")


def lik_derivs(lik, par, y, f):
    """(lp, g, W, d3) elementwise; Poisson's lp leaves out -lgamma(y + 1) (lik_constant), W is floored at W_MIN."""
    y, f = np.asarray(y, np.float64), np.asarray(f, np.float64)
    if lik == "bernoulli":
        p = 1.0 / (1.0 + np.exp(-f))
        lp = y * f - np.logaddexp(0.0, f)
        g, W = y - p, p * (1.0 - p)
        d3 = -W * (1.0 - 2.0 * p)
    elif lik == "poisson":
        rate = par * np.exp(f)
        lp, g, W, d3 = y * (f + math.log(par)) - rate, y - rate, rate, -rate
    else:
        lp = -0.5 * (LOG2PI + math.log(par)) - 0.5 * (y - f) ** 2 / par
        g, W, d3 = (y - f) / par, np.full(np.broadcast(y, f).shape, 1.0 / par), np.zeros(np.broadcast(y, f).shape)
    return lp, g, np.maximum(W, W_MIN), d3


def lik_constant(lik, y):
    y = np.asarray(y, np.float64)
    return -float(np.sum(gammaln(y[~np.isnan(y)] + 1.0))) if lik == "poisson" else 0.0


def sites_at(lik, par, y, f):
    """(z, s, lp sum, correction sum) of the sites formed at f: z NaN and s = 1 at the NaN rows of y."""
    obs = ~np.isnan(y)
    lp, g, W, _ = lik_derivs(lik, par, np.where(obs, y, 0.0), f)
    s = np.where(obs, 1.0 / W, 1.0)
    z = np.where(obs, f + g / W, np.nan)
    logn = -0.5 * (LOG2PI + np.log(s)) - 0.5 * (np.where(obs, z, 0.0) - f) ** 2 / s
    return z, s, float(np.sum(lp[obs])), float(np.sum((lp - logn)[obs]))


# ---- dense algebra ------------------------------------------------------------------------------------------------------
def matern_K(kname, variance, ell, x1, x2, grad=False):
    """The Matern covariance (and with grad: [dK / d variance, dK / d lengthscale]) -- O.dense_K's formulas with derivatives."""
    dist = np.abs(np.asarray(x1, np.float64)[:, None] - np.asarray(x2, np.float64)[None, :])
    if kname == "m12":
        r = dist / ell
        K, dKdr = np.exp(-r), -np.exp(-r)
    elif kname == "m32":
        r = math.sqrt(3.0) * dist / ell
        K, dKdr = (1.0 + r) * np.exp(-r), -r * np.exp(-r)
    else:
        r = math.sqrt(5.0) * dist / ell
        K, dKdr = (1.0 + r + r * r / 3.0) * np.exp(-r), -(r / 3.0) * (1.0 + r) * np.exp(-r)
    if not grad:
        return variance * K
    return variance * K, [K, variance * dKdr * (-r / ell)]


def dense_laplace(K, y, lik, par, tol=1e-11, damp=True, max_iter=200):
    """R&W Algorithm 3.1 on the OBSERVED rows (K, y dense over them), damped on the (f, alpha) segment: step 1, 1/2, ... until
    Psi = sum lp - f^T alpha / 2 is finite and not below the old one (less 1e-12 of it); 20 halvings at the most.  Returns a
    dict: f, alpha, v (posterior variances), W, d3, z, s, evidence (eq. 3.32, lik_constant included), iterations, halvings,
    diverged."""
    n = y.size
    f, a = np.zeros(n), np.zeros(n)
    psi = float(np.sum(lik_derivs(lik, par, y, f)[0]))
    out = {"iterations": 0, "halvings": 0, "diverged": False}
    with np.errstate(over="ignore", invalid="ignore"):
        for it in range(max_iter):
            _, g, W, _ = lik_derivs(lik, par, y, f)
            sw = np.sqrt(W)
            L = np.linalg.cholesky(np.eye(n) + sw[:, None] * K * sw[None, :])
            b = W * f + g
            a_new = b - sw * np.linalg.solve(L.T, np.linalg.solve(L, sw * (K @ b)))
            f_new = K @ a_new
            move = float(np.max(np.abs(f_new - f)))
            step, halvings = 1.0, 0
            while True:
                f2, a2 = f + step * (f_new - f), a + step * (a_new - a)
                psi2 = float(np.sum(lik_derivs(lik, par, y, f2)[0]) - 0.5 * f2 @ a2)
                if not damp or (np.isfinite(psi2) and psi2 >= psi - 1e-12 * abs(psi)) or halvings >= 20:
                    break
                step, halvings = 0.5 * step, halvings + 1
            f, a, psi = f2, a2, psi2
            out["iterations"], out["halvings"] = it + 1, out["halvings"] + halvings
            if not np.all(np.isfinite(f)) or not np.isfinite(psi):
                out["diverged"] = True
                return out
            if move <= tol:
                break
    lp, g, W, d3 = lik_derivs(lik, par, y, f)
    sw = np.sqrt(W)
    B = np.eye(n) + sw[:, None] * K * sw[None, :]
    L = np.linalg.cholesky(B)
    V = np.linalg.solve(L, sw[:, None] * K)
    out.update(f=f, alpha=a, W=W, d3=d3, g=g, s=1.0 / W, z=f + g / W, v=np.diag(K) - np.sum(V * V, axis=0),
               evidence=float(np.sum(lp) - 0.5 * f @ a - np.sum(np.log(np.diag(L)))) + lik_constant(lik, y))
    return out


def dense_gradient(K, dKs, fit):
    """d log q / d theta_j for the derivatives dKs of K (R&W eq. 5.21 - 5.24): the explicit part at a fixed mode and the implicit
    part through it, dlogq / df_i = v_i d3_i / 2 (the sign from differences: test_laplace_host.py)."""
    f, a, W, d3, g, v = (fit[k] for k in ("f", "alpha", "W", "d3", "g", "v"))
    n = f.size
    sw = np.sqrt(W)
    B = np.eye(n) + sw[:, None] * K * sw[None, :]
    R = sw[:, None] * np.linalg.solve(B, np.diag(sw))               # (K + W^-1)^-1
    dq_df = 0.5 * v * d3
    out = []
    for C in dKs:
        explicit = 0.5 * a @ C @ a - 0.5 * np.trace(R @ C)
        b = C @ g
        out.append(float(explicit + dq_df @ (b - K @ (R @ b))))
    return np.array(out)


def dense_fit(kname, variance, ell, t, y, lik, par, tol=1e-11, tq=None, grad=False):
    """dense_laplace on the observed rows of (t, y) with the mode and variance carried to EVERY row (and to tq) by the Gaussian
    predictive equations of the sites.  Returns the dict of dense_laplace plus f_all, v_all (N,), mean_q, var_q, gradient."""
    t, y = (np.asarray(a, np.float64).reshape(-1) for a in (t, y))
    o = ~np.isnan(y)
    if grad:
        K, dKs = matern_K(kname, variance, ell, t[o], t[o], grad=True)
    else:
        K = matern_K(kname, variance, ell, t[o], t[o])
    fit = dense_laplace(K, y[o], lik, par, tol=tol)
    C = K + np.diag(fit["s"])

    def predict(x):
        Kx = matern_K(kname, variance, ell, t[o], x)
        return Kx.T @ fit["alpha"], variance - np.sum(Kx * np.linalg.solve(C, Kx), axis=0)

    fit["f_all"], fit["v_all"] = predict(t)
    if tq is not None:
        fit["mean_q"], fit["var_q"] = predict(np.asarray(tq, np.float64).reshape(-1))
    if grad:
        fit["gradient"] = dense_gradient(K, dKs, fit)
    return fit


# ---- one Newton pass in state-space form ------------------------------------------------------------------------------------
def ss_newton(sde, t, y, z, s, f_prev, lik, par, ssm=None):
    """dict of ARRAYS (N,) and "sums" (6,): Kalman filter over the sites (z, s) with R = 0 (NaN rows of z carry none), RTS
    smoother, f = H x smoothed, alpha = (z - f) / s, the sites at f, the sums of pgps_gp_newton_f64."""
    t, y, z, s = (np.asarray(a, np.float64).reshape(-1) for a in (t, y, z, s))
    P0, Fs, Qs, H, _ = O.get_ssm(sde, t, 1.0) if ssm is None else ssm
    h = H.reshape(-1)
    n, d = t.size, h.size
    m, P, ll = np.zeros(d), P0.copy(), 0.0
    fm, fP, pm, pP = np.empty((n, d)), np.empty((n, d, d)), np.empty((n, d)), np.empty((n, d, d))
    for k in range(n):
        m = Fs[k] @ m
        P = Fs[k] @ P @ Fs[k].T + Qs[k]
        P = 0.5 * (P + P.T)
        pm[k], pP[k] = m, P
        if not np.isnan(z[k]):
            S = float(h @ P @ h) + s[k]
            r = z[k] - float(h @ m)
            ll += -0.5 * (LOG2PI + math.log(S) + r * r / S)
            u = P @ h
            m = m + u * (r / S)
            P = P - np.outer(u, u) / S
            P = 0.5 * (P + P.T)
        fm[k], fP[k] = m, P
    sm, sP = fm.copy(), fP.copy()
    for k in range(n - 2, -1, -1):
        G = np.linalg.solve(pP[k + 1], Fs[k + 1] @ fP[k]).T
        sm[k] = fm[k] + G @ (sm[k + 1] - pm[k + 1])
        sP[k] = fP[k] + G @ (sP[k + 1] - pP[k + 1]) @ G.T
    f, v = sm @ h, np.einsum("i,nij,j->n", h, sP, h)
    obs = ~np.isnan(y)
    alpha = np.where(obs, (np.where(obs, z, 0.0) - f) / s, 0.0)
    z_new, s_new, lp, corr = sites_at(lik, par, y, f)
    move = 0.0 if f_prev is None else float(np.max(np.abs(f - f_prev)))
    return {"f": f, "v": v, "alpha": alpha, "zs": z_new, "ss": s_new,
            "sums": np.array([ll, lp, float(f @ alpha), corr, move, float(obs.sum())])}


# ---- data -------------------------------------------------------------------------------------------------------------------
def observations(lik, t, nan, seed=0, spaced=False):
    """Draws of the likelihood under a smooth latent function of t; NaN where `nan` is True."""
    rng = np.random.RandomState(500 + t.size + seed)
    latent = (np.sin(0.7 * t) + 0.5 * np.sin(0.13 * t + 1.0)) if spaced else (np.sin(np.pi * t) + np.sin(2 * np.pi * t))
    if lik == "bernoulli":
        y = (rng.rand(t.size) < 1.0 / (1.0 + np.exp(-2.0 * latent))).astype(np.float64)
    elif lik == "poisson":
        y = rng.poisson(2.0 * np.exp(latent)).astype(np.float64)
    else:
        y = latent + 0.3 * rng.randn(t.size)
    y[nan] = np.nan
    return y


PARS = {"gaussian": 0.09, "bernoulli": 0.0, "poisson": 1.5}


@functools.lru_cache(maxsize=None)
def case(lik, n, run=None, repeated=False, spaced=False):
    """(t, y) read-only: the times and the missing rows of the predictive-check tests' series (loo_refs.case), the observations
    drawn from `lik`."""
    if spaced:
        t, y0, _ = spaced_series(n, 0.05)
    else:
        import loo_refs
        t, y0, _ = loo_refs.case(n, run, repeated)
    y = observations(lik, np.asarray(t), np.isnan(y0), spaced=spaced)
    t = np.array(t)
    for a in (t, y):
        a.setflags(write=False)
    return t, y


@functools.lru_cache(maxsize=None)
def _ssm(kname, n, run, repeated, spaced):
    """O.get_ssm of a case's times: shared by the likelihoods (the times do not depend on them)."""
    return O.get_ssm(sde_of(kname), case("bernoulli", n, run, repeated, spaced)[0], 1.0)


@functools.lru_cache(maxsize=None)
def pass_case(kname, lik, n, run=None, repeated=False, spaced=False):
    """(t, y, z, s, f_prev, reference of one pass): the start sites are formed at f_prev = 0.3 sin(t).  Computed once, shared."""
    t, y = case(lik, n, run, repeated, spaced)
    f_prev = 0.3 * np.sin(t)
    z, s, _, _ = sites_at(lik, PARS[lik], y, f_prev)
    ref = ss_newton(sde_of(kname), t, y, z, s, f_prev, lik, PARS[lik], ssm=_ssm(kname, n, run, repeated, spaced))
    for a in (z, s, f_prev) + tuple(ref.values()):
        a.setflags(write=False)
    return t, y, z, s, f_prev, ref


def err(got, want):
    """rel() with NaN pattern checked first (zs is NaN at the missing rows); a reference with no entry above rel()'s floor is
    compared absolutely (loo_refs.err)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return np.inf
    keep = ~np.isnan(want)
    if not keep.any():
        return 0.0
    got, want = got[keep], want[keep]
    if float(np.max(np.abs(want))) < 1e-6:
        return float(np.max(np.abs(got - want)))
    return rel(got, want)
