"""What tests/test_panel_fit_host.py and tests/test_gpu_panel_fit.py share: the seeded series of the fit tests, the oracle's
objective (oracle.np_grad's log-likelihood and adjoints, contracted for a single Matern kernel), and the measures both assert
on (the projected gradient in x = log theta, the Hessian of f in x by central differences of a gradient).  No GPU here."""
import numpy as np

from oracle import np_grad as G
from pssgp.forms import matern_closed_forms
from pssgp.gradients import matern_contract
from pssgp.kernels import Matern12, Matern32, Matern52
from pssgp.model import StateSpaceGP

KERNELS = {"Matern12": Matern12, "Matern32": Matern32, "Matern52": Matern52}
START = (1.0, 1.0, 1.0)                 # variance, lengthscales, noise_variance
NAMES = ["variance", "lengthscales", "noise_variance"]
R_TRUE = 0.1
GTOL = 1e-6
MAX_ITER = 60


def series(n, seed, nan_only=False):
    """Sorted times at about 12 rows per unit of time (at least 3 units), two sines plus noise of variance R_TRUE + s with given
    variances s, 10 % of the rows NaN from 10 rows on (never the middle one); nan_only: every row NaN."""
    rng = np.random.RandomState(7000 + 13 * n + seed)
    t = np.sort(rng.rand(n)) * max(3.0, n / 12.0) + 0.05
    s = R_TRUE * 10.0 ** rng.uniform(-2.0, 0.0, n)
    y = np.sin(2.0 * t) + 0.5 * np.sin(0.7 * t + 1.0) + np.sqrt(R_TRUE + s) * rng.randn(n)
    if n >= 10:
        y[rng.rand(n) < 0.1] = np.nan
        y[n // 2] = 0.3
    if nan_only:
        y[:] = np.nan
    return t, y, s


def unit52():
    """(P1, H1, N, N^2 / 2) of the Matern-5/2 SDE at lam = 1, variance 1, as the model keeps it."""
    m = StateSpaceGP((np.zeros((1, 1)), np.zeros((1, 1))), Matern52(variance=1.0, lengthscales=1.0), noise_variance=0.1)
    assert m._matern_forms() is not None
    return m._matern52_unit


def oracle_ll_and_grad(name, theta, t, y, s=None, unit=None):
    """(ll, d ll / d theta) of one series at theta = (variance, lengthscales, noise_variance) from oracle.np_grad (the filter
    starts at the series' own first time, as the panel's does).  With given variances s the oracle's scalar-noise sweep does
    not apply: None."""
    assert s is None
    lam, N1, _, Pinf, H = matern_closed_forms(name, float(theta[0]), float(theta[1]), unit)
    d = len(Pinf)
    Pinf, H = np.array(Pinf, np.float64), np.array(H, np.float64).reshape(-1)
    F = (np.zeros((d, d)) if N1 is None else np.array(N1, np.float64)) - lam * np.eye(d)
    ll, Abar, Ubar, _, Rbar = G.ll_grad_stats(F, Pinf, H, float(theta[2]), t, y, t0=float(t[0]))
    return ll, matern_contract(Abar.reshape(-1), Ubar, Rbar, F.reshape(-1), Pinf @ H, NAMES, float(theta[1]), float(theta[0]))


def objective(lls_and_grads, thetas, n_obs, free):
    """(f, g) in x = log theta of (lls, grads) = lls_and_grads(thetas): f = -ll / max(1, n_obs), g = -theta grad / max(1, n_obs)
    at the free coordinates, 0 elsewhere."""
    lls, grads = lls_and_grads(thetas)
    scale = np.maximum(1.0, np.asarray(n_obs, np.float64))
    return -np.asarray(lls) / scale, np.where(np.asarray(free, bool)[None, :], -(thetas * grads) / scale[:, None], 0.0)


def projected_gradient_norm(g, thetas, lo, hi):
    """max |q| per row: g with the components that point out of the box at a bound set to 0 (a theta ON a bound is the bound bit
    for bit, so the comparison is made in theta)."""
    pinned = ((thetas <= lo) & (g > 0.0)) | ((thetas >= hi) & (g < 0.0))
    return np.max(np.abs(np.where(pinned, 0.0, g)), axis=1)


def hessian_min_eigenvalues(lls_and_grads, thetas, n_obs, free, step=1e-4):
    """The smallest eigenvalue, per row, of the Hessian of f in x = log theta at `thetas`, restricted to the free coordinates, by
    central differences (step in x) of the gradient g."""
    S, P = thetas.shape
    idx = [i for i in range(P) if free[i]]
    Hs = np.zeros((S, len(idx), len(idx)))
    for a, i in enumerate(idx):
        up, dn = thetas.copy(), thetas.copy()
        up[:, i] *= np.exp(step)
        dn[:, i] *= np.exp(-step)
        gu, gd = objective(lls_and_grads, up, n_obs, free)[1], objective(lls_and_grads, dn, n_obs, free)[1]
        Hs[:, a, :] = (gu - gd)[:, idx] / (2.0 * step)
    Hs = 0.5 * (Hs + np.transpose(Hs, (0, 2, 1)))
    return np.array([np.linalg.eigvalsh(h)[0] for h in Hs])
