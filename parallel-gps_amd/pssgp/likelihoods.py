"""Observation likelihoods of LaplaceStateSpaceGP (pssgp/laplace.py): y_k ~ p(y | f(t_k)), log-concave in f.

Each class carries the id and the parameter the device kernels take (csrc/pgps_lik.h holds the same formulas), the numpy twin
log_prob_derivs(y, f) -> (lp, g, W, d3) with lp = log p, g = d lp / d f, W = -d^2 lp / d f^2 floored at W_MIN, d3 = d^3 lp / d f^3,
the check of the observations, and the predictive law of a NEW observation under a Gaussian law N(m, v) of f.
"""
import numpy as np
from scipy.special import gammaln

from ._backend.sites import LIK_BERNOULLI_LOGIT, LIK_GAUSSIAN, LIK_POISSON_EXP, LIK_W_MIN

W_MIN = LIK_W_MIN
_GH_X, _GH_W = np.polynomial.hermite.hermgauss(32)
_GH_W = _GH_W / np.sqrt(np.pi)


def _gauss_hermite(fn, m, v):
    """E[fn(f)] under f ~ N(m, v), elementwise in (m, v): 32-point Gauss-Hermite quadrature."""
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    f = m[..., None] + np.sqrt(2.0 * np.maximum(v, 0.0))[..., None] * _GH_X
    return np.sum(fn(f) * _GH_W, axis=-1)


def _log_gauss_hermite(logfn, m, v):
    """log E[exp(logfn(f))] under f ~ N(m, v): the same nodes, summed in the log domain."""
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    f = m[..., None] + np.sqrt(2.0 * np.maximum(v, 0.0))[..., None] * _GH_X
    a = logfn(f) + np.log(_GH_W)
    top = np.max(a, axis=-1, keepdims=True)
    return top[..., 0] + np.log(np.sum(np.exp(a - top), axis=-1))


class Likelihood:
    lik_id = None
    name = "likelihood"

    @property
    def par(self):
        return 1.0

    def validate(self, y):
        """Raises ValueError unless every entry of y is a value the likelihood can produce, or NaN (a missing row)."""

    def log_prob_derivs(self, y, f):
        raise NotImplementedError

    def log_prob_constant(self, y):
        """What log_prob_derivs' lp leaves out: a sum over the observed rows that does not depend on f."""
        return 0.0

    def log_prob(self, y, f):
        return self.log_prob_derivs(y, f)[0]

    def predict_log_density(self, m, v, y):
        """log of E[p(y | f)] under f ~ N(m, v), elementwise; NaN where y is."""
        y = np.asarray(y, np.float64)
        y0 = np.where(np.isnan(y), self._any_valid, y)
        out = _log_gauss_hermite(lambda f: self._log_prob_full(y0[..., None], f), m, v)
        return np.where(np.isnan(y), np.nan, out)


class Gaussian(Likelihood):
    """y ~ N(f, variance): the model of StateSpaceGP, here for cross-checks (one Newton step from f = 0 is exact)."""
    lik_id = LIK_GAUSSIAN
    name = "Gaussian"
    _any_valid = 0.0

    def __init__(self, variance=1.0):
        if not (np.isfinite(variance) and variance > 0.0):
            raise ValueError(f"the Gaussian likelihood needs variance > 0, got {variance}")
        self.variance = float(variance)

    @property
    def par(self):
        return self.variance

    def log_prob_derivs(self, y, f):
        y, f = np.asarray(y, np.float64), np.asarray(f, np.float64)
        r = y - f
        g = r / self.variance
        W = np.full(np.broadcast(y, f).shape, max(1.0 / self.variance, W_MIN))
        return -0.5 * (np.log(2.0 * np.pi * self.variance) + r * g), g, W, np.zeros_like(W)

    def _log_prob_full(self, y, f):
        return self.log_prob_derivs(y, f)[0]

    def predict_mean_and_var(self, m, v):
        m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
        return m.copy(), v + self.variance

    def predict_log_density(self, m, v, y):
        m, v, y = (np.asarray(a, np.float64) for a in (m, v, y))
        s = v + self.variance
        return -0.5 * (np.log(2.0 * np.pi * s) + (y - m) ** 2 / s)


class Bernoulli(Likelihood):
    """y in {0, 1}, p(y = 1 | f) = 1 / (1 + exp(-f)) (the logit link)."""
    lik_id = LIK_BERNOULLI_LOGIT
    name = "Bernoulli"
    _any_valid = 0.0

    def validate(self, y):
        y = np.asarray(y, np.float64)
        seen = y[~np.isnan(y)]
        if not np.all((seen == 0.0) | (seen == 1.0)):
            raise ValueError("Bernoulli observations must be 0, 1 or NaN")

    def log_prob_derivs(self, y, f):
        y, f = np.asarray(y, np.float64), np.asarray(f, np.float64)
        a = (2.0 * y - 1.0) * f
        lp = -(np.maximum(-a, 0.0) + np.log1p(np.exp(-np.abs(a))))          # -softplus(-a)
        e = np.exp(-np.abs(f))
        r = 1.0 / (1.0 + e)
        p = np.where(f >= 0.0, r, e * r)
        W = e * r * r                                                       # p (1 - p)
        d3 = W * np.where(f >= 0.0, 1.0, -1.0) * (1.0 - e) * r              # -W (1 - 2 p)
        return lp, y - p, np.maximum(W, W_MIN), d3

    def _log_prob_full(self, y, f):
        return self.log_prob_derivs(y, f)[0]

    def predict_mean_and_var(self, m, v):
        """E[y] = E[sigmoid(f)] by quadrature; Var[y] = p (1 - p) of a 0 / 1 variable."""
        p = _gauss_hermite(lambda f: 1.0 / (1.0 + np.exp(-f)), m, v)
        return p, p * (1.0 - p)


class Poisson(Likelihood):
    """y ~ Poisson(exposure exp(f)) (the log link); lp of log_prob_derivs leaves out -lgamma(y + 1)."""
    lik_id = LIK_POISSON_EXP
    name = "Poisson"
    _any_valid = 0.0

    def __init__(self, exposure=1.0):
        if not (np.isfinite(exposure) and exposure > 0.0):
            raise ValueError(f"the Poisson likelihood needs exposure > 0, got {exposure}")
        self.exposure = float(exposure)

    @property
    def par(self):
        return self.exposure

    def validate(self, y):
        y = np.asarray(y, np.float64)
        seen = y[~np.isnan(y)]
        if not (np.all(np.isfinite(seen)) and np.all(seen >= 0.0) and np.all(seen == np.floor(seen))):
            raise ValueError("Poisson observations must be non-negative integer values or NaN")

    def log_prob_derivs(self, y, f):
        y, f = np.asarray(y, np.float64), np.asarray(f, np.float64)
        rate = self.exposure * np.exp(f)
        return y * (f + np.log(self.exposure)) - rate, y - rate, np.maximum(rate, W_MIN), -rate

    def log_prob_constant(self, y):
        y = np.asarray(y, np.float64)
        return -float(np.sum(gammaln(y[~np.isnan(y)] + 1.0)))

    def _log_prob_full(self, y, f):
        return self.log_prob_derivs(y, f)[0] - gammaln(y + 1.0)

    def predict_mean_and_var(self, m, v):
        """Closed form (the log-normal moments of the rate): E[y] = E[rate], Var[y] = E[rate] + Var[rate]."""
        m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
        mean = self.exposure * np.exp(m + 0.5 * v)
        return mean, mean + mean * mean * np.expm1(v)
