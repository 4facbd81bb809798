"""Mean functions m(t) = Phi(t) beta with explicit basis functions (Rasmussen & Williams, section 2.7): what
StateSpaceGP(..., mean_function=...) takes.

Every mean function has `design(t) -> (n, p)` in float64 -- the basis functions at the times t -- and `beta` (p,), a plain
settable float64 array, initially zeros; `mf(t) = design(t) @ beta`.  The coefficients are linear parameters: the model
estimates them exactly (StateSpaceGP.mean_coefficients / fit_mean_function), integrates them out under a flat prior
(log_marginal_likelihood_flat_mean, predict_f_gls) or trains them with the kernel (trainable_parameters).
"""
import numpy as np


class MeanFunction:
    """Base: a subclass sets `num_functions` (p) before calling this constructor and implements `_design(t (n,)) -> (n, p)`."""

    num_functions = 0

    def __init__(self):
        self._beta = np.zeros(self.num_functions, np.float64)

    @property
    def beta(self):
        return self._beta

    @beta.setter
    def beta(self, value):
        b = np.array(value, dtype=np.float64).reshape(-1)
        if b.shape[0] != self.num_functions:
            raise ValueError(f"beta must have {self.num_functions} entries, got shape {np.shape(value)}")
        self._beta = b

    def design(self, t):
        """Phi (n, p), float64, at the times t (any shape: flattened)."""
        t = np.asarray(t, np.float64).reshape(-1)
        Phi = np.asarray(self._design(t), np.float64)
        if Phi.shape != (t.shape[0], self.num_functions):
            raise ValueError(f"the design matrix must have shape ({t.shape[0]}, {self.num_functions}), got {Phi.shape}")
        return np.ascontiguousarray(Phi)

    def __call__(self, t):
        return self.design(t) @ self._beta

    def _design(self, t):
        raise NotImplementedError


class Polynomial(MeanFunction):
    """1, u, .., u^degree in u = (t - center) / scale: centre and scale the times of a long record, or the powers are
    nearly collinear and the normal equations ill-conditioned."""

    def __init__(self, degree, center=0.0, scale=1.0):
        degree = int(degree)
        if degree < 0:
            raise ValueError(f"degree must be >= 0, got {degree}")
        if float(scale) == 0.0:
            raise ValueError("scale must not be 0")
        self.degree, self.center, self.scale = degree, float(center), float(scale)
        self.num_functions = degree + 1
        super().__init__()

    def _design(self, t):
        u = (t - self.center) / self.scale
        return u[:, None] ** np.arange(self.degree + 1)[None, :]


class Constant(Polynomial):
    """m(t) = beta_0."""

    def __init__(self):
        super().__init__(0)


class Linear(Polynomial):
    """m(t) = beta_0 + beta_1 t."""

    def __init__(self):
        super().__init__(1)


class Basis(MeanFunction):
    """A user's basis: fn(t (n,)) -> (n, num_functions)."""

    def __init__(self, fn, num_functions):
        if int(num_functions) < 1:
            raise ValueError(f"num_functions must be >= 1, got {num_functions}")
        self.fn, self.num_functions = fn, int(num_functions)
        super().__init__()

    def _design(self, t):
        return self.fn(t)
