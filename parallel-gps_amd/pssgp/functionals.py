"""The posterior of linear functionals of the state: additive components and derivatives of f (a mixin of the one class,
beside forms.py, gradients.py, batches.py, checks.py and trend.py).

predict_f returns the law of f = H x, the sum of everything in the kernel.  The smoother carries the whole state at every
query step, and two things are linear functionals c x of it:

  additive components   a sum kernel has a block-diagonal SDE and H = [H_1 .. H_J]: part j alone is c_j x with c_j = H
                        restricted to block j's columns (kernel.component_functionals());
  derivatives           f^(n) = H F^n x wherever H F^j L = 0 for all j < n (kernel.derivative_functional(n)).

Both are  mean = C sm,  cov = C sP C^T  at the query rows for a small C (J, d).  parallel=True, sorted training times,
2 <= d <= 32 and J <= 8: one device call (_backend.lti_predict_lin -- merge, discretisation, filter + smoother, the J means
and the (J, J) block of every query, nothing else leaves the device).  Everything else -- parallel=False, times out of
order, d = 1, more rows -- is the host twin: _host_smoothed and the two products in numpy, any kernel, no device.
"""
import numpy as np

from . import _backend, config


class ModelFunctionals:
    """predict_functionals, predict_components, component_names, predict_f_derivative.  Single-output models with one shared
    noise variance and no mean function."""

    def _functionals_model(self, name):
        if self.num_latent_gps > 1:
            raise NotImplementedError(f"{name} covers single-output models; this one has {self.num_latent_gps} output columns")
        if self._obs_var is not None:
            raise NotImplementedError(f"{name} is not available with observation_variances set")
        if self._mean_function is not None:
            raise NotImplementedError(f"{name} is not available with a mean_function set")

    def _host_smoothed_any_order(self, tq):
        """(sms, sPs, flags) of _host_smoothed; training times out of order are sorted for it (stable) in a local copy, as
        the predictive checks sort theirs -- the query rows' moments do not depend on the order the data were given in."""
        ts, ys = self.data
        if ts.shape[0] < 1:
            raise ValueError("the functionals of the state need at least one data row")
        data = None
        if not self._ts_sorted():
            order = np.argsort(ts.reshape(-1), kind="stable")
            data = (ts[order], ys[order])
        _, _, _, sms, sPs, _, flags = self._host_smoothed(tq, data)
        return sms, sPs, flags

    def _functionals(self, Xnew, C):
        """(mean (K, J), cov (K, J, J)) of C x at Xnew in fp64, rows in the order of Xnew (any order, repeats allowed)."""
        sde = self.kernel.get_sde()
        d = np.asarray(sde.F).shape[0]
        C = np.asarray(C, np.float64)
        if C.ndim == 1:
            C = C[None, :]
        if C.ndim != 2 or C.shape[0] < 1 or C.shape[1] != d:
            raise ValueError(f"C must be (J, {d}) with J >= 1 -- rows over the state of kernel.get_sde() -- got shape {C.shape}")
        J = C.shape[0]
        xq = np.asarray(Xnew, dtype=np.float64).reshape(-1)
        if xq.size == 0:
            return np.zeros((0, J)), np.zeros((0, J, J))
        tq, inverse = np.unique(xq, return_inverse=True)          # sorted, each time once
        ts, ys = self.data
        device = (self.parallel and self._ts_sorted() and _backend.LTI_DIM_MIN <= d <= _backend.LTI_DIM_MAX
                  and J <= _backend.LTI_FUNCTIONALS_MAX)
        if device:
            mean, cov, _ = _backend.lti_predict_lin(sde.F, sde.P0, sde.H, C, self.noise_variance,
                                                    np.asarray(ts, np.float64).reshape(-1),
                                                    np.asarray(ys, np.float64).reshape(-1), tq)
        else:
            sms, sPs, flags = self._host_smoothed_any_order(tq)
            mean = sms[flags] @ C.T
            cov = np.einsum("ia,nab,jb->nij", C, sPs[flags], C)
            cov = 0.5 * (cov + np.swapaxes(cov, 1, 2))
        return mean[inverse], cov[inverse]

    def predict_functionals(self, Xnew, C):
        """Posterior mean (K, J) and covariance (K, J, J) of the J linear functionals C x(t) of the state at every time of
        Xnew, C (J, d) in the coordinates of kernel.get_sde().  Every (J, J) block is symmetric bit for bit; no covariance
        ACROSS query times is returned.  Computed in fp64 and rounded to the default float.  Any order of Xnew; equal times
        give equal rows."""
        self._functionals_model("predict_functionals")
        dtype = config.default_float()
        mean, cov = self._functionals(Xnew, C)
        return mean.astype(dtype), cov.astype(dtype)

    def component_names(self):
        """The names of predict_components' J columns: kernel.component_functionals()[0]."""
        return list(self.kernel.component_functionals()[0])

    def predict_components(self, Xnew, cross_cov=False):
        """The posterior of every additive part of the kernel at Xnew: mean (K, J) and var (K, J) -- with cross_cov=True the
        (K, J, J) covariance BETWEEN the parts at each time.  The means sum to predict_f's mean and 1^T cov 1 is its
        variance; any subset sum a (0 / 1 entries) has mean a^T mean and variance a^T cov a.  A kernel that is no sum is one
        part (J = 1: predict_f)."""
        self._functionals_model("predict_components")
        dtype = config.default_float()
        mean, cov = self._functionals(Xnew, self.kernel.component_functionals()[1])
        if cross_cov:
            return mean.astype(dtype), cov.astype(dtype)
        return mean.astype(dtype), np.diagonal(cov, axis1=1, axis2=2).astype(dtype)

    def predict_f_derivative(self, Xnew, order=1):
        """Posterior mean (K, 1) and variance (K, 1) of the `order`-th mean-square derivative of f at Xnew; ValueError where
        the kernel is not that many times differentiable (kernel.derivative_functional)."""
        self._functionals_model("predict_f_derivative")
        dtype = config.default_float()
        mean, cov = self._functionals(Xnew, self.kernel.derivative_functional(order)[None, :])
        return mean.astype(dtype), cov[:, :, 0].astype(dtype)
