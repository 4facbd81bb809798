"""Predictive checks of a fitted StateSpaceGP against its own data, and the predictive law of new observations
(a mixin of the one class, beside forms.py, gradients.py and batches.py).

Two laws of every training observation y_k come out of the passes the model makes anyway:

  one step ahead   y_k | y_1..k-1 ~ N(mu_k, S_k),  mu_k = H m_k^-,  S_k = H P_k^- H^T + R_k: the pair the Kalman pass hands to the
                   log-likelihood, so the log densities sum to maximum_log_likelihood_objective();
  leave one out    y_k | y_-k: with (m, v) the smoothed mean and variance of f(t_k) = H x_k given ALL data, removing the factor
                   N(y_k | f_k, R_k) gives  var = R_k^2 / (R_k - v),  mean = (m R_k - y_k v) / (R_k - v)
                   (Rasmussen & Williams section 5.4.2, eq. 5.10-5.12).

R_k = noise_variance (+ s_k with observation_variances set).  One filter and one smoother pass over the N training steps: no
merge, no query rows, no refit.  predict_y / predict_log_density are GPflow's methods over predict_f.
"""
import numpy as np

from . import _backend, config
from ._evaluation import _mean_function_route
from .kalman import sequential


def _loo_from_smoothed(m, v, Rk, y):
    """The leave-one-out law of y (N,) from the smoothed law (m, v) of f and the step variances Rk; at the NaN rows of y
    nothing is left out: (m, v + Rk)."""
    obs = ~np.isnan(y)
    y0 = np.where(obs, y, 0.0)
    gap = np.where(obs, Rk - v, 1.0)
    return np.where(obs, (m * Rk - y0 * v) / gap, m), np.where(obs, Rk * Rk / gap, v + Rk)


class ModelChecks:
    """one_step_ahead, leave_one_out, loo_log_predictive_density, predict_y, predict_log_density.  Single-output models."""

    def _single_output(self, name):
        if self.num_latent_gps > 1:
            raise NotImplementedError(f"{name} covers single-output models; this one has {self.num_latent_gps} output columns")

    def _step_variances(self):
        """R_k of every step (N,) in fp64, checked: positive wherever y is observed (leaving out a noise-free observation is
        undefined).  NaN where observation_variances is (its missing rows only)."""
        y = np.asarray(self.data[1], np.float64).reshape(-1)
        R = np.float64(self.noise_variance)
        if self._obs_var is None:
            if not R > 0.0:
                raise ValueError(f"the predictive checks need noise_variance > 0, got {self.noise_variance}")
            return np.full(y.shape, R)
        Rk = R + self._obs_var
        if not np.all(Rk[~np.isnan(y)] > 0.0):
            raise ValueError("the predictive checks need noise_variance + observation_variances > 0 wherever y is observed")
        return Rk

    def _checks(self, osa, loo):
        """The dict of _backend.gp_loo (arrays (N,), fp64, in the order of the data rows) on either route.  The fused route of
        the class docstring without observation_variances: _backend.gp_loo, never the resident series.  Everything else: the
        host twin in fp64 (_host_discretise, sequential.kf with the predicted moments, sequential.ks), any kernel, both modes;
        times out of order are sorted for it (stable) and the rows put back."""
        ts, ys = self.data
        Rk = self._step_variances()
        if ts.shape[0] < 1:
            raise ValueError("the predictive checks need at least one data row")
        fused = self._fused_route() if self._obs_var is None else None
        if fused is not None:
            sde, form = fused
            return _backend.gp_loo(form, sde.P0, sde.H, self.noise_variance, ts.reshape(-1), ys.reshape(-1), osa=osa, loo=loo)
        from .model import _host_discretise, _is_sorted
        t = np.asarray(ts, np.float64).reshape(-1)
        y = np.asarray(ys, np.float64).reshape(-1)
        order = None if _is_sorted(t) else np.argsort(t, kind="stable")
        if order is not None:
            t, y, Rk = t[order], y[order], Rk[order]
        sde = self.kernel.get_sde()
        h = np.asarray(sde.H, np.float64).reshape(-1)
        P0 = np.asarray(sde.P0, np.float64)
        Fs, Qs = _host_discretise(sde.F, P0, t)
        ssm = (P0, Fs, Qs, h[None, :], np.reshape(np.float64(self.noise_variance), (1, 1)))
        fms, fPs, ll, mps, Pps = sequential.kf(ssm, y, return_loglikelihood=True, return_predicted=True,
                                               observation_variances=None if self._obs_var is None else Rk)
        out = {"osa_mean": mps @ h, "osa_var": np.einsum("i,nij,j->n", h, Pps, h) + Rk}
        sms, sPs = sequential.ks(ssm, fms, fPs, mps, Pps)
        out["loo_mean"], out["loo_var"] = _loo_from_smoothed(sms @ h, np.einsum("i,nij,j->n", h, sPs, h), Rk, y)
        for name in ("osa", "loo"):
            out[f"{name}_log_density"] = _backend.normal_log_density(y, out[f"{name}_mean"], out[f"{name}_var"])
        if order is not None:
            for key, val in out.items():
                back = np.empty_like(val)
                back[order] = val
                out[key] = back
        out["ll"] = float(ll)
        out["loo_lpd"] = float(np.nansum(out["loo_log_density"]))
        return out

    @staticmethod
    def _columns_of(out, name):
        dtype = config.default_float()
        return tuple(out[f"{name}_{part}"][:, None].astype(dtype) for part in ("mean", "var", "log_density"))

    @_mean_function_route("_trend_one_step_ahead")
    def one_step_ahead(self):
        """(mean, var, log_density), each (N, 1), in the order of the data rows: the law of y_k given the observations BEFORE
        it (in time), N(mean, var) with the noise in var, and log N(y_k | mean, var) -- the prequential predictive; the
        standardised innovations (y - mean) / sqrt(var) are the residuals of the time-series model.  At a NaN row of y, mean and
        var are the law of an observation there and log_density is NaN; the log densities of the observed rows sum to
        maximum_log_likelihood_objective().  Computed in fp64 and rounded to the default float.  noise_variance <= 0 (with
        observation_variances: noise_variance + s_k <= 0 at an observed row) raises ValueError; Y with more than one column
        NotImplementedError."""
        self._single_output("one_step_ahead")
        return self._columns_of(self._checks(True, False), "osa")

    @_mean_function_route("_trend_leave_one_out")
    def leave_one_out(self):
        """(mean, var, log_density), each (N, 1), in the order of the data rows: the law of y_k given ALL OTHER observations,
        N(mean, var) with the noise in var, and log N(y_k | mean, var) -- leave-one-out cross-validation without a refit.  At a
        NaN row of y nothing is left out: mean and var are the law of an observation there given all data, log_density is NaN.
        Computed in fp64 and rounded to the default float.  Errors as one_step_ahead."""
        self._single_output("leave_one_out")
        return self._columns_of(self._checks(False, True), "loo")

    @_mean_function_route("_trend_loo_lpd")
    def loo_log_predictive_density(self):
        """The leave-one-out cross-validation score (pseudo-likelihood): the sum of leave_one_out()'s log densities over the
        observed rows, a scalar.  On the fused route no per-step array is stored or copied back."""
        self._single_output("loo_log_predictive_density")
        return config.default_float()(self._checks(False, False)["loo_lpd"])

    def predict_y(self, Xnew, full_cov=False, full_output_cov=False):
        """Mean (K, 1) and variance (K, 1) of a NEW observation at `Xnew` (GPflow's predict_y): predict_f with noise_variance
        added to the variance.  With observation_variances set the new points' variances are unknown: NotImplementedError."""
        self._single_output("predict_y")
        if self._obs_var is not None:
            raise NotImplementedError("predict_y is not available with observation_variances set: the variances of new points are unknown")
        if full_cov or full_output_cov:
            raise NotImplementedError("predict_y covers the marginals (full_cov = full_output_cov = False)")
        mean, var = self.predict_f(Xnew)
        return mean, var + var.dtype.type(self.noise_variance)

    @_mean_function_route("_trend_predict_log_density")
    def predict_log_density(self, data, full_cov=False, full_output_cov=False):
        """log N(Ynew | predict_y(Xnew)) for data = (Xnew, Ynew), (K, 1) (GPflow's predict_log_density): the score of
        held-out observations; NaN where Ynew is."""
        self._single_output("predict_log_density")
        Xnew, Ynew = data
        mean, var = self.predict_y(Xnew, full_cov=full_cov, full_output_cov=full_output_cov)
        Ynew = np.asarray(Ynew, np.float64).reshape(mean.shape)
        return _backend.normal_log_density(Ynew, mean, var).astype(config.default_float())
