"""Mean functions of StateSpaceGP (a mixin of the one class, beside forms.py, gradients.py, batches.py and checks.py).

With m(t) = Phi(t) beta (mean_functions.py), K_y = K + R I = L L^T on the observed rows in time order and W = L^-1 V the
standardised innovations of the columns V = [y, phi_1 .. phi_p] (one covariance pass: gains and innovation variances do not
depend on the column), the Gram matrix G = W^T W = V^T K_y^-1 V has (1 + p)^2 entries

    g_yy = y^T K_y^-1 y,    b = Phi^T K_y^-1 y,    A = Phi^T K_y^-1 Phi

and everything about beta comes from it (Rasmussen & Williams section 2.7):

    ll(beta)            = -1/2 (n log 2 pi + logdet + g_yy - 2 beta^T b + beta^T A beta)
    d ll / d beta       = b - A beta
    beta_hat, its cov   = A^-1 b,  A^-1                                   (generalised least squares)
    profile ll          = -1/2 (n log 2 pi + logdet + g_yy - b^T A^-1 b)
    flat-prior marginal = profile ll - 1/2 log |A| + (p / 2) log 2 pi     (eq. 2.45)

The evaluations the model had before have GPflow's meaning at the CURRENT beta: the GP models y - m(t).  They are delegated to
one internal zero-mean model on (t, y - Phi beta); m is added to returned means and draws and taken from the y side of
densities.
"""
from dataclasses import dataclass

import numpy as np
from scipy.linalg import solve_triangular

from . import _backend, config
from .kalman import sequential

_LOG_2PI = float(np.log(2.0 * np.pi))


@dataclass
class MeanGram:
    """mean_gram()'s record: G (1 + p, 1 + p) for V = [y, Phi], logdet = log |K_y|, the number of observed rows, and G's blocks."""
    G: np.ndarray
    logdet: float
    n_obs: int
    g_yy: float
    b: np.ndarray
    A: np.ndarray


_RANK = "the mean function's design matrix does not have full column rank on the observed rows"
# _chol_design's refusals, under the status the device solve gives them (csrc/pgps_panel_trend.hip.h)
RANK_MESSAGES = {1: _RANK + " (a basis function is zero or not finite there)", 2: _RANK,
                 3: _RANK + " (its basis functions are linearly dependent)"}


def _chol_design(A):
    """(L, s) with diag(s) A diag(s) = L L^T, s = 1 / sqrt(diag A): the factor of A on unit diagonal, so that a pivot measures
    how much of a basis function its predecessors leave.  ValueError when the design matrix has no full column rank on the
    observed rows (a pivot at rounding level, or no factor at all)."""
    A = np.asarray(A, np.float64)
    p = A.shape[0]
    dg = np.diag(A)
    if not (np.all(np.isfinite(A)) and np.all(dg > 0.0)):
        raise ValueError(RANK_MESSAGES[1])
    s = 1.0 / np.sqrt(dg)
    try:
        L = np.linalg.cholesky(A * s[:, None] * s[None, :])
    except np.linalg.LinAlgError:
        raise ValueError(RANK_MESSAGES[2]) from None
    if np.min(np.diag(L)) ** 2 <= 64.0 * p * np.finfo(np.float64).eps:
        raise ValueError(RANK_MESSAGES[3])
    return L, s


def _chol_solve(L, s, B):
    """A^-1 B for the factor of _chol_design."""
    B = np.asarray(B, np.float64)
    sB = B * (s if B.ndim == 1 else s[:, None])
    X = solve_triangular(L, solve_triangular(L, sB, lower=True), lower=True, trans="T")
    return X * (s if B.ndim == 1 else s[:, None])


class ModelTrend:
    """mean_function, whiten, mean_gram, mean_coefficients, fit_mean_function, log_marginal_likelihood_flat_mean,
    predict_f_gls, and the routes of the delegated evaluations."""

    @property
    def mean_function(self):
        """The model's mean function (mean_functions.py), or None: the zero-mean model, exactly as without the argument."""
        return self._mean_function

    @mean_function.setter
    def mean_function(self, value):
        if value is not None:
            if self.num_latent_gps > 1:
                raise NotImplementedError(f"mean_function covers single-output models; this one has {self.num_latent_gps} "
                                          "output columns")
            if self._obs_var is not None:
                raise NotImplementedError("mean_function is not available with observation_variances set")
            if not (callable(getattr(value, "design", None)) and hasattr(value, "beta")):
                raise TypeError("mean_function must have design(t) -> (n, p) and beta (p,) (pssgp.mean_functions)")
        self._mean_function = value
        self._residual = None

    # -- the columns V = [y, Phi] ---------------------------------------------------------------------
    def _design_columns(self):
        """(Phi (N, p), V (N, 1 + p) = [y, Phi] in float64 with the rows where y is NaN set to NaN in all columns)."""
        if self._mean_function is None:
            raise ValueError("the model has no mean_function")
        ts, ys = self.data
        Phi = self._mean_function.design(ts.reshape(-1))
        V = np.concatenate([np.asarray(ys, np.float64).reshape(-1, 1), Phi], axis=1)
        V[np.isnan(V[:, 0])] = np.nan
        return Phi, V

    def _whiten_host(self, V):
        """The host twin of _backend.gp_whiten_multi: the sequential filter's standardised innovations of every column of V
        (N, C) (rows where y is NaN already NaN), in fp64 -- any kernel, both modes; times out of order are sorted for it
        (stable) and the rows put back.  (W, logdet, n_obs)."""
        from .model import _host_discretise, _is_sorted
        ts, _ = self.data
        t = np.asarray(ts, np.float64).reshape(-1)
        order = None if _is_sorted(t) else np.argsort(t, kind="stable")
        if order is not None:
            t, V = t[order], V[order]
        sde = self.kernel.get_sde()
        h = np.asarray(sde.H, np.float64).reshape(-1)
        P0 = np.asarray(sde.P0, np.float64)
        Fs, Qs = _host_discretise(sde.F, P0, t)
        ssm = (P0, Fs, Qs, h[None, :], np.reshape(np.float64(self.noise_variance), (1, 1)))
        obs = ~np.isnan(V[:, 0])
        W = np.zeros(V.shape, np.float64)
        S = None
        for c in range(V.shape[1]):
            _, _, _, mps, Pps = sequential.kf(ssm, np.ascontiguousarray(V[:, c]), return_loglikelihood=True, return_predicted=True)
            if S is None:
                S = np.einsum("i,nij,j->n", h, Pps, h) + np.float64(self.noise_variance)
            W[obs, c] = (V[obs, c] - (mps @ h)[obs]) / np.sqrt(S[obs])
        if order is not None:
            back = np.empty_like(W)
            back[order] = W
            W = back
        return W, float(np.sum(np.log(S[obs]))), int(np.count_nonzero(obs))

    def whiten(self, V):
        """W (N, C), float64, for V (N,) or (N, C): the standardised innovations (V[k, c] - mu_c[k]) / sqrt(S_k) of the Kalman
        pass over the training times, column by column -- W = L^-1 V with K + noise_variance I = L L^T on the observed rows in
        time order, so a^T K_y^-1 b = whiten(a)^T whiten(b) for any vectors over the training points.  Rows where y is NaN
        are missing steps: zero rows of W (V is not read there).  Works with mean_function=None as well.  The fused route of
        the class docstring: one covariance pass for all columns (_backend.gp_whiten_multi); everything else: the host twin."""
        if self.num_latent_gps > 1:
            raise NotImplementedError(f"whiten covers single-output models; this one has {self.num_latent_gps} output columns")
        if self._obs_var is not None:
            raise NotImplementedError("whiten is not available with observation_variances set")
        return self._whiten(V)[0]

    def _whiten(self, V):
        ts, ys = self.data
        V = np.array(V, dtype=np.float64)
        V = V[:, None] if V.ndim == 1 else V
        if V.ndim != 2 or V.shape[0] != ts.shape[0] or V.shape[1] < 1:
            raise ValueError(f"V must be ({ts.shape[0]},) or ({ts.shape[0]}, C) like the data, got shape {V.shape}")
        V[np.isnan(np.asarray(ys, np.float64).reshape(-1))] = np.nan
        fused = self._fused_route()
        if fused is not None:
            sde, form = fused
            return _backend.gp_whiten_multi(form, sde.P0, sde.H, self.noise_variance, ts.reshape(-1), V)
        return self._whiten_host(V)

    def mean_gram(self):
        """MeanGram: G = V^T K_y^-1 V for V = [y, Phi], logdet, n_obs and the blocks g_yy, b, A (module docstring).  The fused
        route with 1 + p <= 16: one covariance pass and one Gram pass on the device, W never leaves it
        (_backend.gp_gram_multi).  Everything else -- parallel=False, float32 data, other kernels, times out of order, more
        columns -- the host twin: W^T W of the sequential filter's innovations."""
        _, V = self._design_columns()
        fused = self._fused_route()
        if fused is not None and V.shape[1] <= _backend.GRAM_COLUMNS_MAX:
            sde, form = fused
            G, logdet, n_obs = _backend.gp_gram_multi(form, sde.P0, sde.H, self.noise_variance, self.data[0].reshape(-1), V)
        else:
            W, logdet, n_obs = self._whiten_host(V)
            G = W.T @ W
            G = 0.5 * (G + G.T)
        return MeanGram(G=G, logdet=logdet, n_obs=n_obs, g_yy=float(G[0, 0]), b=G[1:, 0].copy(), A=G[1:, 1:].copy())

    def _gls_solution(self):
        g = self.mean_gram()
        L, s = _chol_design(g.A)
        beta = _chol_solve(L, s, g.b)
        return g, L, s, beta

    def mean_coefficients(self):
        """(beta_hat (p,), cov_beta (p, p), profile_ll): the generalised-least-squares estimate A^-1 b of the mean function's
        coefficients at the current kernel and noise, its covariance A^-1, and the log-likelihood at beta_hat.  A design
        matrix without full column rank on the observed rows raises ValueError."""
        g, L, s, beta = self._gls_solution()
        cov = _chol_solve(L, s, np.eye(g.A.shape[0]))
        profile = -0.5 * (g.n_obs * _LOG_2PI + g.logdet + g.g_yy - float(g.b @ beta))
        return beta, 0.5 * (cov + cov.T), np.float64(profile)

    def fit_mean_function(self):
        """Assigns beta_hat of mean_coefficients() to mean_function.beta and returns it."""
        beta = self.mean_coefficients()[0]
        self._mean_function.beta = beta
        return self._mean_function.beta

    def log_marginal_likelihood_flat_mean(self):
        """The marginal likelihood with beta integrated out under a flat prior (R&W eq. 2.45): the profile log-likelihood
        - 1/2 log |A| + (p / 2) log 2 pi.  It does not depend on mean_function.beta."""
        g, L, s, beta = self._gls_solution()
        p = g.A.shape[0]
        profile = -0.5 * (g.n_obs * _LOG_2PI + g.logdet + g.g_yy - float(g.b @ beta))
        logdet_A = 2.0 * float(np.sum(np.log(np.diag(L)))) - 2.0 * float(np.sum(np.log(s)))
        return np.float64(profile - 0.5 * logdet_A + 0.5 * p * _LOG_2PI)

    def _gls_columns_model(self, V):
        """The zero-mean model on the columns [y, Phi]: its predict_f is ONE _backend.gp_predict_multi call on the fused route and
        the column loop off it."""
        ts, ys = self.data
        return type(self)((ts, V.astype(ys.dtype)), self.kernel, self.noise_variance, parallel=self.parallel,
                          max_parallel=self.max_parallel)

    def predict_f_gls(self, Xnew):
        """Posterior mean (K, 1) and variance (K, 1) of f = GP + m at `Xnew` with beta integrated out under a flat prior (R&W
        eq. 2.41, 2.42).  With P = [p_y, P_Phi] the zero-mean predictions of the columns [y, Phi] at the queries and var their
        shared variance: Rq = Phi(Xnew) - P_Phi, mean = p_y + Rq beta_hat, var = var + diag(Rq A^-1 Rq^T).  It does not depend
        on mean_function.beta."""
        _, V = self._design_columns()
        g, L, s, beta = self._gls_solution()
        xq = np.asarray(Xnew, dtype=config.default_float()).reshape(-1)
        P, var = self._gls_columns_model(V).predict_f(xq[:, None])
        P, var = np.asarray(P, np.float64), np.asarray(var, np.float64)[:, 0]
        Rq = self._mean_function.design(xq) - P[:, 1:]
        mean = P[:, 0] + Rq @ beta
        var = var + np.einsum("kp,pk->k", Rq, _chol_solve(L, s, Rq.T))
        dtype = config.default_float()
        return mean[:, None].astype(dtype), var[:, None].astype(dtype)

    # -- GPflow's meaning of the evaluations the model had before: the GP models y - m(t) ------------------
    def _residual_model(self):
        """The zero-mean model on (t, y - Phi beta): shares the kernel object and follows noise_variance; rebuilt when the data
        or beta change."""
        ts, ys = self.data
        beta = np.asarray(self._mean_function.beta, np.float64)
        stamp = (self._data_stamp(ts, ys), id(self._mean_function), beta.tobytes())
        kept = getattr(self, "_residual", None)
        if kept is None or kept[0] != stamp:
            res = (ys - self._mean_function(ts.reshape(-1))[:, None]).astype(ys.dtype)
            model = type(self)((ts, res), self.kernel, self.noise_variance, parallel=self.parallel, max_parallel=self.max_parallel)
            kept = self._residual = (stamp, model)
        kept[1].kernel = self.kernel
        kept[1].noise_variance = self.noise_variance
        return kept[1]

    def _mean_at(self, X, dtype):
        return self._mean_function(np.asarray(X, np.float64).reshape(-1))[:, None].astype(dtype)

    def _trend_objective(self):
        return self._residual_model().maximum_log_likelihood_objective()

    def _trend_predict_f(self, Xnew, full_cov=False, full_output_cov=False):
        mean, var = self._residual_model().predict_f(Xnew, full_cov=full_cov, full_output_cov=full_output_cov)
        return mean + self._mean_at(Xnew, mean.dtype), var

    def _trend_predict_f_samples(self, Xnew, num_samples=None, full_cov=True, full_output_cov=False, seed=None):
        f = self._residual_model().predict_f_samples(Xnew, num_samples=num_samples, full_cov=full_cov,
                                                     full_output_cov=full_output_cov, seed=seed)
        return f + self._mean_at(Xnew, f.dtype)             # (K, 1) broadcasts over the draws

    def _trend_check(self, name):
        mean, var, log_density = getattr(self._residual_model(), name)()
        return mean + self._mean_at(self.data[0], mean.dtype), var, log_density

    def _trend_one_step_ahead(self):
        return self._trend_check("one_step_ahead")

    def _trend_leave_one_out(self):
        return self._trend_check("leave_one_out")

    def _trend_loo_lpd(self):
        return self._residual_model().loo_log_predictive_density()

    def _trend_predict_log_density(self, data, full_cov=False, full_output_cov=False):
        Xnew, Ynew = data
        Ynew = np.asarray(Ynew, np.float64).reshape(-1, 1)
        return self._residual_model().predict_log_density((Xnew, Ynew - self._mean_at(Xnew, np.float64)), full_cov=full_cov,
                                                          full_output_cov=full_output_cov)

    def _trend_ll_and_grad(self, wrt=None, method=None):
        """The residual model's (ll, gradient) followed by d ll / d beta = b - A beta from mean_gram().  `wrt` masks the beta
        entries like any other; with only beta entries asked for, the kernel's gradient is not computed (and parallel=False
        models answer too)."""
        res = self._residual_model()
        n_res = len(res.trainable_parameters())
        beta = np.asarray(self._mean_function.beta, np.float64)
        wrt_res = None if wrt is None else [int(i) for i in wrt if int(i) < n_res]
        if wrt is not None and any(not 0 <= int(i) < n_res + beta.shape[0] for i in wrt):
            raise IndexError(f"wrt indexes {n_res + beta.shape[0]} trainable parameters, got {list(wrt)}")
        if wrt_res is not None and not wrt_res:
            ll, g_res = res.maximum_log_likelihood_objective(), np.zeros(n_res)
        else:
            ll, g_res = res.log_likelihood_and_grad(wrt=wrt_res, method=method)
        g_beta = np.zeros(beta.shape[0])
        if wrt is None or any(int(i) >= n_res for i in wrt):
            g = self.mean_gram()
            g_beta = g.b - g.A @ beta
            if wrt is not None:
                keep = np.zeros(beta.shape[0], bool)
                keep[[int(i) - n_res for i in wrt if int(i) >= n_res]] = True
                g_beta = np.where(keep, g_beta, 0.0)
        return ll, np.concatenate([np.asarray(g_res, np.float64).reshape(-1), g_beta])
