"""Mean functions of StateSpaceGPPanel (a mixin of the one class, as trend.py is of StateSpaceGP): every series i has its own
trend m_i(t) = Phi_i(t) beta_i on the ONE basis the panel holds (mean_functions.py), with coefficients betas (S, p).

Everything about beta_i comes from the small Gram matrix G_i = V_i^T K_y^-1 V_i, V_i = [y_i, Phi_i] (trend.py's module docstring;
DESIGN.md 4x, 4ad), with K_y = K + diag(noise_variance + s_k) on the observed rows of series i.  The definition of entry i is
the computation on series i alone.  The device route -- parallel=True, a single Matern kernel, float64, 1 + p <= 8 columns --
forms all short series' Gram matrices in ONE call (_backend.panel.gp_panel_gram_dev: one workgroup per series) on columns that
live on the device beside the series.  Everything else -- parallel=False, other kernels, float32, more columns, a series above
_backend.PANEL_MAX_STEPS steps (spliced back) -- is the loop: with scalar noise a StateSpaceGP(..., mean_function=...) on the series,
with observation_variances (where the single model has no such route) the host twin below.
profile_log_likelihoods_and_grads goes further on that route: Gram, the S small solves (one lane per series, where the Gram
records lie), the residuals and the adjoint pass are ONE call (_backend.panel.gp_panel_profile_grad_dev).

The evaluations the panel had before have GPflow's meaning at the CURRENT betas: they run on the residual panel
(t_i, y_i - Phi_i beta_i), kept until betas or data change; Phi(X) beta_i is added to returned means.
"""
import numpy as np

from . import _backend, config
from .gradients import mask_wrt
from .kalman import sequential
from .model import StateSpaceGP
from .trend import _LOG_2PI, RANK_MESSAGES, MeanGram, _chol_design, _chol_solve


def whiten_host(kernel, noise_variance, t, V, observation_variances=None):
    """The host twin of the panel's Gram kernel on ONE series: the sequential filter's standardised innovations of every column
    of V (n, C) (rows where y is NaN already NaN in all columns) over the sorted times t, with the step's noise variance
    noise_variance + observation_variances[k] where those are given -- the per-step analogue of ModelTrend._whiten_host, any
    kernel, fp64.  (W (n, C), logdet, n_obs)."""
    from .model import _host_discretise
    t = np.asarray(t, np.float64).reshape(-1)
    V = np.asarray(V, np.float64)
    sde = kernel.get_sde()
    h = np.asarray(sde.H, np.float64).reshape(-1)
    P0 = np.asarray(sde.P0, np.float64)
    Fs, Qs = _host_discretise(sde.F, P0, t)
    R = np.float64(noise_variance)
    ssm = (P0, Fs, Qs, h[None, :], np.reshape(R, (1, 1)))
    noise = None if observation_variances is None else R + np.asarray(observation_variances, np.float64).reshape(-1)
    obs = ~np.isnan(V[:, 0])
    W = np.zeros(V.shape, np.float64)
    S = None
    for c in range(V.shape[1]):
        _, _, _, mps, Pps = sequential.kf(ssm, np.ascontiguousarray(V[:, c]), return_loglikelihood=True, return_predicted=True,
                                          observation_variances=noise)
        if S is None:
            S = np.einsum("i,nij,j->n", h, Pps, h) + (R if noise is None else noise)
        W[obs, c] = (V[obs, c] - (mps @ h)[obs]) / np.sqrt(S[obs])
    return W, float(np.sum(np.log(S[obs]))), int(np.count_nonzero(obs))


def _mean_gram(G, logdet, n_obs):
    G = np.asarray(G, np.float64)
    return MeanGram(G=G, logdet=float(logdet), n_obs=int(n_obs), g_yy=float(G[0, 0]), b=G[1:, 0].copy(), A=G[1:, 1:].copy())


class PanelTrend:
    """mean_function, betas, mean_grams, mean_coefficients, fit_mean_functions, profile_log_likelihoods,
    log_marginal_likelihoods_flat_mean, profile_log_likelihood_and_grad, profile_log_likelihoods_and_grads, and the residual
    panel of the delegated evaluations."""

    # -- the basis and the coefficients ----------------------------------------------------------------------
    @property
    def mean_function(self):
        """The panel's basis (mean_functions.py), or None: the zero-mean panel, exactly as without the argument.  Its own
        .beta is not used."""
        return self._mean_function

    def _set_mean_function(self, value):
        if value is not None and not callable(getattr(value, "design", None)):
            raise TypeError("mean_function must have design(t) -> (n, p) (pssgp.mean_functions)")
        self._mean_function = value
        self._num_functions = 0 if value is None else int(value.design(np.zeros(1)).shape[1])

    @property
    def betas(self):
        """(S, p) float64: row i holds the trend coefficients of series i (zeros at first)."""
        self._need_mean()
        return self._betas

    @betas.setter
    def betas(self, value):
        self._need_mean()
        b = np.array(value, dtype=np.float64)
        if b.shape != (self.num_series, self._num_functions):
            raise ValueError(f"betas must have shape ({self.num_series}, {self._num_functions}), got {b.shape}")
        self._betas = b

    def _need_mean(self):
        if self._mean_function is None:
            raise ValueError("the panel has no mean_function")

    def _design_columns(self, s):
        """V (n, 1 + p) = [y, Phi] of series s in time order, float64, the rows where y is NaN set to NaN in all columns."""
        ts, ys = self._models[s].data
        Phi = self._mean_function.design(ts.reshape(-1))
        V = np.concatenate([np.asarray(ys, np.float64).reshape(-1, 1), Phi], axis=1)
        V[np.isnan(V[:, 0])] = np.nan
        return V

    def _trend_on_device(self):
        return (self._fused() is not None and bool(self._short)
                and 1 + self._num_functions <= _backend.PANEL_GRAM_COLUMNS_MAX)

    # -- the Gram matrices -------------------------------------------------------------------------------------
    def _trend_model(self, s):
        """StateSpaceGP(..., mean_function=...) on series s at the panel's current setting (scalar noise: the definition)."""
        kept = self._trend_models.get(s)
        if kept is None:
            ts, ys = self._models[s].data
            kept = self._trend_models[s] = StateSpaceGP((ts, ys), self.kernel, self.noise_variance, parallel=self.parallel,
                                                        mean_function=self._mean_function)
        kept.kernel = self.kernel
        kept.noise_variance = self.noise_variance
        return kept

    def _single_gram(self, s):
        """MeanGram of series s alone at the current setting: the single model, or with observation_variances the twin."""
        if self._obs_in is None:
            return self._trend_model(s).mean_gram()
        m = self._models[s]
        W, logdet, n_obs = whiten_host(self.kernel, self.noise_variance, m.data[0], self._design_columns(s),
                                       m.observation_variances)
        G = W.T @ W
        return _mean_gram(0.5 * (G + G.T), logdet, n_obs)

    def mean_grams(self, thetas=None):
        """A list of S MeanGram (trend.py): G_i = V_i^T K_y^-1 V_i for V_i = [y_i, Phi_i], logdet, n_obs and the blocks g_yy, b,
        A of every series, at row i of thetas where given."""
        self._need_mean()
        thetas, params = self._check_thetas(thetas)
        out = [None] * self.num_series
        with StateSpaceGP._parameters_restored(params):
            alone = range(self.num_series)
            if self._trend_on_device():
                G, logdet, n_obs = _backend.panel.gp_panel_gram_dev(self._resident(), self._table(thetas, params))
                for i, s in enumerate(self._short):
                    out[s] = _mean_gram(G[i], logdet[i], n_obs[i])
                alone = self._long
            for s in alone:
                if thetas is not None:
                    StateSpaceGP._assign(params, thetas[s])
                out[s] = self._single_gram(s)
        return out

    @staticmethod
    def _solved(grams):
        """[(gram, L, s, beta_hat)] per series; a rank-deficient series raises ValueError and names it."""
        out = []
        for i, g in enumerate(grams):
            try:
                L, sc = _chol_design(g.A)
            except ValueError as e:
                raise ValueError(f"series {i}: {e}") from None
            out.append((g, L, sc, _chol_solve(L, sc, g.b)))
        return out

    @staticmethod
    def _profile(g, beta):
        return -0.5 * (g.n_obs * _LOG_2PI + g.logdet + g.g_yy - float(g.b @ beta))

    def mean_coefficients(self, thetas=None):
        """(betas_hat (S, p), covs (S, p, p), profile_lls (S,)): the generalised-least-squares estimate A_i^-1 b_i of every
        series' coefficients at the current kernel and noise (row i of thetas where given), its covariance A_i^-1 and the
        log-likelihood at it.  A series whose design matrix has no full column rank on its observed rows raises ValueError."""
        sol = self._solved(self.mean_grams(thetas))
        p = self._num_functions
        betas = np.stack([beta for _, _, _, beta in sol])
        covs = np.empty((self.num_series, p, p), np.float64)
        for i, (g, L, sc, _) in enumerate(sol):
            cov = _chol_solve(L, sc, np.eye(p))
            covs[i] = 0.5 * (cov + cov.T)
        return betas, covs, np.asarray([self._profile(g, beta) for g, _, _, beta in sol], np.float64)

    def fit_mean_functions(self, thetas=None):
        """Assigns betas_hat of mean_coefficients() to betas and returns them."""
        self.betas = self.mean_coefficients(thetas)[0]
        return self._betas

    def profile_log_likelihoods(self, thetas=None):
        """(S,): every series' log-likelihood at its own beta_hat.  It does not depend on betas."""
        return np.asarray([self._profile(g, beta) for g, _, _, beta in self._solved(self.mean_grams(thetas))], np.float64)

    def log_marginal_likelihoods_flat_mean(self, thetas=None):
        """(S,): every series' marginal likelihood with beta_i integrated out under a flat prior (R&W eq. 2.45): the profile
        log-likelihood - 1/2 log |A_i| + (p / 2) log 2 pi.  It does not depend on betas."""
        out = np.empty(self.num_series, np.float64)
        p = self._num_functions
        for i, (g, L, sc, beta) in enumerate(self._solved(self.mean_grams(thetas))):
            logdet_A = 2.0 * float(np.sum(np.log(np.diag(L)))) - 2.0 * float(np.sum(np.log(sc)))
            out[i] = self._profile(g, beta) - 0.5 * logdet_A + 0.5 * p * _LOG_2PI
        return out

    def profile_log_likelihood_and_grad(self, wrt=None):
        """(sum of the profile log-likelihoods, its gradient over trainable_parameters()) at the shared parameters.  At beta_hat
        d ll / d beta = 0, so the gradient with respect to the kernel and the noise is that of the plain likelihood of the
        residuals y_i - Phi_i beta_hat_i.  On the device route: the Gram call, S small solves on the host, betas_hat up, the
        residual kernel, the panel's adjoint pass -- no per-row array crosses the bus.  betas stay as they are."""
        self._need_mean()
        params = self.trainable_parameters()
        sol = self._solved(self.mean_grams())
        betas_hat = np.stack([beta for _, _, _, beta in sol])
        ll, g = 0.0, np.zeros(len(params), np.float64)
        alone = range(self.num_series)
        if self._trend_on_device():
            fused = self._fused()
            pd = self._resident()
            view = _backend.panel.gp_panel_residual_dev(pd, betas_hat[self._short], pd.residual_view())
            rows = _backend.panel.gp_panel_ll_grad_dev(view, self._table(None, params))
            total = np.sum(rows, axis=0)
            ll += float(total[0])
            g += self._helper()._host_adjoint_grad(fused, _backend.split_grad_stats(total, fused[1][1].shape[0]), None)
            alone = self._long
        for s in alone:
            m = self._models[s]
            ts, ys = m.data
            res = (np.asarray(ys, np.float64) - (self._mean_function.design(ts.reshape(-1)) @ betas_hat[s])[:, None]).astype(ys.dtype)
            single = StateSpaceGP((ts, res), self.kernel, self.noise_variance, parallel=self.parallel,
                                  observation_variances=m.observation_variances)
            l1, g1 = self._single_grad(single)
            ll, g = ll + l1, g + g1
        return np.float64(ll), mask_wrt(g, wrt)

    def _residual_single(self, s, beta):
        """The zero-mean single model on (t_s, y_s - Phi_s beta) at the panel's current setting."""
        m = self._models[s]
        ts, ys = m.data
        res = (np.asarray(ys, np.float64) - (self._mean_function.design(ts.reshape(-1)) @ beta)[:, None]).astype(ys.dtype)
        return StateSpaceGP((ts, res), self.kernel, self.noise_variance, parallel=self.parallel,
                            observation_variances=m.observation_variances)

    def profile_log_likelihoods_and_grads(self, thetas=None, reduce=None):
        """reduce=None: ((S,), (S, P)) over trainable_parameters() -- row s is the profile log-likelihood of series s at its own
        beta_hat and its gradient, at row s of thetas where given.  At beta_hat d ll / d beta = 0, so the gradient is that of
        the plain likelihood of the residuals y_s - Phi_s beta_hat_s.  reduce="sum": (float64, (P,)) at the shared parameters
        (thetas must be None): the S rows are summed and contracted ONCE, as log_likelihood_and_grad does -- the meaning of
        profile_log_likelihood_and_grad() without its host solves.

        Device route: ONE _backend.panel.gp_panel_profile_grad_dev call on the short series -- Gram, the S solves, the
        residuals and the adjoint pass queued back to back on the device -- with the long series spliced back.  Everything
        else is the loop: all solves first (a rank-deficient series raises ValueError and is named before any gradient is
        asked for), then the residual model's log_likelihood_and_grad() per series.  betas and the panel's parameters stay as
        they are, on the error paths too."""
        self._need_mean()
        if reduce not in (None, "sum"):
            raise ValueError(f"reduce must be None or 'sum', got {reduce!r}")
        if reduce == "sum" and thetas is not None:
            raise ValueError("reduce='sum' is the population objective at the shared parameters: thetas must be None")
        thetas, params = self._check_thetas(thetas)
        S, P = self.num_series, len(params)
        lls, grads = np.empty(S, np.float64), np.zeros((S, P), np.float64)
        total_ll, total_g = 0.0, np.zeros(P, np.float64)
        with StateSpaceGP._parameters_restored(params):
            alone, failed = range(S), {}
            if self._trend_on_device():
                fused = self._fused()
                rows, _, sol = _backend.panel.gp_panel_profile_grad_dev(self._resident(), self._table(thetas, params))
                p = self._num_functions
                status = np.rint(sol[:, p * p + 3]).astype(np.int64)
                for i in np.flatnonzero(status != 0):
                    failed[self._short[int(i)]] = RANK_MESSAGES[int(status[i])]
                d = fused[1][1].shape[0]
                helper = self._helper()
                if failed:
                    pass                    # (raised below, behind the loop's solves: the lowest such series is named)
                elif reduce == "sum":
                    total = np.sum(rows, axis=0)
                    total_ll += float(total[0])
                    total_g += helper._host_adjoint_grad(fused, _backend.split_grad_stats(total, d), None)
                else:
                    for i, s in enumerate(self._short):
                        if thetas is not None:              # (the contraction reads the kernel's setting: row s)
                            StateSpaceGP._assign(params, thetas[s])
                            fused = self._fused()
                        lls[s] = rows[i, 0]
                        grads[s] = helper._host_adjoint_grad(fused, _backend.split_grad_stats(rows[i], d), None)
                alone = self._long
            alone = list(alone)
            # the loop: every solve before any gradient
            betas_hat = {}
            for s in alone:
                if thetas is not None:
                    StateSpaceGP._assign(params, thetas[s])
                g = self._single_gram(s)
                try:
                    L, sc = _chol_design(g.A)
                except ValueError as e:
                    failed[s] = str(e)
                    continue
                betas_hat[s] = _chol_solve(L, sc, g.b)
            if failed:                      # (the lowest such series, as _solved names it)
                s = min(failed)
                raise ValueError(f"series {s}: {failed[s]}")
            for s in alone:
                if thetas is not None:
                    StateSpaceGP._assign(params, thetas[s])
                l1, g1 = self._single_grad(self._residual_single(s, betas_hat[s]))
                lls[s], grads[s] = l1, g1
                total_ll, total_g = total_ll + l1, total_g + g1
        if reduce == "sum":
            return np.float64(total_ll), total_g
        return lls, grads

    # -- GPflow's meaning of the evaluations the panel had before: the GPs model y_i - m_i(t) ---------------
    def _residual_panel(self):
        """The zero-mean panel on (t_i, y_i - Phi_i beta_i), rows in the order given: shares the kernel object and follows
        noise_variance; rebuilt when the data or betas change."""
        stamp = (self._data_version, self._betas.tobytes())
        kept = self._residual
        if kept is None or kept[0] != stamp:
            if kept is not None:
                kept[1]._release()
            series = []
            for s, (t, y) in enumerate(self._data):
                y = np.asarray(y, np.float64)
                m = (self._mean_function.design(np.asarray(t, np.float64).reshape(-1)) @ self._betas[s]).reshape(y.shape)
                series.append((t, y - m))
            panel = type(self)(series, self.kernel, self.noise_variance, parallel=self.parallel,
                               observation_variances=self._obs_in)
            kept = self._residual = (stamp, panel)
        kept[1].kernel = self.kernel
        kept[1].noise_variance = self.noise_variance
        return kept[1]

    def _mean_at(self, s, X, dtype):
        return (self._mean_function.design(np.asarray(X, np.float64).reshape(-1)) @ self._betas[s])[:, None].astype(dtype)

    def _trend_predict_f(self, Xnews, thetas):
        Xnews = list(Xnews)
        out = self._residual_panel().predict_f(Xnews, thetas)
        return [(mean + self._mean_at(s, Xnews[s], mean.dtype), var) for s, (mean, var) in enumerate(out)]

    def _trend_check(self, name, thetas):
        out = getattr(self._residual_panel(), name)(thetas)
        return [(mean + self._mean_at(s, self._data[s][0], mean.dtype), var, ld) for s, (mean, var, ld) in enumerate(out)]
