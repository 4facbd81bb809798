"""StateSpaceGPPanel: S independent series, each with its own time stamps and length, under one kernel -- the light curves of
a survey with their error bars, one record per patient or sensor, the folds of a cross-validation.

The definition of every result is the loop: row s is what a StateSpaceGP on series s alone returns.  That loop is also the host
twin (parallel=False, kernels other than a single Matern-1/2, -3/2 or -5/2, float32).  The device route -- parallel=True, a
single Matern kernel, float64 -- evaluates all series in ONE call of the panel entry points (_backend.panel: one workgroup per
series) on concatenated arrays that live on the device from construction, or from the assignment of
`data`, until the panel is dropped.  A series above _backend.PANEL_MAX_STEPS steps (counted merged with its queries in
predict_f) leaves the panel call: its own internal StateSpaceGP evaluates it and the result is spliced back in place.
The predictive checks of every series (one_step_ahead, leave_one_out, loo_log_predictive_densities)
follow the same two routes.
"""
import numpy as np

from . import _backend, config
from .gradients import mask_wrt
from .model import StateSpaceGP
from .panel_fit import PanelFitting
from .panel_trend import PanelTrend


def _column(a, what, s):
    a = np.asarray(a, dtype=config.default_float())
    if a.ndim == 2 and a.shape[1] == 1:
        a = a[:, 0]
    if a.ndim != 1:
        raise ValueError(f"series {s}: {what} must be (n,) or (n, 1), got shape {a.shape}")
    return a


class StateSpaceGPPanel(PanelTrend, PanelFitting):
    """StateSpaceGPPanel(series, kernel, noise_variance=1.0, parallel=True, observation_variances=None, mean_function=None).

    series: a list of S pairs (t_i, y_i), each (n_i,) or (n_i, 1), n_i >= 1; NaN in y is a missing observation.  Times in any
    order: every series is sorted once (stable) at construction.  observation_variances: None, or a list of S arrays of given
    per-observation noise variances, each validated as StateSpaceGP validates its own.

    `thetas` of the methods below is in the order of trainable_parameters(): None = the panel's own parameters shared by all
    series, or (S, P) = one row per series.  The panel's own parameters are restored on every exit path.

    mean_function: None, or one basis of pssgp.mean_functions: series i then has the trend Phi_i(t) betas[i] (panel_trend.py;
    DESIGN.md section 4ad), with or without observation_variances.  betas (S, p) is a settable float64 array, zeros at first;
    every evaluation below models y_i - Phi_i betas[i] and adds Phi(X) betas[i] to the means it returns.  None is the panel
    exactly as without the argument."""

    def __init__(self, series, kernel, noise_variance=1.0, parallel=True, observation_variances=None, mean_function=None):
        self._set_mean_function(mean_function)
        self._data_version = 0
        self._residual = None
        self.kernel = kernel
        self.noise_variance = float(noise_variance)
        self.parallel = bool(parallel)
        self._panel_data = None
        self._obs_in = observation_variances
        self.data = series

    # -- data ----------------------------------------------------------------------------------------------
    @property
    def data(self):
        return self._data

    @data.setter
    def data(self, series):
        self._build(series, self._obs_in)

    @property
    def observation_variances(self):
        return self._obs_in

    @observation_variances.setter
    def observation_variances(self, value):
        self._build(self._data, value)

    def _build(self, series, obs):
        series = list(series)
        if len(series) < 1:
            raise ValueError("a panel holds at least one series")
        if obs is not None:
            obs = list(obs)
            if len(obs) != len(series):
                raise ValueError(f"observation_variances has {len(obs)} entries, the panel {len(series)} series")
        data, models, orders = [], [], []
        for s, pair in enumerate(series):
            if len(pair) != 2:
                raise ValueError(f"series {s}: expected a pair (t, y)")
            t, y = _column(pair[0], "t", s), _column(pair[1], "y", s)
            if t.shape[0] < 1:
                raise ValueError(f"series {s} is empty")
            if y.shape[0] != t.shape[0]:
                raise ValueError(f"series {s}: t has {t.shape[0]} rows, y {y.shape[0]}")
            order = None if np.all(np.diff(t) >= 0) else np.argsort(t, kind="stable")
            v = None if obs is None else np.asarray(obs[s], np.float64)
            if v is not None and v.ndim == 2 and v.shape[1] == 1:
                v = v[:, 0]
            if order is not None:
                t, y = t[order], y[order]
                if v is not None and v.shape == t.shape:
                    v = v[order]
            # (the single model validates the variances' shape and values against its data)
            models.append(StateSpaceGP((np.ascontiguousarray(t)[:, None], np.ascontiguousarray(y)[:, None]), self.kernel,
                                       self.noise_variance, parallel=self.parallel, observation_variances=v))
            data.append((pair[0], pair[1]))
            orders.append(order)
        self._release()
        self._data, self._obs_in, self._models = data, obs, models
        self._data_version += 1
        self._trend_models = {}
        if self._mean_function is not None and getattr(self, "_betas", np.zeros((0, 0))).shape != (len(models), self._num_functions):
            self._betas = np.zeros((len(models), self._num_functions), np.float64)
        self._orders = orders           # (the stable sort of every series that was not in time order, else None)
        # the smallest given variance at an observed row of every series (the predictive checks' rule on the device route)
        self._obs_floor = None if obs is None else [
            float(np.min(m.observation_variances[~np.isnan(m.data[1].reshape(-1))], initial=np.inf)) for m in models]
        self.num_series = len(models)
        self._short = [s for s, m in enumerate(models) if m.data[0].shape[0] <= _backend.PANEL_MAX_STEPS]
        self._long = [s for s, m in enumerate(models) if m.data[0].shape[0] > _backend.PANEL_MAX_STEPS]
        if self._fused() is not None and self._short:
            self._resident()

    def _release(self):
        pd, self._panel_data = getattr(self, "_panel_data", None), None
        if pd is not None:
            pd.close()
        kept, self._residual = getattr(self, "_residual", None), None
        if kept is not None:
            kept[1]._release()

    def __del__(self):
        try:
            self._release()
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass

    def _resident(self):
        """The short series, concatenated, on the device (made once per data assignment; owned by the panel)."""
        if self._panel_data is None:
            ms = [self._models[s] for s in self._short]
            offs = np.concatenate([[0], np.cumsum([m.data[0].shape[0] for m in ms])])
            ts = np.concatenate([m.data[0].reshape(-1) for m in ms])
            ys = np.concatenate([m.data[1].reshape(-1) for m in ms])
            rs = None if self._obs_in is None else np.concatenate([m.observation_variances for m in ms])
            V = None                # (with a mean function: the columns [y, Phi] of every series beside them)
            if self._mean_function is not None and 1 + self._num_functions <= _backend.PANEL_GRAM_COLUMNS_MAX:
                V = np.concatenate([self._design_columns(s) for s in self._short])
            self._panel_data = _backend.PanelData(offs, ts, ys, rs, V=V)
        return self._panel_data

    # -- the kernel's forms and parameters --------------------------------------------------------------------
    def _helper(self):
        """A StateSpaceGP on no data of its own that holds the kernel: its memoised device forms and gradient contraction are
        the ones the panel uses."""
        h = getattr(self, "_gp", None)
        if h is None or h.kernel is not self.kernel:
            h = self._gp = StateSpaceGP((np.zeros((1, 1)), np.zeros((1, 1))), self.kernel, noise_variance=1.0, parallel=True)
        return h

    def _fused(self):
        """(sde-like, form) where the device route applies, else None (the loop over the single models)."""
        if not self.parallel or config.default_float() != np.float64:
            return None
        return self._helper()._matern_forms()

    def trainable_parameters(self):
        """[(owner, attribute name)] in the order of `thetas` and of the gradients: the kernel's leaves, then the panel's
        noise_variance."""
        return self._helper().trainable_parameters()[:-1] + [(self, "noise_variance")]

    def _check_thetas(self, thetas):
        params = self.trainable_parameters()
        if thetas is None:
            return None, params
        thetas = np.asarray(thetas, np.float64)
        if thetas.ndim != 2 or thetas.shape != (self.num_series, len(params)):
            raise ValueError(f"thetas has shape {thetas.shape}: expected ({self.num_series}, {len(params)}), one row per series")
        return thetas, params

    def _synced(self, s):
        """The single model of series s at the panel's current setting."""
        m = self._models[s]
        m.kernel = self.kernel
        m.noise_variance = self.noise_variance
        return m

    def _row(self, fused):
        sde, form = fused
        return np.concatenate([[float(form[0])], np.asarray(form[1], np.float64).reshape(-1), np.asarray(form[2], np.float64).reshape(-1),
                               np.asarray(sde.P0, np.float64).reshape(-1), np.asarray(sde.H, np.float64).reshape(-1),
                               [float(self.noise_variance)]])

    def _table(self, thetas, params):
        """The model table of the panel call: one row at the current setting, or the rows of the short series' thetas."""
        if thetas is None:
            return self._row(self._fused())[None, :]
        rows = []
        for s in self._short:
            StateSpaceGP._assign(params, thetas[s])
            fused = self._fused()
            if fused is None:
                raise ValueError(f"thetas row {s} is no valid setting of the kernel (variance and lengthscale must be > 0)")
            rows.append(self._row(fused))
        return np.ascontiguousarray(np.stack(rows))

    def _each(self, thetas, params, visit, subset=None):
        """visit(s, single model of series s) with row s of thetas assigned (or the current setting), for s in subset."""
        out = {}
        for s in range(self.num_series) if subset is None else subset:
            if thetas is not None:
                StateSpaceGP._assign(params, thetas[s])
            out[s] = visit(s, self._synced(s))
        return out

    # -- evaluations -----------------------------------------------------------------------------------------
    def log_likelihoods(self, thetas=None):
        """(S,): the marginal log-likelihood of every series."""
        if self._mean_function is not None:
            return self._residual_panel().log_likelihoods(thetas)
        thetas, params = self._check_thetas(thetas)
        dtype = config.default_float()
        out = np.empty(self.num_series, dtype)
        with StateSpaceGP._parameters_restored(params):
            if self._fused() is None:
                for s, v in self._each(thetas, params, lambda s, m: m.maximum_log_likelihood_objective()).items():
                    out[s] = v
                return out
            if self._short:
                out[self._short] = _backend.panel.gp_panel_ll_dev(self._resident(), self._table(thetas, params))
            for s, v in self._each(thetas, params, lambda s, m: m.maximum_log_likelihood_objective(), self._long).items():
                out[s] = v
        return out

    def maximum_log_likelihood_objective(self):
        """The sum of the series' log-likelihoods at the shared parameters (a population fit)."""
        return config.default_float()(np.sum(self.log_likelihoods()))

    def training_loss(self):
        return -self.maximum_log_likelihood_objective()

    def _single_grad(self, m):
        ll, g = m.log_likelihood_and_grad()
        return float(ll), np.asarray(g, np.float64)

    def log_likelihoods_and_grads(self, thetas=None):
        """((S,), (S, P)): every series' log-likelihood and its gradient with respect to trainable_parameters() (at row s of
        thetas where given).  Where the single model has no gradient, its NotImplementedError is raised."""
        if self._mean_function is not None:
            return self._residual_panel().log_likelihoods_and_grads(thetas)
        thetas, params = self._check_thetas(thetas)
        S, P = self.num_series, len(params)
        lls, grads = np.empty(S, np.float64), np.empty((S, P), np.float64)
        with StateSpaceGP._parameters_restored(params):
            fused = self._fused()
            if fused is None:
                for s, (ll, g) in self._each(thetas, params, lambda s, m: self._single_grad(m)).items():
                    lls[s], grads[s] = ll, g
                return lls.astype(config.default_float()), grads
            if self._short:
                rows = _backend.panel.gp_panel_ll_grad_dev(self._resident(), self._table(thetas, params))
                d = fused[1][1].shape[0]
                helper = self._helper()
                for i, s in enumerate(self._short):
                    if thetas is not None:                  # (the contraction reads the kernel's setting: row s)
                        StateSpaceGP._assign(params, thetas[s])
                        fused = self._fused()
                    lls[s] = rows[i, 0]
                    grads[s] = helper._host_adjoint_grad(fused, _backend.split_grad_stats(rows[i], d), None)
            for s, (ll, g) in self._each(thetas, params, lambda s, m: self._single_grad(m), self._long).items():
                lls[s], grads[s] = ll, g
        return lls, grads

    def log_likelihood_and_grad(self, wrt=None):
        """(sum of the log-likelihoods, its gradient) at the shared parameters.  On the device route the S adjoint rows are
        summed first and contracted once."""
        if self._mean_function is not None:
            return self._residual_panel().log_likelihood_and_grad(wrt)
        params = self.trainable_parameters()
        fused = self._fused()
        if fused is None:
            out = self._each(None, params, lambda s, m: self._single_grad(m))
            return (config.default_float()(np.sum([o[0] for o in out.values()])),
                    mask_wrt(np.sum([o[1] for o in out.values()], axis=0), wrt))
        ll, g = 0.0, np.zeros(len(params), np.float64)
        if self._short:
            rows = _backend.panel.gp_panel_ll_grad_dev(self._resident(), self._table(None, params))
            d = fused[1][1].shape[0]
            total = np.sum(rows, axis=0)
            ll += float(total[0])
            g += self._helper()._host_adjoint_grad(fused, _backend.split_grad_stats(total, d), None)
        for s in self._long:
            l1, g1 = self._single_grad(self._synced(s))
            ll, g = ll + l1, g + g1
        return np.float64(ll), mask_wrt(g, wrt)

    def predict_f(self, Xnews, thetas=None):
        """A list of S pairs (mean (K_i, 1), var (K_i, 1)): the posterior of f at Xnews[i] for series i.  Queries in any order,
        repeated times allowed; an empty Xnews[i] gives empty arrays."""
        if self._mean_function is not None:
            return self._trend_predict_f(Xnews, thetas)
        Xnews = list(Xnews)
        if len(Xnews) != self.num_series:
            raise ValueError(f"Xnews has {len(Xnews)} entries, the panel {self.num_series} series")
        thetas, params = self._check_thetas(thetas)
        dtype = config.default_float()
        uniq = [np.unique(np.asarray(x, dtype=dtype).reshape(-1), return_inverse=True) for x in Xnews]
        means = [np.zeros(0, dtype)] * self.num_series
        vars_ = [np.zeros(0, dtype)] * self.num_series

        def single(s, m):
            mean, var = m.predict_f(uniq[s][0][:, None])
            return np.asarray(mean).reshape(-1), np.asarray(var).reshape(-1)

        asked = [s for s in range(self.num_series) if uniq[s][0].size > 0]
        with StateSpaceGP._parameters_restored(params):
            if self._fused() is None:
                alone = asked
            else:
                n_of = lambda s: self._models[s].data[0].shape[0]
                inside = [s for s in self._short if uniq[s][0].size > 0 and n_of(s) + uniq[s][0].size <= _backend.PANEL_MAX_STEPS]
                keep = set(inside)
                alone = [s for s in asked if s not in keep]
                if inside:
                    counts = [uniq[s][0].size if s in keep else 0 for s in self._short]
                    qoffs = np.concatenate([[0], np.cumsum(counts)])
                    tq = np.concatenate([uniq[s][0] for s in self._short if s in keep]).astype(np.float64)
                    mean, var, _ = _backend.panel.gp_panel_predict_dev(self._resident(), self._table(thetas, params), qoffs, tq)
                    for i, s in enumerate(self._short):
                        if s in keep:
                            means[s], vars_[s] = mean[qoffs[i]:qoffs[i + 1]], var[qoffs[i]:qoffs[i + 1]]
            for s, (mean, var) in self._each(thetas, params, single, alone).items():
                means[s], vars_[s] = mean, var
        return [(np.asarray(means[s])[uniq[s][1].reshape(-1)][:, None].astype(dtype, copy=False),
                 np.asarray(vars_[s])[uniq[s][1].reshape(-1)][:, None].astype(dtype, copy=False)) for s in range(self.num_series)]

    # -- predictive checks ---------------------------------------------------------
    def _check_noise(self, thetas):
        """The single model's rule on the device route, where no single model is asked: noise_variance (+ s_k) > 0 wherever y
        is observed, for every short series (at its own row of thetas)."""
        for s in self._short:
            R = float(self.noise_variance if thetas is None else thetas[s, -1])
            if self._obs_in is None:
                if not R > 0.0:
                    raise ValueError(f"the predictive checks need noise_variance > 0, got {R}")
            elif not R + self._obs_floor[s] > 0.0:
                raise ValueError("the predictive checks need noise_variance + observation_variances > 0 wherever y is observed")

    def _checks(self, thetas, osa, loo):
        """A list of S dicts as StateSpaceGP._checks returns them (fp64, rows in TIME order: the order of the single models'
        data), on either route: the loop of the single models, or ONE gp_panel_loo_dev call on the resident short series with
        the long ones spliced back from their own models."""
        thetas, params = self._check_thetas(thetas)
        out = [None] * self.num_series
        with StateSpaceGP._parameters_restored(params):
            alone = None
            if self._fused() is not None:
                alone = self._long
                if self._short:
                    self._check_noise(thetas)
                    pd = self._resident()
                    res = _backend.panel.gp_panel_loo_dev(pd, self._table(thetas, params), osa=osa, loo=loo)
                    rows = [k for k, v in res.items() if k not in ("ll", "loo_lpd")]
                    for i, s in enumerate(self._short):
                        a, b = int(pd.offs[i]), int(pd.offs[i + 1])
                        out[s] = {k: res[k][a:b] for k in rows}
                        out[s]["ll"], out[s]["loo_lpd"] = float(res["ll"][i]), float(res["loo_lpd"][i])
            for s, v in self._each(thetas, params, lambda s, m: m._checks(osa, loo), alone).items():
                out[s] = v
        return out

    def _columns(self, out, name):
        """The triples of series s = 0 .. S - 1 from _checks' dicts: rows put back in the order they were given."""
        cols = []
        for s, o in enumerate(out):
            order = self._orders[s]
            if order is not None:
                o = dict(o)
                for part in ("mean", "var", "log_density"):
                    back = np.empty_like(o[f"{name}_{part}"])
                    back[order] = o[f"{name}_{part}"]
                    o[f"{name}_{part}"] = back
            cols.append(StateSpaceGP._columns_of(o, name))
        return cols

    def one_step_ahead(self, thetas=None):
        """A list of S triples (mean, var, log_density), each (n_i, 1), in the order the rows of series i were given: what
        StateSpaceGP.one_step_ahead returns on series i alone (at row i of thetas where given).  log_density is NaN at the NaN
        rows of y.  Computed in fp64 and rounded to the default float.  noise_variance <= 0 (with observation_variances:
        noise_variance + s_k <= 0 at an observed row) raises ValueError."""
        if self._mean_function is not None:
            return self._trend_check("one_step_ahead", thetas)
        return self._columns(self._checks(thetas, True, False), "osa")

    def leave_one_out(self, thetas=None):
        """A list of S triples (mean, var, log_density) as one_step_ahead returns them: the law of every y_k given ALL OTHER
        observations of its series (StateSpaceGP.leave_one_out on series i alone), without a refit."""
        if self._mean_function is not None:
            return self._trend_check("leave_one_out", thetas)
        return self._columns(self._checks(thetas, False, True), "loo")

    def loo_log_predictive_densities(self, thetas=None):
        """(S,): the leave-one-out cross-validation score of every series, the sum of leave_one_out()'s log densities over its
        observed rows -- which series the model explains badly.  On the device route no per-row array is stored or copied."""
        if self._mean_function is not None:
            return self._residual_panel().loo_log_predictive_densities(thetas)
        return np.asarray([o["loo_lpd"] for o in self._checks(thetas, False, False)], np.float64).astype(config.default_float())

    def loo_log_predictive_density(self):
        """The sum of loo_log_predictive_densities() at the shared parameters."""
        return config.default_float()(np.sum(self.loo_log_predictive_densities()))
