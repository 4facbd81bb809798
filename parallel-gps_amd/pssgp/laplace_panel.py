"""LaplaceStateSpaceGPPanel: Laplace inference (LaplaceStateSpaceGP: counts, on / off records) for S independent series, each
with its own time stamps and length, under one kernel -- the spike trains of many neurons, event counts per patient or sensor,
the count light curves of a survey.

The definition of every result is the loop: row s is what a LaplaceStateSpaceGP on series s alone returns.  That loop is also
the host twin (parallel=False, kernels other than a single Matern-1/2, -3/2 or -5/2, float32).  The device route -- parallel=True,
a single Matern kernel, float64 -- runs the mode search of ALL series in ONE call (_backend.panel.gp_panel_laplace_dev: one
workgroup per series with the whole damped Newton loop inside the kernel) on concatenated arrays that
live on the device; the modes, their variances and the sites stay there for the gradient and for predict_f, and nothing per row
comes back unless it is asked for (fit_modes, posterior_modes).  A series above _backend.PANEL_MAX_STEPS steps (counted merged
with its queries in predict_f) leaves the panel call: its own LaplaceStateSpaceGP evaluates it and the result is spliced back.
"""
import warnings

import numpy as np

from . import _backend, config
from .gradients import mask_wrt
from .laplace import LaplaceStateSpaceGP
from .likelihoods import Likelihood
from .model import StateSpaceGP
from .panel import _column


class LaplaceStateSpaceGPPanel:
    """LaplaceStateSpaceGPPanel(series, kernel, likelihood, parallel=True, tol=1e-8, max_iter=50).

    series: a list of S pairs (t_i, y_i) as StateSpaceGPPanel takes them (any order of times, NaN in y = missing).
    likelihood: one Likelihood, or a list of S of the same class (per-series Poisson exposures).

    `thetas` of the methods below is in the order of trainable_parameters() (the kernel's parameters; there is no noise
    variance): None = the panel's own parameters shared by all series, or (S, P) = one row per series.  The panel's own
    parameters are restored on every exit path.  max_iter: the search inside the kernel is capped at 1000 steps; a panel with
    max_iter outside 1 .. 1000 takes the loop of single models instead (S host-driven searches: correct, and S times slower).
    A search that does not converge keeps its last iterate; the panel then raises
    ONE RuntimeWarning that names how many series did not."""

    def __init__(self, series, kernel, likelihood, parallel=True, tol=1e-8, max_iter=50):
        self.kernel = kernel
        self.parallel = bool(parallel)
        self.tol = float(tol)
        self.max_iter = int(max_iter)
        self.fit_info = None
        self._panel_data = None
        self._likelihood_in = likelihood
        self.data = series

    # -- data ----------------------------------------------------------------------------------------------
    @property
    def data(self):
        return self._data

    @data.setter
    def data(self, series):
        series = list(series)
        if len(series) < 1:
            raise ValueError("a panel holds at least one series")
        liks = self._likelihood_in
        if isinstance(liks, Likelihood):
            liks = [liks] * len(series)
        else:
            liks = list(liks) if isinstance(liks, (list, tuple)) else [None]
            if not all(isinstance(l, Likelihood) for l in liks):
                raise TypeError("likelihood must be a pssgp.likelihoods.Likelihood or a list of them")
            if len(liks) != len(series):
                raise ValueError(f"likelihood has {len(liks)} entries, the panel {len(series)} series")
            if len({type(l) for l in liks}) != 1:
                raise ValueError("the likelihoods of a panel must be of one class")
        if not isinstance(liks[0], Likelihood):
            raise TypeError("likelihood must be a pssgp.likelihoods.Likelihood or a list of them")
        data, models = [], []
        for s, pair in enumerate(series):
            if len(pair) != 2:
                raise ValueError(f"series {s}: expected a pair (t, y)")
            t, y = _column(pair[0], "t", s), _column(pair[1], "y", s)
            if t.shape[0] < 1:
                raise ValueError(f"series {s} is empty")
            if y.shape[0] != t.shape[0]:
                raise ValueError(f"series {s}: t has {t.shape[0]} rows, y {y.shape[0]}")
            models.append(LaplaceStateSpaceGP((t[:, None], y[:, None]), self.kernel, liks[s], parallel=self.parallel, tol=self.tol,
                                              max_iter=self.max_iter))
            data.append((pair[0], pair[1]))
        self._release()
        self._data, self._models, self._liks = data, models, liks
        self.num_series = len(models)
        self._short = [s for s, m in enumerate(models) if m._t.shape[0] <= _backend.PANEL_MAX_STEPS]
        self._long = [s for s, m in enumerate(models) if m._t.shape[0] > _backend.PANEL_MAX_STEPS]
        self._fit = None

    @property
    def likelihood(self):
        return self._likelihood_in

    def _release(self):
        pd, self._panel_data = getattr(self, "_panel_data", None), None
        if pd is not None:
            pd.close()

    def __del__(self):
        try:
            self._release()
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass

    def _resident(self):
        """The short series (sorted), concatenated, on the device (made once per data assignment; owned by the panel)."""
        if self._panel_data is None:
            ms = [self._models[s] for s in self._short]
            offs = np.concatenate([[0], np.cumsum([m._t.shape[0] for m in ms])])
            self._panel_data = _backend.PanelData(offs, np.concatenate([m._t for m in ms]), np.concatenate([m._y for m in ms]))
        return self._panel_data

    # -- the kernel's forms and parameters --------------------------------------------------------------------
    def _helper(self):
        h = getattr(self, "_gp", None)
        if h is None or h.kernel is not self.kernel:
            h = self._gp = StateSpaceGP((np.zeros((1, 1)), np.zeros((1, 1))), self.kernel, noise_variance=0.0, parallel=True)
        return h

    def _fused(self):
        """(sde-like, form) where the device route applies, else None (the loop over the single models).  The kernel's search
        is capped at NEWTON_MAX_ITER_CAP = 1000 steps: a panel with max_iter outside 1 .. 1000 takes the loop, whose single
        models accept any max_iter (documented in the class's docstring and the README)."""
        if not self.parallel or config.default_float() != np.float64:
            return None
        if not 1 <= self.max_iter <= _backend.NEWTON_MAX_ITER_CAP:
            return None
        return self._helper()._matern_forms()

    def trainable_parameters(self):
        """[(owner, attribute name)] of the kernel's parameters, in the order of `thetas` and of the gradients."""
        return self._helper().trainable_parameters()[:-1]

    def _check_thetas(self, thetas):
        params = self.trainable_parameters()
        if thetas is None:
            return None, params
        thetas = np.asarray(thetas, np.float64)
        if thetas.ndim != 2 or thetas.shape != (self.num_series, len(params)):
            raise ValueError(f"thetas has shape {thetas.shape}: expected ({self.num_series}, {len(params)}), one row per series")
        return thetas, params

    def _synced(self, s):
        m = self._models[s]
        m.kernel = self.kernel
        m.tol, m.max_iter = self.tol, self.max_iter
        return m

    def _row(self, fused):
        sde, form = fused
        return np.concatenate([[float(form[0])], np.asarray(form[1], np.float64).reshape(-1), np.asarray(form[2], np.float64).reshape(-1),
                               np.asarray(sde.P0, np.float64).reshape(-1), np.asarray(sde.H, np.float64).reshape(-1), [0.0]])

    def _table(self, thetas, params):
        """The model table of the panel call (R = 0): one row at the current setting, or the rows of the short series' thetas."""
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

    def _pars(self):
        p = np.array([float(self._liks[s].par) for s in self._short], np.float64)
        return p[:1] if p.size and np.all(p == p[0]) else p

    def _each(self, thetas, params, visit, subset=None):
        """visit(s, single model of series s) with row s of thetas assigned (or the current setting), for s in subset."""
        out = {}
        for s in range(self.num_series) if subset is None else subset:
            if thetas is not None:
                StateSpaceGP._assign(params, thetas[s])
            out[s] = visit(s, self._synced(s))
        return out

    # -- the mode searches ---------------------------------------------------------------------------------------
    def _setting(self, thetas):
        return (self._helper()._param_key(), id(self.kernel), None if thetas is None else thetas.tobytes(),
                tuple((id(l), float(l.par)) for l in self._liks), self.parallel, self.tol, self.max_iter,
                str(config.default_float()))

    def _searched(self, thetas, params, rows):
        """The searches at this setting: {"info": S dicts, "log_evidence": (S,), "rows": None or S dicts of fit_mode}.  On the
        device route the per-row arrays stay on the device unless `rows`.  Cached by the setting; called with the parameters
        under _parameters_restored."""
        key = self._setting(thetas)
        fit = self._fit if self._fit is not None and self._fit[0] == key else None
        if fit is not None and (fit[1]["rows"] is not None or not rows):
            return fit[1]                   # (on the device route the modes of this setting are still in the PanelData)
        S = self.num_series
        info, ev, per = [None] * S, np.empty(S, np.float64), [None] * S
        fused = self._fused()
        alone = list(range(S)) if fused is None else self._long
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for s, (f, i) in self._each(thetas, params, lambda s, m: (m.fit_mode(), dict(m.fit_info)), alone).items():
                info[s], ev[s], per[s] = i, f["log_evidence"], f
        for w in caught:
            if not (issubclass(w.category, RuntimeWarning) and "did not converge" in str(w.message)):
                warnings.warn_explicit(w.message, w.category, w.filename, w.lineno)
        if fused is not None and self._short:
            data = self._resident()
            lik = self._liks[0]
            # the call replaces the sites the PanelData holds: whatever was cached for another setting is void from here on,
            # also when something below raises (the warning under -W error)
            self._fit = None
            out = _backend.panel.gp_panel_laplace_dev(data, self._table(thetas, params), lik.lik_id, self._pars(), self.tol,
                                                      self.max_iter, rows=rows)
            table = out["info"] if rows else out
            for i, s in enumerate(self._short):
                r = table[i]
                info[s] = {"iterations": int(r[3]), "halvings": int(r[4]), "converged": bool(r[5] != 0.0), "psi": float(r[2])}
                ev[s] = r[0] + r[1] + self._liks[s].log_prob_constant(self._models[s]._y)
                if rows:
                    a, b = int(data.offs[i]), int(data.offs[i + 1])
                    per[s] = {"f": out["f"][a:b], "v": out["v"][a:b], "z": out["zs"][a:b], "s": out["ss"][a:b],
                              "log_evidence": ev[s]}
        have_rows = all(p is not None for p in per)
        result = {"info": info, "log_evidence": ev, "rows": per if have_rows else None}
        self.fit_info = info
        self._fit = (key, result)           # (the cache and the device's sites now belong to the same setting: before the warning)
        bad = sum(not i["converged"] for i in info)
        if bad:
            warnings.warn(f"LaplaceStateSpaceGPPanel: the mode search of {bad} of {S} series did not converge in {self.max_iter} "
                          f"Newton steps (tol {self.tol:.3g})", RuntimeWarning, stacklevel=3)
        return result

    def fit_modes(self, thetas=None):
        """Runs the S mode searches (or returns the cached ones): a list of S dicts as LaplaceStateSpaceGP.fit_mode returns
        them -- "f", "v", "z", "s" (n_i,) fp64 in TIME order and "log_evidence".  fit_info is set: a list of S dicts."""
        thetas, params = self._check_thetas(thetas)
        with StateSpaceGP._parameters_restored(params):
            return self._searched(thetas, params, True)["rows"]

    def posterior_modes(self):
        """A list of S pairs (f^ (n_i, 1), var (n_i, 1)) in the order of the data rows."""
        dtype = config.default_float()
        fits = self.fit_modes()
        return [tuple(self._models[s]._in_data_order(fits[s][k])[:, None].astype(dtype) for k in ("f", "v"))
                for s in range(self.num_series)]

    # -- evaluations -----------------------------------------------------------------------------------------
    def log_evidences(self, thetas=None):
        """(S,): the Laplace approximation of the log evidence of every series."""
        thetas, params = self._check_thetas(thetas)
        with StateSpaceGP._parameters_restored(params):
            return self._searched(thetas, params, False)["log_evidence"].astype(config.default_float())

    def maximum_log_likelihood_objective(self):
        """The sum of the series' log evidences at the shared parameters (a population fit)."""
        return config.default_float()(np.sum(self.log_evidences()))

    def training_loss(self):
        return -self.maximum_log_likelihood_objective()

    @staticmethod
    def _single_grad(m):
        ll, g = m.log_likelihood_and_grad()
        return float(ll), np.asarray(g, np.float64)

    def _grad_rows(self, thetas, params):
        """(log evidences (S,), the adjoint rows of the short series) on the device route, the searches run first."""
        fit = self._searched(thetas, params, False)
        rows = None
        if self._short:
            rows = _backend.panel.gp_panel_laplace_grad_dev(self._resident(), self._table(thetas, params), self._liks[0].lik_id,
                                                            self._pars())
        return fit["log_evidence"], rows

    def log_evidences_and_grads(self, thetas=None):
        """((S,), (S, P)): every series' log evidence and its exact gradient with respect to trainable_parameters() (at row s
        of thetas where given).  Off the device route the single model's NotImplementedError is raised."""
        thetas, params = self._check_thetas(thetas)
        S, P = self.num_series, len(params)
        lls, grads = np.empty(S, np.float64), np.empty((S, P), np.float64)
        with StateSpaceGP._parameters_restored(params):
            fused = self._fused()
            if fused is None:
                for s, (ll, g) in self._each(thetas, params, lambda s, m: self._single_grad(m)).items():
                    lls[s], grads[s] = ll, g
                return lls.astype(config.default_float()), grads
            ev, rows = self._grad_rows(thetas, params)
            d = fused[1][1].shape[0]
            helper = self._helper()
            for i, s in enumerate(self._short):
                if thetas is not None:                  # (the contraction reads the kernel's setting: row s)
                    StateSpaceGP._assign(params, thetas[s])
                    fused = self._fused()
                lls[s] = ev[s]
                grads[s] = helper._host_adjoint_grad(fused, _backend.split_grad_stats(rows[i], d), None)[:-1]
            for s, (ll, g) in self._each(thetas, params, lambda s, m: self._single_grad(m), self._long).items():
                lls[s], grads[s] = ll, g
        return lls, grads

    def log_likelihood_and_grad(self, wrt=None):
        """(sum of the log evidences, its gradient) at the shared parameters.  On the device route the S adjoint rows are
        summed first and contracted once."""
        params = self.trainable_parameters()
        fused = self._fused()
        if fused is None:
            out = self._each(None, params, lambda s, m: self._single_grad(m))
            return (config.default_float()(np.sum([o[0] for o in out.values()])),
                    mask_wrt(np.sum([o[1] for o in out.values()], axis=0), wrt))
        ev, rows = self._grad_rows(None, params)
        ll, g = 0.0, np.zeros(len(params), np.float64)
        if self._short:
            d = fused[1][1].shape[0]
            ll += float(np.sum(ev[self._short]))
            g += self._helper()._host_adjoint_grad(fused, _backend.split_grad_stats(np.sum(rows, axis=0), d), None)[:-1]
        for s in self._long:
            l1, g1 = self._single_grad(self._synced(s))
            ll, g = ll + l1, g + g1
        return np.float64(ll), mask_wrt(g, wrt)

    def predict_f(self, Xnews, thetas=None):
        """A list of S pairs (mean (K_i, 1), var (K_i, 1)): the posterior of f under the approximation at Xnews[i] for series
        i.  Queries in any order, repeated times allowed; an empty Xnews[i] gives empty arrays."""
        Xnews = list(Xnews)
        if len(Xnews) != self.num_series:
            raise ValueError(f"Xnews has {len(Xnews)} entries, the panel {self.num_series} series")
        thetas, params = self._check_thetas(thetas)
        dtype = config.default_float()
        uniq = [np.unique(np.asarray(x, dtype=np.float64).reshape(-1), return_inverse=True) for x in Xnews]
        means = [np.zeros(0, dtype)] * self.num_series
        vars_ = [np.zeros(0, dtype)] * self.num_series

        def single(s, m):
            mean, var = m.predict_f(uniq[s][0][:, None])
            return np.asarray(mean).reshape(-1), np.asarray(var).reshape(-1)

        asked = [s for s in range(self.num_series) if uniq[s][0].size > 0]
        with StateSpaceGP._parameters_restored(params):
            if asked:
                self._searched(thetas, params, False)       # (the searches, and their one warning; the single models cache theirs)
            if self._fused() is None:
                alone = asked
            else:
                n_of = lambda s: self._models[s]._t.shape[0]
                inside = [s for s in self._short if uniq[s][0].size > 0 and n_of(s) + uniq[s][0].size <= _backend.PANEL_MAX_STEPS]
                keep = set(inside)
                alone = [s for s in asked if s not in keep]
                if inside:
                    counts = [uniq[s][0].size if s in keep else 0 for s in self._short]
                    qoffs = np.concatenate([[0], np.cumsum(counts)])
                    tq = np.concatenate([uniq[s][0] for s in self._short if s in keep])
                    mean, var = _backend.panel.gp_panel_laplace_predict_dev(self._resident(), self._table(thetas, params), qoffs, tq)
                    for i, s in enumerate(self._short):
                        if s in keep:
                            means[s], vars_[s] = mean[qoffs[i]:qoffs[i + 1]], var[qoffs[i]:qoffs[i + 1]]
            with warnings.catch_warnings():
                warnings.filterwarnings("ignore", message=".*did not converge.*", category=RuntimeWarning)
                for s, (mean, var) in self._each(thetas, params, single, alone).items():
                    means[s], vars_[s] = mean, var
        return [(np.asarray(means[s])[uniq[s][1].reshape(-1)][:, None].astype(dtype, copy=False),
                 np.asarray(vars_[s])[uniq[s][1].reshape(-1)][:, None].astype(dtype, copy=False)) for s in range(self.num_series)]

    def predict_y(self, Xnews, thetas=None):
        """A list of S pairs (mean, var) of a NEW observation at Xnews[i]: the likelihood's predict_mean_and_var over predict_f."""
        out = []
        for s, (mean, var) in enumerate(self.predict_f(Xnews, thetas)):
            m, v = self._liks[s].predict_mean_and_var(np.asarray(mean, np.float64), np.asarray(var, np.float64))
            out.append((m.astype(mean.dtype), v.astype(mean.dtype)))
        return out

    def predict_log_density(self, data, thetas=None):
        """A list of S arrays (K_i, 1): log p(Ynew | data) for data = a list of S pairs (Xnew_i, Ynew_i); NaN where Ynew is."""
        data = list(data)
        if len(data) != self.num_series:
            raise ValueError(f"data has {len(data)} entries, the panel {self.num_series} series")
        out = []
        for s, (mean, var) in enumerate(self.predict_f([d[0] for d in data], thetas)):
            ynew = np.asarray(data[s][1], np.float64).reshape(mean.shape)
            self._liks[s].validate(ynew)
            dens = self._liks[s].predict_log_density(np.asarray(mean, np.float64), np.asarray(var, np.float64), ynew)
            out.append(dens.astype(mean.dtype))
        return out
