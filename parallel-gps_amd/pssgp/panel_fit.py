"""StateSpaceGPPanel.fit_each: every series' own hyper-parameter fit.

`PanelFitting` is a mixin of StateSpaceGPPanel.  The rule is csrc/pgps_fit.h (projected BFGS over x = log theta).  Two routes run it:
the launch (pgps_gp_panel_fit_dev_f64: one workgroup per series runs the whole search on the device) and the twin
(fitting.bfgs_box in lock step, one evaluation of all series per step).  The twin also serves what leaves the launch: series
above the panel's step limit, kernels other than a single Matern-1/2, -3/2, -5/2.
"""
import warnings

import numpy as np

from . import _backend, fitting
from .forms import _MATERN_DIMS
from .gradients import matern_contract
from .model import StateSpaceGP

_FIT_NAMES = ["variance", "lengthscales", "noise_variance"]      # the launch's theta, in this order


class PanelFitting:
    """fit_each and what it is made of (reads the panel's _models, _short, _long, _resident, _helper, _fused)."""

    def _fit_arguments(self, thetas0, wrt, bounds):
        """(theta0, lo, hi (S, P) float64, free (P,) bool), validated."""
        params = self.trainable_parameters()
        S, P = self.num_series, len(params)
        if thetas0 is None:
            theta0 = np.tile(np.array([float(getattr(o, n)) for o, n in params], np.float64), (S, 1))
        else:
            theta0 = np.array(self._check_thetas(thetas0)[0], np.float64)
        free = np.ones(P, bool)
        if wrt is not None:
            idx = [int(i) for i in wrt]
            if any(not 0 <= i < P for i in idx):
                raise ValueError(f"wrt holds an index outside 0 .. {P - 1}: {list(wrt)}")
            free[:] = False
            free[idx] = True
        if bounds is None:
            lo, hi = theta0 * 1e-4, theta0 * 1e4
        else:
            if len(bounds) != 2:
                raise ValueError("bounds must be a pair (lower, upper)")
            lo, hi = (np.asarray(b, np.float64) for b in bounds)
            for name, b in (("lower", lo), ("upper", hi)):
                if b.shape not in ((P,), (S, P)):
                    raise ValueError(f"bounds: {name} must be ({P},) or ({S}, {P}), got shape {b.shape}")
            lo, hi = np.broadcast_to(lo, (S, P)).copy(), np.broadcast_to(hi, (S, P)).copy()
        fr = free[None, :]
        pos = lambda a: np.isfinite(a) & (a > 0.0)
        if not np.all(np.where(fr, pos(theta0) & pos(lo) & pos(hi), True)):
            raise ValueError("fit_each: the start and the bounds of a free parameter must be finite and > 0")
        if not np.all(np.where(fr, lo < hi, True)):
            raise ValueError("fit_each: a free parameter needs lower < upper")
        fixed_noise = [i for i, (_, n) in enumerate(params) if n == "noise_variance" and not free[i]]
        fixed = theta0[:, [i for i in range(P) if not free[i] and i not in fixed_noise]]
        if not np.all(pos(fixed)):
            raise ValueError("fit_each: a fixed kernel parameter must be finite and > 0")
        for i in fixed_noise:
            R = theta0[:, i]
            if not np.all(np.isfinite(R) & (R >= 0.0)) or (self._obs_in is None and not np.all(R > 0.0)):
                raise ValueError("fit_each: a fixed noise_variance must be > 0 (>= 0 with observation_variances)")
        lo, hi = np.where(fr, lo, theta0), np.where(fr, hi, theta0)
        return theta0, lo, hi, free

    def _n_obs(self):
        return np.array([int(np.count_nonzero(~np.isnan(m.data[1]))) for m in self._models], np.float64)

    def _short_lls_and_grads(self, thetas, params):
        """(lls, grads) of the short series at their rows of `thetas` (len(_short), 3) by array operations: the table from
        ModelForms._matern_table, ONE panel call, the 2-D form of matern_contract.  None where the array forms do not apply."""
        helper = self._helper()
        table = helper._matern_table(thetas, params)
        if table is None:
            return None
        d = _MATERN_DIMS[type(self.kernel).__name__]
        dd = d * d
        rows = _backend.panel.gp_panel_ll_grad_dev(self._resident(), table)
        F = table[:, 1:1 + dd].copy()
        F[:, ::d + 1] -= table[:, :1]                            # F = N1 - lam I
        Pinf, H = table[:, 1 + 2 * dd:1 + 3 * dd].reshape(-1, d, d), table[:, 1 + 3 * dd:1 + 3 * dd + d]
        PH = np.einsum("bij,bj->bi", Pinf, H)
        grads = matern_contract(rows[:, 1:1 + dd], rows[:, 1 + dd:1 + dd + d], rows[:, 1 + dd + 2 * d], F, PH,
                                [n for _, n in params], thetas[:, 1], thetas[:, 0])
        return rows[:, 0].copy(), grads

    def _fit_twin(self, sub, lls_and_grads, theta0, lo, hi, free, n_obs, gtol, max_iter):
        """bfgs_box over the series `sub`: lls_and_grads(thetas (len(sub), P)) -> (lls, grads).  Rows of a PanelFit for `sub`."""
        t0, tlo, thi = theta0[sub], lo[sub], hi[sub]
        x0, xlo, xhi = fitting.log_box(t0, tlo, thi, free)
        scale = np.maximum(1.0, n_obs[sub])
        to_theta = lambda X: fitting.thetas_of(X, x0, xlo, xhi, t0, tlo, thi, free)

        def evaluate(X):
            th = to_theta(X)
            lls, grads = lls_and_grads(th)
            return -lls / scale, np.where(free[None, :], -(th * grads) / scale[:, None], 0.0)

        r = fitting.bfgs_box(evaluate, x0, xlo, xhi, free, gtol, max_iter)
        return to_theta(r.x), -r.f * scale, -r.f0 * scale, r.iterations, r.evaluations, r.status, r.grad_norm

    def fit_each(self, thetas0=None, wrt=None, bounds=None, gtol=1e-6, max_iter=100, in_kernel=True):
        """Fit every series' own hyper-parameters: maximise its log-likelihood over theta in the order of
        trainable_parameters(), inside a box, by the rule of csrc/pgps_fit.h (projected BFGS in log theta; converged when the
        largest component of the projected gradient of -ll / max(1, n_obs) in log theta is <= gtol).

        thetas0: None (every series starts at the panel's own setting) or (S, P).  wrt: the free parameters by index (None:
        all); the others keep their start value exactly.  bounds: None (start times [1e-4, 1e4] per free parameter) or
        (lower, upper), each (P,) or (S, P).  in_kernel=True: ONE launch per group runs all searches on the device (single
        Matern-1/2, -3/2, -5/2 kernel, float64, parallel=True; a series above the panel's step limit is fitted by the twin
        and spliced back); False: the twin, one device call per lock step.

        Returns a fitting.PanelFit: thetas (S, P), log_likelihoods, start_log_likelihoods, iterations, evaluations, status,
        grad_norm, (S,) each; status is one of fitting.STATUS_*.  The panel's own parameters are untouched.  ONE
        RuntimeWarning names how many series ended with a status other than STATUS_CONVERGED.  A series with no observed
        row returns its start (status 0, 0 iterations).  Where the single model has no gradient (parallel=False, float32),
        its NotImplementedError is raised."""
        if self._mean_function is not None:
            return self._residual_panel().fit_each(thetas0, wrt, bounds, gtol, max_iter, in_kernel)
        fitting.check_controls(gtol, max_iter)
        theta0, lo, hi, free = self._fit_arguments(thetas0, wrt, bounds)
        params = self.trainable_parameters()
        S, P = theta0.shape
        n_obs = self._n_obs()
        # thetas | ll | ll at the start | iterations | evaluations | status | grad_norm: the fields of fitting.PanelFit
        out = [np.empty((S, P)), np.empty(S), np.empty(S)] + [np.zeros(S, np.int64) for _ in range(3)] + [np.empty(S)]

        def put(sub, rows):
            for dst, src in zip(out, rows):
                dst[sub] = src

        with StateSpaceGP._parameters_restored(params):
            fused = self._fused()
            if fused is None:
                # the loop over the single models, all series in lock step (their NotImplementedError where they have no gradient)
                put(slice(None), self._fit_twin(np.arange(S), self.log_likelihoods_and_grads, theta0, lo, hi, free, n_obs, gtol,
                                                max_iter))
            else:
                short, long_ = np.array(self._short, int), np.array(self._long, int)
                launch = bool(in_kernel) and [n for _, n in params] == _FIT_NAMES
                if short.size and launch:
                    d = _MATERN_DIMS[type(self.kernel).__name__]
                    unit = None
                    if d == 3:
                        P1, H1, N1, N2 = self._helper()._matern52_unit
                        unit = np.concatenate([[1.0], N1.reshape(-1), N2.reshape(-1), P1.reshape(-1), H1.reshape(-1), [0.0]])
                    th, info = _backend.panel.gp_panel_fit_dev(self._resident(), d, unit, theta0[short], lo[short], hi[short],
                                                               free, gtol, max_iter)
                    ints = lambda c: np.rint(info[:, c]).astype(np.int64)
                    put(short, (th, info[:, 0], info[:, 1], ints(2), ints(3), ints(4), info[:, 5]))
                elif short.size:
                    def resident(th):
                        fast = self._short_lls_and_grads(th, params)
                        if fast is not None:
                            return fast
                        full = theta0.copy()
                        full[short] = th
                        lls, grads = self.log_likelihoods_and_grads(full)
                        return lls[short], grads[short]

                    put(short, self._fit_twin(short, resident, theta0, lo, hi, free, n_obs, gtol, max_iter))
                if long_.size:
                    def alone(th):
                        full = theta0.copy()
                        full[long_] = th
                        res = self._each(full, params, lambda s, m: self._single_grad(m), list(long_))
                        return np.array([res[s][0] for s in long_]), np.stack([res[s][1] for s in long_])

                    put(long_, self._fit_twin(long_, alone, theta0, lo, hi, free, n_obs, gtol, max_iter))
        fit = fitting.PanelFit(*out)
        bad = int(np.count_nonzero(fit.status != fitting.STATUS_CONVERGED))
        if bad:
            warnings.warn(f"fit_each: {bad} of {S} series ended with a status other than STATUS_CONVERGED "
                          f"(fitting.STATUS_NAMES; see the result's status)", RuntimeWarning, stacklevel=2)
        return fit
