"""LaplaceStateSpaceGP: GP models on one input (time) axis whose observations are NOT Gaussian -- event counts (Poisson), on / off
records (Bernoulli) -- by the Laplace approximation in state-space form (Rasmussen & Williams chapter 3).

The posterior mode f^ of f at the N training times is found by damped Newton steps.  One step is a Gaussian smoothing pass over
SITES: pseudo-observations z_k = f_k + g_k / W_k with variances s_k = 1 / W_k (g, W the first two derivatives of log p(y_k | f_k)):
    f+ = K (K + S)^-1 z,    alpha+ = K^-1 f+ = (z - f+) / s,    Psi(f) = sum_k log p(y_k | f_k) - f^T alpha / 2.
The step is damped on the segment between (f, alpha) and (f+, alpha+): a = 1, 1/2, 1/4, ... until Psi does not decrease.  At the
mode the evidence is the Gaussian log-likelihood of the sites plus a per-step correction,
    log q(y) = log N(z | 0, K + S) + sum_k [log p(y_k | f^_k) - log N(z_k | f^_k, s_k)],
predictions of f are those of the Gaussian model with observations z and per-step variances s, and the exact gradient of log q is
that of  G(z + w) - G(w) + G(0),  G(x) the Gaussian log-likelihood of observations x at FIXED s, w_k = v_k d3_k / (2 W_k).

parallel=True with a single Matern-1/2, -3/2 or -5/2 kernel: the device route -- every per-step array stays on the device, a step
is one call of _backend.SiteBuffers.newton (four launches) and brings six doubles back.  Everything else (parallel=False; RBF,
Periodic, sums, products): the host twin of the same loop on sequential.kf / ks, any kernel.
"""
import warnings

import numpy as np

from . import _backend, config
from ._backend.fused import _fused_model
from .kalman import sequential
from .likelihoods import Likelihood
from .model import StateSpaceGP, _host_discretise, _merge_queries, _project

_MAX_HALVINGS = 20
_PSI_SLACK = 1e-12


class LaplaceStateSpaceGP:
    """LaplaceStateSpaceGP(data, kernel, likelihood, parallel=True, tol=1e-8, max_iter=50).  data = (X (N,) or (N, 1), Y (N,) or
    (N, 1)); NaN rows of Y are missing observations.  Single output.  Times in any order: sorted once (stable), results come
    back in the order of the data rows.  Every evaluation runs in fp64 and is rounded to config.default_float() at the end.

    fit_mode() runs the Newton search from f = 0 and is cached until a kernel parameter, the kernel, the likelihood or the data
    is assigned; fit_info = {"iterations", "halvings", "converged", "psi"}.  A search that does not converge in max_iter steps
    warns (RuntimeWarning) and keeps its last iterate."""

    def __init__(self, data, kernel, likelihood, parallel=True, tol=1e-8, max_iter=50):
        if not isinstance(likelihood, Likelihood):
            raise TypeError("likelihood must be a pssgp.likelihoods.Likelihood")
        self.kernel = kernel
        self.likelihood = likelihood
        self.parallel = bool(parallel)
        self.tol = float(tol)
        self.max_iter = int(max_iter)
        self.num_latent_gps = 1
        self.fit_info = None
        self._fit = None
        self.data = data

    # -- data ----------------------------------------------------------------------------------------------
    @property
    def data(self):
        return self._data

    @data.setter
    def data(self, value):
        ts, ys = (np.asarray(a, dtype=config.default_float()) for a in value)
        ts = ts[:, None] if ts.ndim == 1 else ts
        ys = ys[:, None] if ys.ndim == 1 else ys
        if ts.ndim != 2 or ts.shape[1] != 1 or ys.shape != ts.shape or ts.shape[0] < 1:
            raise ValueError(f"data must be (X (N, 1), Y (N, 1)) with N >= 1, got shapes {ts.shape}, {ys.shape}")
        self.likelihood.validate(ys)
        t = np.asarray(ts, np.float64).reshape(-1)
        y = np.asarray(ys, np.float64).reshape(-1)
        self._order = None if np.all(np.diff(t) >= 0) else np.argsort(t, kind="stable")
        if self._order is not None:
            t, y = t[self._order], y[self._order]
        self._t, self._y = np.ascontiguousarray(t), np.ascontiguousarray(y)
        self._data = ts, ys
        self._fit = None

    def _in_data_order(self, a):
        if self._order is None:
            return a
        out = np.empty_like(a)
        out[self._order] = a
        return out

    # -- the kernel's forms --------------------------------------------------------------------------------
    def _helper(self):
        """A StateSpaceGP on no data of its own that holds the kernel: its memoised device forms and gradient contraction are
        the ones this model uses."""
        h = getattr(self, "_gp", None)
        if h is None or h.kernel is not self.kernel:
            h = self._gp = StateSpaceGP((np.zeros((1, 1)), np.zeros((1, 1))), self.kernel, noise_variance=0.0, parallel=True)
        return h

    def _fused(self):
        """(sde-like, form) of the device route, or None (the host twin)."""
        return self._helper()._matern_forms() if self.parallel else None

    def trainable_parameters(self):
        """[(owner, attribute name)] of the kernel's parameters, in the order of the gradient (the likelihoods have no
        trainable parameter)."""
        return self._helper().trainable_parameters()[:-1]

    def _setting(self):
        lik = self.likelihood
        return (self._helper()._param_key(), id(self.kernel), id(lik), float(lik.par), self.parallel, self.tol, self.max_iter)

    # -- the mode search -------------------------------------------------------------------------------------
    def _search(self, start, newton, halve, accept):
        """The damped Newton loop over three operations of a route (device buffers or host arrays):
          start()  -> (lp, fa, corr) of f = 0;   newton() -> the six sums of a pass from the current iterate into the proposal;
          halve()  -> (lp, fa, corr) of the proposal moved half way back to the current iterate;   accept() -> proposal := current.
        Returns (ll_sites, corr, info): the Gaussian log-likelihood of the sites at the accepted mode, the correction there."""
        lp, fa, corr = start()
        psi = lp - 0.5 * fa
        info = {"iterations": 0, "halvings": 0, "converged": False, "psi": float(psi)}
        move = np.nan
        for it in range(self.max_iter + 1):
            s = newton()
            if info["converged"]:
                # the closing pass from the accepted mode: its sites' log-likelihood and its variances are the mode's own
                # (the proposal it wrote moves by the square of the last step: below rounding)
                return float(s[0]), float(corr), info
            if it == self.max_iter:
                break
            move = s[4]
            lp, fa, c_new = s[1], s[2], s[3]
            psi_new = lp - 0.5 * fa
            halvings = 0
            while not (np.isfinite(psi_new) and psi_new >= psi - _PSI_SLACK * abs(psi)) and halvings < _MAX_HALVINGS:
                lp, fa, c_new = halve()
                psi_new = lp - 0.5 * fa
                halvings += 1
            accept()
            psi, corr = psi_new, c_new
            info["iterations"] = it + 1
            info["halvings"] += halvings
            info["psi"] = float(psi)
            info["converged"] = bool(np.isfinite(move) and move <= self.tol)
        warnings.warn(f"LaplaceStateSpaceGP: the mode search did not converge in {self.max_iter} Newton steps "
                      f"(last move {move:.3g}, tol {self.tol:.3g})", RuntimeWarning, stacklevel=3)
        return float(s[0]), float(corr), info

    def _fit_device(self, fused):
        sde, form = fused
        d, model = _fused_model(form, np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1))
        lik = self.likelihood
        buf = _backend.SiteBuffers(self._t, self._y, lik.lik_id, lik.par)
        try:
            with buf.ctx.lock:
                ll_sites, corr, info = self._search(lambda: buf.start(), lambda: buf.newton(model, d), buf.halve, buf.accept)
                # the closing pass wrote the mode's variances (and an iterate equal to the mode to rounding) into the proposal
                out = {"f": buf.fetch("f"), "v": buf.fetch("v", proposal=True), "z": buf.fetch("zs"), "s": buf.fetch("ss")}
        finally:
            buf.close()
        return ll_sites, corr, info, out

    def _host_ssm(self, t):
        sde = self.kernel.get_sde()
        h = np.asarray(sde.H, np.float64).reshape(-1)
        P0 = np.asarray(sde.P0, np.float64)
        Fs, Qs = _host_discretise(sde.F, P0, t)
        return (P0, Fs, Qs, h[None, :], np.zeros((1, 1))), h

    def _fit_host(self):
        """The host twin: the same loop on sequential.kf / ks with observation_variances = s and R = 0."""
        lik, y = self.likelihood, self._y
        obs = ~np.isnan(y)
        ssm, h = self._host_ssm(self._t)
        y0 = np.where(obs, y, 0.0)
        st = {}

        def sites(f, alpha):
            lp, g, W, _ = lik.log_prob_derivs(y0, f)
            s = np.where(obs, 1.0 / W, 1.0)
            z = np.where(obs, f + g / W, np.nan)
            corr = np.sum((lp + 0.5 * (np.log(2.0 * np.pi) - np.log(W) + g * g / W))[obs])
            return {"f": f, "alpha": alpha, "z": z, "s": s}, (float(np.sum(lp[obs])), float(f @ alpha), float(corr))

        def start():
            st["cur"], sums = sites(np.zeros_like(y), np.zeros_like(y))
            return sums

        def newton():
            c = st["cur"]
            fms, fPs, ll, mps, Pps = sequential.kf(ssm, c["z"], return_loglikelihood=True, return_predicted=True,
                                                   observation_variances=c["s"])
            sms, sPs = sequential.ks(ssm, fms, fPs, mps, Pps)
            f = sms @ h
            alpha = np.where(obs, (np.where(obs, c["z"], 0.0) - f) / c["s"], 0.0)
            st["new"], (lp, fa, corr) = sites(f, alpha)
            st["new"]["v"] = np.einsum("i,nij,j->n", h, sPs, h)
            return np.array([float(ll), lp, fa, corr, float(np.max(np.abs(f - c["f"]))), float(np.sum(obs))])

        def halve():
            c, p = st["cur"], st["new"]
            v = p["v"]
            st["new"], sums = sites(c["f"] + 0.5 * (p["f"] - c["f"]), c["alpha"] + 0.5 * (p["alpha"] - c["alpha"]))
            st["new"]["v"] = v
            return sums

        def accept():
            st["cur"], st["new"] = st["new"], st["cur"]

        ll_sites, corr, info = self._search(start, newton, halve, accept)
        c = st["cur"]
        return ll_sites, corr, info, {"f": c["f"], "v": st["new"]["v"], "z": c["z"], "s": c["s"]}

    def fit_mode(self):
        """Runs the mode search (or returns the cached one): a dict with the mode "f", its posterior variances "v" and the
        sites "z", "s" at it -- (N,) fp64 in TIME order -- and "log_evidence".  fit_info is set."""
        key = self._setting()
        if self._fit is not None and self._fit[0] == key:
            return self._fit[1]
        fused = self._fused()
        ll_sites, corr, info, out = self._fit_host() if fused is None else self._fit_device(fused)
        out["log_evidence"] = ll_sites + corr + self.likelihood.log_prob_constant(self._y)
        self.fit_info = info
        self._fit = (key, out)
        return out

    # -- evaluations ---------------------------------------------------------------------------------------
    def posterior_mode(self):
        """(f^ (N, 1), var (N, 1)): the mode of the posterior of f at the training times and the variances of the Gaussian
        approximation there, in the order of the data rows."""
        fit = self.fit_mode()
        dtype = config.default_float()
        return tuple(self._in_data_order(fit[k])[:, None].astype(dtype) for k in ("f", "v"))

    def maximum_log_likelihood_objective(self):
        """The Laplace approximation of the log evidence log p(y) at the current hyper-parameters."""
        return config.default_float()(self.fit_mode()["log_evidence"])

    def training_loss(self):
        return -self.maximum_log_likelihood_objective()

    def log_likelihood_and_grad(self, wrt=None):
        """(log evidence, its exact gradient in the order of trainable_parameters()): the explicit part at fixed sites plus the
        implicit part through the mode (R&W section 5.5.1), as the gradient of G(z + w) - G(w) + G(0) -- three calls of the
        per-observation-noise adjoint pass at R = 0, their statistics combined BEFORE the one contraction.  The device route
        only (NotImplementedError elsewhere, as with observation_variances)."""
        fused = self._fused()
        if fused is None:
            raise NotImplementedError("gradients of the Laplace evidence need parallel=True and a single Matern-1/2, -3/2 or "
                                      "-5/2 kernel")
        fit = self.fit_mode()
        y, f, v, z, s = self._y, fit["f"], fit["v"], fit["z"], fit["s"]
        obs = ~np.isnan(y)
        _, _, W, d3 = self.likelihood.log_prob_derivs(np.where(obs, y, 0.0), f)
        w = np.where(obs, 0.5 * v * d3 / W, np.nan)
        sde, form = fused
        P0, H = np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1)
        total = None
        for sign, x in ((1.0, z + w), (-1.0, w), (1.0, np.where(obs, 0.0, np.nan))):
            stats = _backend.gp_ll_grad_adj_het(form, P0, H, 0.0, self._t, x, s)
            total = [sign * np.asarray(a) for a in stats] if total is None else [a + sign * np.asarray(b) for a, b in zip(total, stats)]
        helper = self._helper()
        g = helper._host_adjoint_grad(fused, tuple(total), None)[:-1]           # (the last entry is noise_variance's: there is none)
        if wrt is not None:
            from .gradients import mask_wrt
            g = mask_wrt(g, wrt)
        return config.default_float()(fit["log_evidence"]), g

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False):
        """Mean (K, 1) and variance (K, 1) of f at Xnew under the Gaussian approximation: predict_f of the Gaussian model with
        observations z and per-step variances s (any order of Xnew)."""
        if full_cov or full_output_cov:
            raise NotImplementedError("LaplaceStateSpaceGP.predict_f covers the marginals (full_cov = full_output_cov = False)")
        dtype = config.default_float()
        xq = np.asarray(Xnew, np.float64).reshape(-1)
        if xq.size == 0:
            return np.zeros((0, 1), dtype), np.zeros((0, 1), dtype)
        fit = self.fit_mode()
        tq, inverse = np.unique(xq, return_inverse=True)
        fused = self._fused()
        if fused is not None:
            sde, form = fused
            mean, var, _ = _backend.gp_predict_het(form, sde.P0, sde.H, 0.0, self._t, fit["z"], fit["s"], tq)
        else:
            all_ts, all_z, all_s, flags = _merge_queries(self._t, fit["z"][:, None], tq, (fit["s"], np.full(tq.shape, np.nan)))
            ssm, h = self._host_ssm(all_ts)
            sms, sPs = sequential.kfs(ssm, all_z, observation_variances=all_s)
            mean, var = _project(sms, sPs, flags, h)
        return mean[inverse][:, None].astype(dtype), var[inverse][:, None].astype(dtype)

    def predict_y(self, Xnew, full_cov=False, full_output_cov=False):
        """Mean (K, 1) and variance (K, 1) of a NEW observation at Xnew: the likelihood's predict_mean_and_var over predict_f."""
        mean, var = self.predict_f(Xnew, full_cov=full_cov, full_output_cov=full_output_cov)
        m, v = self.likelihood.predict_mean_and_var(np.asarray(mean, np.float64), np.asarray(var, np.float64))
        return m.astype(mean.dtype), v.astype(mean.dtype)

    def predict_log_density(self, data, full_cov=False, full_output_cov=False):
        """log p(Ynew | data) at Xnew for data = (Xnew, Ynew), (K, 1): the likelihood averaged over predict_f's law; NaN where
        Ynew is."""
        Xnew, Ynew = data
        mean, var = self.predict_f(Xnew, full_cov=full_cov, full_output_cov=full_output_cov)
        Ynew = np.asarray(Ynew, np.float64).reshape(mean.shape)
        self.likelihood.validate(Ynew)
        out = self.likelihood.predict_log_density(np.asarray(mean, np.float64), np.asarray(var, np.float64), Ynew)
        return out.astype(mean.dtype)
