"""Batched evaluation of StateSpaceGP: the likelihood, the posterior and the exact gradient at B hyper-parameter settings over
one series (`ModelBatches`, a mixin of StateSpaceGP), with the host half they share: `thetas` checked, each row assigned to
the model in turn, the model's own parameters restored on every exit path.
"""
import contextlib

import numpy as np

from . import _backend, config
from ._evaluation import _single_output_evaluation, _zero_mean_evaluation
from .gradients import mask_wrt, matern_contract
from .kernels import Matern12, Matern32, Matern52, RBF


class ModelBatches:
    def _check_thetas(self, thetas):
        """`thetas` as a float64 (B, P) array (one setting may be given as a vector) and the model's trainable parameters."""
        thetas = np.asarray(thetas, np.float64)
        if thetas.ndim == 1:
            thetas = thetas[None, :]
        params = self.trainable_parameters()
        if thetas.ndim != 2 or thetas.shape[1] != len(params):
            raise ValueError(f"thetas has shape {thetas.shape}, the model {len(params)} trainable parameters: expected (B, {len(params)})")
        return thetas, params

    @staticmethod
    @contextlib.contextmanager
    def _parameters_restored(params):
        """The values of `params` at entry are assigned back on every exit path."""
        saved = [getattr(o, n) for o, n in params]
        try:
            yield
        finally:
            for (o, n), v in zip(params, saved):
                setattr(o, n, v)

    @staticmethod
    def _assign(params, row):
        """Row `row` of a batch becomes the model's setting."""
        for (o, n), v in zip(params, row):
            setattr(o, n, float(v))

    def _each_setting(self, thetas, visit):
        """The host half of a batched evaluation, shared by log_likelihood_batch and predict_f_batch: validates `thetas`
        (B, P), assigns each row to the model in turn and calls visit(b, form, F, P0, H) with the row's SDE -- `form` its
        nilpotent form (lam, N1, N2) or None -- and restores the model's own parameters on every exit path.  Economies:
        settings that differ in the noise only share one SDE; for a single Matern / RBF kernel the variance is a scaling
        of Pinf and a nearby lengthscale a scaling of time, so one SDE is built per lengthscale neighbourhood."""
        thetas, params = self._check_thetas(thetas)
        with self._parameters_restored(params):
            memo = {}                   # kernel parameters -> its SDE: settings that differ in the noise only share it
            first_with = {}             # the parameters after the variance -> the first setting that had them
            leaf_variance = isinstance(self.kernel, (Matern12, Matern32, Matern52, RBF)) and params[0] == (self.kernel, "variance")
            for b, row in enumerate(thetas):
                self._assign(params, row)
                key = tuple(float(v) for v in row[:-1])
                if key not in memo and leaf_variance and key[0] != 0.0:
                    # a single Matern / RBF kernel: F, H do not depend on its variance and Pinf is linear in it
                    # (balance_ss normalises L and H, q carries the scale) -- one SDE per lengthscale
                    other = first_with.get(key[1:])          # (the first setting built with these other parameters)
                    if other is not None:
                        fo, Fo, Po, Ho = memo[other]
                        memo[key] = (fo, Fo, Po * (key[0] / other[0]), Ho)
                if key not in memo and leaf_variance and key[0] != 0.0 and len(key) == 2 and key[1] > 0.0:
                    # ... and its lengthscale is a scaling of time: k(tau / l).  The state-space model at lengthscale l is
                    # the one at l0 with F multiplied by l0 / l (same Pinf / variance, same H) -- the same model as
                    # get_sde() builds, in a realisation that differs from it by a diagonal similarity where the
                    # balancing sweeps have not converged (RBF), i.e. the same likelihood up to rounding.  Used for nearby
                    # lengthscales only (the perturbations of a difference quotient, the steps of a sampler): one SDE
                    # construction (0.2 - 0.4 ms for RBF order 6) instead of one per row.
                    for other, (fo, Fo, Po, Ho) in list(memo.items()):
                        if other[0] != 0.0 and other[1] > 0.0 and 0.8 <= key[1] / other[1] <= 1.25:
                            r = other[1] / key[1]
                            form = None if fo is None else (fo[0] * r, fo[1] * r, fo[2] * (r * r))
                            memo[key] = (form, Fo * r, Po * (key[0] / other[0]), Ho)
                            break
                if key not in memo:
                    sde = self.kernel.get_sde()
                    memo[key] = (_backend.nilpotent_form(sde.F), np.asarray(sde.F, np.float64), np.asarray(sde.P0, np.float64),
                                 np.asarray(sde.H, np.float64).reshape(-1))
                if key[0] != 0.0:
                    first_with.setdefault(key[1:], key)
                form, F, P0, H = memo[key]
                visit(b, form, F, P0, H)
        return thetas.shape[0]

    @_zero_mean_evaluation
    @_single_output_evaluation
    def log_likelihood_batch(self, thetas):
        """Marginal log-likelihoods at B hyper-parameter settings in one call: `thetas` is (B, P) in the
        order of `trainable_parameters()`.  The B filters share the series and run side by side on
        the GPU (pgps_gp_ll_batch_*) -- the evaluation pattern of the reference's HMC / grid-search
        drivers (pssgp/experiments/*/mcmc.py), which loop over maximum_log_likelihood_objective."""
        if not self.parallel:
            raise NotImplementedError("batched evaluation runs on the parallel (HIP) path: construct with parallel=True")
        models, general = [], []
        ts, Y = self.data
        stream = [None]                 # state dimensions 17..32: asynchronous single evaluations, see below
        n_rows = np.atleast_2d(np.asarray(thetas)).shape[0]

        def visit(b, form, F, P0, H):
            if form is not None:
                models.append((form, P0, H, self.noise_variance))
            d = F.shape[0]
            if _backend.LTI_BATCH_DIM_MAX < d <= _backend.LTI_DIM_MAX:
                # one device evaluation per setting on the wave-cooperative kernels, enqueued as soon as its model
                # exists: the device runs setting i while the host builds the SDE of setting i + 1
                if stream[0] is None:
                    stream[0] = _backend.LtiLlStream(ts.reshape(-1), Y.reshape(-1), n_rows)
                stream[0].push(F, P0, H, self.noise_variance)
                return
            # kernels without the closed-form discretisation (RBF, Periodic, sums, products): general-LTI batch
            general.append((F, P0, H, self.noise_variance))

        try:
            n_rows = self._each_setting(thetas, visit)
            if stream[0] is not None:
                if stream[0].count != n_rows:
                    raise ValueError("all settings of a batch must give the same state dimension")
                out, stream[0] = stream[0].finish(), None
                return out
        finally:
            if stream[0] is not None:
                stream[0].close()
        if len(models) == len(general):
            return _backend.gp_ll_batch(models, ts.reshape(-1), Y.reshape(-1))
        d = general[0][0].shape[0]
        if _backend.LTI_DIM_MIN <= d <= _backend.LTI_BATCH_DIM_MAX:
            ser = self._device_series() if ts.dtype == np.float64 else None
            if ser is not None and ser.has_lti:
                return ser.lti_ll_batch(general)
            return _backend.lti_ll_batch(general, ts.reshape(-1), Y.reshape(-1))
        raise NotImplementedError(f"batched evaluation covers the Matern family and state dimensions "
                                  f"{_backend.LTI_DIM_MIN}..{_backend.LTI_DIM_MAX}; this kernel has d = {d}")

    @staticmethod
    def _mixture_weights(weights, B):
        """`weights` normalised to sum 1 (None: equal), validated: one per setting, none negative, not all zero."""
        if weights is None:
            return np.full(B, 1.0 / B)
        w = np.asarray(weights, np.float64).reshape(-1)
        if w.shape[0] != B:
            raise ValueError(f"weights has {w.shape[0]} entries, thetas {B} rows")
        if not np.all(np.isfinite(w)) or np.any(w < 0.0) or not w.sum() > 0.0:
            raise ValueError("weights must be finite, non-negative and not all zero")
        return w / w.sum()

    @staticmethod
    def _mix_moments_host(mean, var, w):
        """Moments of sum_b w_b N(mean_b, var_b), (B, K) -> (K,), (K,): the two-pass form, every term of the variance
        non-negative (what k_mix_moments computes on the device)."""
        mix = np.sum(w[:, None] * mean, axis=0)
        return mix, np.sum(w[:, None] * (var + (mean - mix[None, :]) ** 2), axis=0)

    @_zero_mean_evaluation
    @_single_output_evaluation
    def predict_f_batch(self, Xnew, thetas, return_log_likelihood=False, reduce=None, weights=None):
        """predict_f at B hyper-parameter settings over the same series and query grid: `thetas` is (B, P) in the order of
        `trainable_parameters()`.  Returns means (B, K, 1) and variances (B, K, 1) -- row b what predict_f(Xnew) returns
        with row b assigned to the model -- and, with return_log_likelihood=True, the B training log-likelihoods (the
        filter pass has them).  reduce="mixture": the moments (K, 1), (K, 1) of sum_b w_b N(mean_b, var_b) instead, w =
        `weights` normalised (None: equal): mean = sum_b w_b mean_b, var = sum_b w_b (var_b + (mean_b - mean)^2) -- the
        posterior predictive averaged over the draws of a chain (pssgp/experiments/sunspot/mcmc.py:78-97 loops predict_f
        over ten of them).  Xnew in any order, repeated times allowed.  The model's own parameters are restored on every
        exit path.

        parallel=True: a single Matern kernel (fp64 and float32 series) runs the B filters, smoothers and projections in
        one set of launches (pgps_gp_predict_batch_*, on the resident series from the model's second evaluation), and the
        mixture is reduced on the device (k_mix_moments): 2 K numbers come back.  Every other kernel (RBF, Periodic, sums,
        products) with 2 <= d <= 16 runs on the row-cooperative kernels, the B models side by side in the launches of one
        predict (pgps_lti_predict_batch_f64); d = 17 .. 32 takes asynchronous single calls; the SDEs are built as
        log_likelihood_batch builds them.  parallel=False: a host loop over the sequential path
        (_predict_f_host: fp64, discretised on the host), any kernel, no device."""
        if reduce not in (None, "mixture"):
            raise ValueError(f"reduce must be None or 'mixture', got {reduce!r}")
        thetas, params = self._check_thetas(thetas)
        B = thetas.shape[0]
        if reduce is None and weights is not None:
            raise ValueError("weights are the mixture's: pass reduce='mixture'")
        w = self._mixture_weights(weights, B) if reduce == "mixture" else None
        dtype = config.default_float()
        xq = np.asarray(Xnew, dtype=dtype).reshape(-1)
        K = xq.shape[0]
        if K <= 1 or np.all(xq[1:] > xq[:-1]):
            tq, inverse = xq, None                                # already sorted, each time once
        else:
            tq, inverse = np.unique(xq, return_inverse=True)
        rows = (lambda a: a) if inverse is None else (lambda a: a[..., inverse])
        device = self.parallel and K > 0
        if device and getattr(self, "_series", None) is None:     # (a resident series was checked when it was made)
            device = self._ts_sorted()
        mixed = None
        if not device:
            mean, var, lls = self._predict_f_batch_loop(tq, thetas, params, return_log_likelihood or K == 0)
        else:
            mean, var, lls, mixed = self._predict_f_batch_device(tq, thetas, params, w, return_log_likelihood)
        if reduce == "mixture":
            if mixed is None:
                mixed = self._mix_moments_host(np.asarray(mean, np.float64), np.asarray(var, np.float64), w)
            out = (rows(mixed[0])[:, None].astype(dtype, copy=False), rows(mixed[1])[:, None].astype(dtype, copy=False))
        else:
            out = (rows(mean)[:, :, None].astype(dtype, copy=False), rows(var)[:, :, None].astype(dtype, copy=False))
        if return_log_likelihood:
            out = out + (np.asarray(lls, dtype),)
        return out

    def _predict_f_batch_loop(self, tq, thetas, params, want_ll):
        """predict_f_batch as a loop over the settings: assign row b, predict on the sorted unique grid (and the
        log-likelihood).  parallel=False: _predict_f_host, no device; else predict_f and the objective (kernels and series
        the batched device calls do not take, and batches too small for them).  (B, K), (B, K), (B,) or None."""
        B, K = thetas.shape[0], tq.shape[0]
        dtype = config.default_float()
        mean, var = np.zeros((B, K), dtype), np.zeros((B, K), dtype)
        lls = np.zeros(B, dtype) if want_ll else None
        with self._parameters_restored(params):
            for b, row in enumerate(thetas):
                self._assign(params, row)
                if not self.parallel:
                    mean[b], var[b], ll = self._predict_f_host(tq)
                    if want_ll:
                        lls[b] = ll
                    continue
                if K > 0:
                    m, v = self.predict_f(tq[:, None])
                    mean[b], var[b] = m[:, 0], v[:, 0]
                if want_ll:
                    lls[b] = self.maximum_log_likelihood_objective()
        return mean, var, lls

    # predict_f_batch, Matern family: settings from which the batched launches replace the loop of single predicts.  Measured
    # (tools/predict_batch_bench.py --forms, MI355X, N = 3000, K = 2000, resident series, median [min, max] ms): B = 1 batched
    # 0.086 [0.083, 0.111] against the loop's 0.068 [0.062, 0.111]; B = 2 0.085 [0.083, 0.104] against 0.132 [0.128, 0.140] --
    # a call of the batch costs what ~1.3 single predicts do (profiles/predict_batch_bench.json).
    _PREDICT_BATCH_FROM = 2

    def _predict_f_batch_device(self, tq, thetas, params, w, want_ll):
        """The device half of predict_f_batch (sorted series, K > 0): (mean (B, K), var (B, K), lls (B,), mixture or None)."""
        B = thetas.shape[0]
        if B < self._PREDICT_BATCH_FROM and self._matern_forms() is not None:
            return self._predict_f_batch_loop(tq, thetas, params, want_ll) + (None,)     # the loop of single calls is faster
        ts, ys = self.data
        t, y = ts.reshape(-1), ys.reshape(-1)
        ser = self._device_series() if t.dtype == np.float64 else None
        if ser is not None:
            ser.set_queries(tq)
        table = self._matern_table(thetas, params)
        if table is not None:
            if ser is not None:
                return ser.gp_predict_batch(table, mix=w)
            return _backend.gp_predict_batch(table, t, y, tq.astype(t.dtype), mix=w)
        fused, general = [], []

        def visit(b, form, F, P0, H):
            if form is not None and F.shape[0] <= 3:
                fused.append((form, P0, H, self.noise_variance))
            general.append((F, P0, H, self.noise_variance))

        self._each_setting(thetas, visit)
        if len(fused) == B:                     # (a composite kernel whose SDE has the fused form)
            if ser is not None:
                return ser.gp_predict_batch(fused, mix=w)
            return _backend.gp_predict_batch(fused, t, y, tq.astype(t.dtype), mix=w)
        d = general[0][0].shape[0]
        if any(g[0].shape[0] != d for g in general):
            raise ValueError("all settings of a batch must give the same state dimension")
        if _backend.LTI_DIM_MIN <= d <= _backend.LTI_BATCH_DIM_MAX:
            # general-LTI kernels, fp64 arithmetic (a float32 series widened): the B models side by side on the
            # row-cooperative kernels
            if ser is not None and ser.has_lti:
                return ser.lti_predict_batch(general, mix=w)
            return _backend.lti_predict_batch(general, t, y, tq, mix=w)
        if _backend.LTI_BATCH_DIM_MAX < d <= _backend.LTI_DIM_MAX:
            # d = 17 .. 32 (the CO2 kernel): asynchronous single predicts, as LtiLlStream enqueues likelihoods
            return _backend.lti_predict_stream(general, t, y, tq) + (None,)
        # no device form for this kernel (d = 1 outside the Matern family, d > 32): the loop over predict_f
        return self._predict_f_batch_loop(tq, thetas, params, True) + (None,)

    # log_likelihood_and_grad_batch, single Matern kernel: settings from which the batched adjoint launches replace the loop of
    # single gradient calls.  To be the smallest B at which the batch's median lies below the loop's minimum, as
    # tools/grad_batch_bench.py reports it (`batch_from`); NOT MEASURED YET: 2 is the structural expectation -- a
    # batched call is the launches of one gradient, the loop those of B
    _GRAD_BATCH_FROM = 2

    @staticmethod
    def _matern_grad_contract(stats, table, names, lengthscales, variances):
        """The host half of the batched adjoint gradient of a single Matern kernel, over the whole batch with array
        operations: stats (B, 1 + d^2 + 2 d + 1) rows [ll | Abar | Ubar | Hbar | Rbar] of the device, table (B, 1 + 3 d^2 + d
        + 1) rows [lam | N1 | N2 | Pinf | H | R] of _matern_table, names the parameters' attribute names in the order of the
        gradient's columns.  The lengthscale scales time and the variance Pinf (as _fused_adjoint_ll_and_grad):
            d ll / d l = -<Abar, F> / l with F = N1 - lam I,   d ll / d s2 = Ubar . (Pinf H^T) / s2,   d ll / d R = Rbar.
        Returns grads (B, len(names))."""
        stats, table = np.asarray(stats, np.float64), np.asarray(table, np.float64)
        B = table.shape[0]
        d = {6: 1, 16: 2, 32: 3}[table.shape[1]]
        dd = d * d
        F = table[:, 1:1 + dd].copy()
        F[:, ::d + 1] -= table[:, :1]
        Pinf = table[:, 1 + 2 * dd:1 + 3 * dd].reshape(B, d, d)
        PH = np.einsum("bij,bj->bi", Pinf, table[:, 1 + 3 * dd:1 + 3 * dd + d])
        return matern_contract(stats[:, 1:1 + dd], stats[:, 1 + dd:1 + dd + d], stats[:, 1 + dd + 2 * d], F, PH, names,
                               np.asarray(lengthscales, np.float64), np.asarray(variances, np.float64))

    # ... every other kernel (general-LTI models, d = 2 .. 32)
    _GRAD_BATCH_FROM_LTI = 2

    def _general_grad_batch(self, thetas, params, ser):
        """The batched adjoint pass for kernels without the closed-form discretisation: every row's model and derivatives
        from _adjoint_prepared() under assignment and restore (rows that differ in the noise only share one), ONE device
        call for all rows (pgps_lti_ll_grad_batch_* at d <= 16, asynchronous single calls above), the contraction of
        _backend.contract_grad_stats per row.  (stats (B, 1 + d d + 2 d + 1), grads (B, P)), or (None, None) where the loop
        has to do it: the Matern family's own paths, a row without an adjoint rule, mixed state dimensions."""
        assert params[-1] == (self, "noise_variance")      # (the last column of thetas is R: the key below leaves it out)
        fused, lti = self._device_forms()
        if fused is not None or lti is None:
            return None, None
        rows, memo = [], {}
        with self._parameters_restored(params):
            for row in thetas:
                self._assign(params, row)
                key = tuple(float(v) for v in row[:-1])
                if key not in memo:
                    memo[key] = self._adjoint_prepared()
                if memo[key] is None:
                    return None, None
                rows.append(memo[key])
        d = rows[0][0].shape[0]
        if any(r[0].shape[0] != d for r in rows):
            return None, None
        models = [(F, P0, H, float(R)) for (F, P0, H, _), R in zip(rows, thetas[:, -1])]
        ts, Y = self.data
        if ser is not None and d <= _backend.LTI_BATCH_DIM_MAX:
            stats = ser.lti_ll_grad_batch(models)
        else:
            stats = _backend.lti_ll_grad_batch(models, ts.reshape(-1), Y.reshape(-1))
        grads = np.stack([_backend.contract_grad_stats(_backend.split_grad_stats(stats[b], d), rows[b][2], rows[b][3])
                          for b in range(len(rows))])
        return stats, grads

    def _ll_and_grad_batch_loop(self, thetas, params, wrt):
        """log_likelihood_and_grad_batch as a loop: assign row b, log_likelihood_and_grad (its automatic, exact method)."""
        B = thetas.shape[0]
        lls, grads = np.zeros(B), np.zeros((B, len(params)))
        with self._parameters_restored(params):
            for b, row in enumerate(thetas):
                self._assign(params, row)
                lls[b], grads[b] = self.log_likelihood_and_grad(wrt=wrt)
        return lls, grads

    @_zero_mean_evaluation
    @_single_output_evaluation
    def log_likelihood_and_grad_batch(self, thetas, wrt=None):
        """(lls (B,), grads (B, P)): the marginal log-likelihood and its exact gradient at B hyper-parameter settings,
        `thetas` (B, P) in the order of `trainable_parameters()`; row b is what log_likelihood_and_grad() returns with row b
        assigned.  Columns not in `wrt` are 0.  The model's own parameters are untouched on every exit path.  parallel=True.

        A single Matern-1/2, -3/2 or -5/2 kernel on a sorted float64 series from _GRAD_BATCH_FROM settings: ONE batched
        adjoint pass on the device (pgps_gp_ll_grad_adj_batch_*: every setting's filter pass and reverse pass side by side,
        on the resident series from the model's second evaluation), contracted over the batch by _matern_grad_contract.
        Every other kernel with an adjoint rule (one state dimension 2 .. 32 for all rows) from _GRAD_BATCH_FROM_LTI
        settings: _general_grad_batch (pgps_lti_ll_grad_batch_* up to d = 16, asynchronous single calls above).
        Everything else -- float32 or unsorted series, a row without an adjoint rule, mixed state dimensions, smaller
        batches, a library without the entry points -- is a loop over log_likelihood_and_grad; never differences unless
        that method picks them itself.  A row that is not positive raises ValueError."""
        if not self.parallel:
            raise NotImplementedError("gradients run on the parallel (HIP) path: construct with parallel=True")
        thetas, params = self._check_thetas(thetas)
        B = thetas.shape[0]
        ts, Y = self.data
        if not np.all(thetas > 0.0):            # (variances, lengthscales, periods: a row that is not positive has no model)
            bad = int(np.argmax(~np.all(thetas > 0.0, axis=1)))
            raise ValueError(f"every hyper-parameter must be positive: row {bad} of thetas is {thetas[bad]}")
        # the series the batched entry points take: float64 and sorted -- resident from the model's second evaluation, the
        # host arrays at its first
        ser, host_ok = None, False
        if ts.dtype == np.float64:
            ser = self._device_series()
            host_ok = ser is None and getattr(self, "_series", None) is not False and self._ts_sorted()
        stats = grads = None
        if ser is not None or host_ok:
            lib = _backend.load_library()
            table = self._matern_table(thetas, params) if B >= self._GRAD_BATCH_FROM else None
            if table is not None and hasattr(lib, "pgps_gp_ll_grad_adj_batch_f64"):
                stats = ser.gp_ll_grad_adj_batch(table) if ser is not None else \
                    _backend.gp_ll_grad_adj_batch(table, ts.reshape(-1), Y.reshape(-1))
                names = [n for _, n in params]
                grads = self._matern_grad_contract(stats, table, names, thetas[:, names.index("lengthscales")],
                                                   thetas[:, names.index("variance")])
            elif table is None and B >= self._GRAD_BATCH_FROM_LTI and hasattr(lib, "pgps_lti_ll_grad_batch_f64"):
                stats, grads = self._general_grad_batch(thetas, params, ser)
        if stats is not None:
            return stats[:, 0].astype(config.default_float()), mask_wrt(grads, wrt)
        return self._ll_and_grad_batch_loop(thetas, params, wrt)
