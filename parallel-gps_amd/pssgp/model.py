"""StateSpaceGP: GP regression through the state-space form of the kernel.

Mirrors pssgp/model.py:58-117 of the reference: same constructor, `predict_f`,
`maximum_log_likelihood_objective`, `training_loss`; `parallel=True` runs the HIP
associative-scan path (csrc/), `parallel=False` the sequential host recursion.  Data and
results are numpy arrays; hyper-parameters are plain floats (no GPflow `Parameter`s); the
gradient of the log-likelihood comes from `log_likelihood_and_grad` (forward-mode duals inside
the scan kernels) instead of TensorFlow autodiff.

This module holds the model's data, the residency of its series on the device, the public evaluations and the routing
between their paths; the kernel's device forms are forms.py's, the gradient methods gradients.py's, the batched
evaluations batches.py's, the predictive checks checks.py's, the mean function's evaluations trend.py's, the functionals of the
state (additive components, derivatives) functionals.py's (mixins of the one class).
"""
import numpy as np

from . import _backend, config
from ._evaluation import _mean_function_route, _multi_output, _public_evaluation, _single_output_evaluation
from .batches import ModelBatches
from .checks import ModelChecks
from .forms import ModelForms
from .functionals import ModelFunctionals
from .gradients import ModelGradients, mask_wrt
from .kalman.parallel import pkf, pkfs
from .kalman import sequential
from .kalman.sequential import kf, kfs
from .trend import ModelTrend


def _merge_sorted(a, b, *args):
    """Merge two sorted 1-D arrays and any number of (a_x, b_x) payload pairs.

    As pssgp/model.py:15-55: the shorter array is scattered into the longer at
    arange + searchsorted(longer, shorter) (left side: on ties the shorter array's
    point comes first).
    """
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.ndim == b.ndim == 1
    if a.shape[0] < b.shape[0]:
        a, b = b, a
        args = tuple((j, i) for i, j in args)
    n_long, n_short = a.shape[0], b.shape[0]
    where_short = np.arange(n_short) + np.searchsorted(a, b, side="left")
    from_long = np.ones(n_long + n_short, dtype=bool)
    from_long[where_short] = False

    def weave(u, v):
        u, v = np.asarray(u), np.asarray(v)
        out = np.empty((n_long + n_short,) + u.shape[1:], dtype=np.result_type(u, v))
        out[from_long] = u
        out[where_short] = v
        return out

    return (weave(a, b),) + tuple(weave(i, j) for i, j in args)


def _merge_queries(ts, ys, tq, *payloads):
    """The training series (ts (N,), ys (N, M)) merged with the sorted query times tq (K,), as pssgp/model.py:92-105: the
    queries are missing observations (NaN rows of ys' dtype).  `payloads`: further (training values, query values) pairs.
    Returns (all_ts, all_ys, *merged payloads, flags), flags True at the query rows."""
    nan_ys = np.full((tq.shape[0], ys.shape[1]), np.nan, dtype=ys.dtype)
    return _merge_sorted(ts, tq, (ys, nan_ys), *payloads, (np.zeros(ts.shape, dtype=bool), np.ones(tq.shape, dtype=bool)))


def _project(sms, sPs, flags, H):
    """Mean and variance of f = H x at the query rows `flags` of the smoothed series: (K, 1), (K, 1) for H (1, d), the
    reference's layout; (K,), (K,) for the vector H (d,)."""
    if H.ndim == 1:
        return sms[flags] @ H, np.einsum("i,nij,j->n", H, sPs[flags], H)
    return sms[flags] @ H.T, np.einsum("ai,nij,aj->na", H, sPs[flags], H)


def _is_sorted(t):
    return np.all(np.diff(t) >= 0)


def _host_discretise(F, P0, ts, t0=0.0):
    """Fs[k] = expm(dt_k F), Qs[k] = sym(P0 - Fs[k] P0 Fs[k]^T) on the host in fp64 (P0 stationary), dts = diff([t0; ts]):
    what _backend.discretise computes on the device, for the evaluations that stay on the host throughout."""
    from scipy.linalg import expm
    F, P0 = np.asarray(F, np.float64), np.asarray(P0, np.float64)
    dts = np.diff(np.concatenate([[float(t0)], np.asarray(ts, np.float64).reshape(-1)]))
    d = F.shape[0]
    Fs, Qs = np.empty((dts.size, d, d)), np.empty((dts.size, d, d))
    seen = {}
    for k, dt in enumerate(dts):
        hit = seen.get(dt)
        if hit is None:
            Fk = expm(dt * F)
            Qk = P0 - Fk @ P0 @ Fk.T
            hit = seen[dt] = (Fk, 0.5 * (Qk + Qk.T))
        Fs[k], Qs[k] = hit
    return Fs, Qs


def _as_columns(data):
    """(ts (N, 1), ys (N, M)) of the default float from what the user gave."""
    ts, ys = (np.asarray(a, dtype=config.default_float()) for a in data)
    return (ts[:, None] if ts.ndim == 1 else ts), (ys[:, None] if ys.ndim == 1 else ys)


class StateSpaceGP(ModelForms, ModelGradients, ModelBatches, ModelChecks, ModelTrend, ModelFunctionals):
    """GP regression on one input (time) axis.  Y (N, 1) is the reference's model.

    THE FUSED ROUTE.  The evaluations below that name it run the fused HIP kernels on host arrays when: parallel=True, a single
    Matern-1/2, -3/2 or -5/2 kernel (_matern_forms), float64 data, non-empty sorted training times and -- where there are
    query times -- non-empty float64 sorted ones (_fused_route).  Nothing falls from it to another route on a failure (a
    PgpsError propagates).

    Y (N, M), M > 1, has GPflow's meaning of that layout: M independent GPs that share the kernel, the noise variance and the
    inputs; num_latent_gps = M is fixed at construction.  The fused route, and every row of Y observed in all columns or NaN in
    all columns: ONE covariance pass for all columns (_backend.gp_predict_multi / gp_ll_multi -- covariances, gains and
    innovation variances do not depend on y), and for log_likelihood_and_grad (method "adjoint", or method None where
    _multi_grad_pays() finds it cheaper) ONE filter pass and ONE reverse pass on column tiles (_backend.gp_ll_grad_multi).
    Everything else is the column loop: M internal single-column models that share the kernel object, built once per data
    assignment, correct for any missing pattern, M full passes.  predict_f_samples, predict_f_batch, log_likelihood_batch and
    log_likelihood_and_grad_batch are single-output.

    observation_variances (N,) or (N, 1), float64: data with error bars, y_k = f(t_k) + e_k, e_k ~ N(0, noise_variance + s_k) --
    s_k given (finite and >= 0 wherever y is observed; ignored, NaN allowed, at the NaN rows of y), noise_variance the one
    trainable jitter.  None (the default, and None assigned later) is the model with one shared noise variance, exactly.
    The fused route: the per-observation flavour of the fused kernels (_backend.gp_ll_het / gp_predict_het /
    gp_ll_grad_adj_het; never the resident series, which holds no s).  Everything else is the host twin: the sequential
    filter + smoother with a per-step variance (sequential.kf / kfs with observation_variances), any kernel, both modes --
    for maximum_log_likelihood_objective and predict_f; log_likelihood_and_grad (method None / "adjoint") exists on the
    fused route only.  predict_f(full_cov=True), the single-output evaluations above, gradient methods "dual" /
    "differences", gradients of other kernels and Y with more than one column raise NotImplementedError.

    mean_function (pssgp.mean_functions: Constant, Linear, Polynomial, Basis; m(t) = Phi(t) beta with p explicit basis functions,
    Rasmussen & Williams section 2.7): None (the default) is the zero-mean model, exactly -- no route, result or launch changes.
    With one set, every single-output evaluation above has GPflow's meaning at the CURRENT beta: the GP models y - m(t)
    (trend.py: delegation to one internal zero-mean model on the residuals; m added to returned means and draws and taken from
    the y side of densities).  whiten(V) returns the standardised innovations W = L^-1 V of columns over the training points
    (K + noise_variance I = L L^T), mean_gram() the Gram matrix G = V^T K_y^-1 V of V = [y, Phi] with logdet and the number of
    observed rows; from G alone: mean_coefficients() (the GLS estimate, its covariance, the profile log-likelihood),
    fit_mean_function(), log_marginal_likelihood_flat_mean() (R&W eq. 2.45), predict_f_gls() (eq. 2.41, 2.42: beta integrated out
    under a flat prior) and the entries d ll / d beta = b - A beta that log_likelihood_and_grad() appends after noise_variance's
    (trainable_parameters() lists them as (mean_function, "beta", j)).  The fused route: ONE covariance pass over the 1 + p
    columns with the whitened columns kept on the device and one Gram pass (_backend.gp_gram_multi, 1 + p <= 16; whiten():
    _backend.gp_whiten_multi, any number of columns; predict_f_gls: one _backend.gp_predict_multi call on [y, Phi]).
    Everything else -- parallel=False, float32, other kernels, times out of order, more columns -- is the host twin: the
    sequential filter's innovations column by column, any kernel.  Y with more than one column, observation_variances,
    log_likelihood_batch, log_likelihood_and_grad_batch and predict_f_batch (their thetas layout has no place for beta) raise
    NotImplementedError; a design matrix without full column rank on the observed rows raises ValueError.

    Functionals of the state (functionals.py): predict_components -- the posterior of every additive part of a sum kernel --,
    predict_f_derivative and predict_functionals (any C (J, d) over the state of kernel.get_sde()): mean (K, J) = C sm and
    cov (K, J, J) = C sP C^T at the query times.  parallel=True, sorted training times, 2 <= d <= 32, J <= 8: one device call
    (_backend.lti_predict_lin); everything else the host twin (_host_smoothed), any kernel.  Single-output models with one
    noise variance and no mean function."""

    def __init__(self, data, kernel, noise_variance=1.0, parallel=False, max_parallel=10000, observation_variances=None,
                 mean_function=None):
        self.noise_variance = float(noise_variance)
        self._obs_var = None
        self._mean_function = None
        ts, ys = _as_columns(data)
        if ys.ndim != 2 or ys.shape[1] < 1:
            raise ValueError(f"observations must be (N,) or (N, M) with M >= 1, got shape {ys.shape}")
        self.kernel = kernel
        self._data = ts, ys
        self.num_latent_gps = ys.shape[-1]
        self.parallel = bool(parallel)
        self.max_parallel = max_parallel
        if not parallel:
            self._kf = lambda ssm, y: kf(ssm, y, return_loglikelihood=True, return_predicted=False)
            self._kfs = kfs
        else:
            self._kf = lambda ssm, y: pkf(ssm, y, return_loglikelihood=True, max_parallel=ts.shape[0])
            self._kfs = lambda ssm, y: pkfs(ssm, y, max_parallel=max_parallel)
        self.observation_variances = observation_variances
        self.mean_function = mean_function

    @property
    def observation_variances(self):
        """The given per-observation noise variances s (N,), or None (class docstring)."""
        return self._obs_var

    @observation_variances.setter
    def observation_variances(self, value):
        if value is not None and self._mean_function is not None:
            raise NotImplementedError("observation_variances is not available with a mean_function set")
        self._obs_var = None if value is None else self._checked_obs_var(value, self._data[1])

    def _checked_obs_var(self, value, ys):
        if self.num_latent_gps > 1:
            raise NotImplementedError("observation_variances covers single-output models; this one has "
                                      f"{self.num_latent_gps} output columns")
        s = np.array(value, dtype=np.float64)
        if s.ndim == 2 and s.shape[1] == 1:
            s = s[:, 0]
        n = ys.shape[0]
        if s.ndim != 1 or s.shape[0] != n:
            raise ValueError(f"observation_variances must have shape ({n},) or ({n}, 1) like the data, got {np.shape(value)}")
        seen = s[~np.isnan(ys[:, 0])]
        if not (np.all(np.isfinite(seen)) and np.all(seen >= 0.0)):
            raise ValueError("observation_variances must be finite and >= 0 wherever y is observed")
        return np.ascontiguousarray(s)

    @property
    def data(self):
        return self._data

    @data.setter
    def data(self, value):
        """Assigning new data (the GPflow idiom `model.data = (X, Y)` the reference inherits) drops the device copy of
        the series and every memoised result; an IN-PLACE edit of the arrays is caught by the checksum of
        _device_series()."""
        ts, ys = _as_columns(value)
        if ys.ndim != 2 or ys.shape[1] != self.num_latent_gps:
            raise ValueError(f"the model has {self.num_latent_gps} output column(s) (fixed at construction), the new "
                             f"observations have shape {ys.shape}")
        if self._obs_var is not None:
            self._checked_obs_var(self._obs_var, ys)        # (length and values against the NEW data)
        self._data = ts, ys
        self._columns = None
        self.invalidate_device_series()

    # -- residency of the series on the device ----------------------------------------------------------
    @staticmethod
    def _data_stamp(ts, ys):
        """Identity and shape of the arrays a device copy was made from, plus the bytes of their last entries
        (O(1) per evaluation: a whole-array checksum would cost more than a short series' likelihood).  An in-place edit
        that misses every sampled entry is not seen: call invalidate_device_series() after such an edit."""
        return (id(ts), id(ys), ts.shape, ys.shape, ts[-1:].tobytes(), ys[-1:].tobytes())

    def _ts_sorted(self):
        """Non-empty training times in non-decreasing order?"""
        t = self.data[0].reshape(-1)
        return t.size >= 1 and _is_sorted(t)

    def _device_series(self, force=False):
        """The training series resident on the device (pgps_series_*, fp64 fused path): created at the SECOND evaluation of
        the model (or with force=True) and kept for its life -- an optimiser or sampler loop then sends only the model's
        scalars per evaluation.  The first evaluation goes through the host-array entry points, whose staging buffers belong
        to the context: a model that is built, evaluated once and dropped -- the reference's speed protocol,
        experiments/toy_models/speed_and_stability.py:73-87 -- would otherwise pay a set of device and pinned-host
        allocations per call (measured: Matern-3/2, N = K = 4096, model + predict_f 470 us against 175 us).  None when the
        data are not sorted or not float64 (the host entry points take those), and at that first evaluation."""
        ser = getattr(self, "_series", None)
        ts, ys = self.data
        if ser is not None and getattr(self, "_series_stamp", None) != self._data_stamp(ts, ys):
            self.invalidate_device_series()         # the arrays were replaced or edited since the copy was made
            ser = None
        if ser is None and not force and getattr(self, "_n_eval", 0) <= 1:
            return None                             # still inside the model's first evaluation (however many internal calls it makes)
        if ser is None:
            self._series_stamp = self._data_stamp(ts, ys)
            if ts.dtype != np.float64 or not self._ts_sorted():
                self._series = False
                return None
            try:
                self._series = _backend.Series(ts.reshape(-1), ys.reshape(-1))
            except RuntimeError:
                self._series = False
            ser = self._series
        return ser or None

    def invalidate_device_series(self):
        """The device copy of the series is rebuilt at the next evaluation and memoised likelihoods are dropped (done
        automatically when `data` is assigned or found edited)."""
        ser = getattr(self, "_series", None)
        if ser:
            ser.close()
        self._series = None
        self._series_stamp = None
        self._ll_memo = None

    def _memoised_ll(self, ser):
        """The log-likelihood the last prediction on `ser` left behind, if the model is still at that setting; else None."""
        memo = getattr(self, "_ll_memo", None)
        if (memo is not None and memo[2] is ser and memo[4] is self.kernel and memo[1] == float(self.noise_variance)
                and memo[0] == self._param_key()):
            return memo[3]
        return None

    def _memoise_ll(self, ser, ll):
        """The filter pass of a prediction IS the training log-likelihood -- the query rows are missing observations: an
        objective evaluated next at the same setting costs nothing.  (The setting's key is the one _device_forms() has just
        built or validated for this evaluation.)"""
        self._ll_memo = (self._forms_memo[0], float(self.noise_variance), ser, ll, self.kernel)

    # -- routes --------------------------------------------------------------------------------------------
    def _rows_all_or_none(self):
        """Every row of Y observed in all columns or NaN in all columns (then the columns share their covariances)?"""
        nan = np.isnan(self.data[1])
        return bool(np.all(nan.all(axis=1) == nan.any(axis=1)))

    def _fused_route(self, tq=None, complete_rows=False):
        """The fused model (sde-like, form) when the fused route of the class docstring applies (with complete_rows: and
        every row of Y is observed in all columns or in none), else None."""
        ts, ys = self.data
        if not self.parallel or ys.dtype != np.float64 or ts.shape[0] < 1:
            return None
        fused = self._matern_forms()
        if fused is None or not _is_sorted(ts.reshape(-1)):
            return None
        if tq is not None and (tq.size < 1 or tq.dtype != np.float64 or not _is_sorted(tq)):
            return None
        return fused if not complete_rows or self._rows_all_or_none() else None

    def _make_model(self, ts):
        R = np.reshape(np.asarray(self.noise_variance, dtype=config.default_float()), (1, 1))
        return self.kernel.get_ssm(ts, R)

    # -- several outputs on one clock (num_latent_gps > 1) -----------------------------------------
    def _column_models(self):
        """The column loop's M single-column models: they share the kernel object and follow the noise variance; built once
        per data assignment (and again when the arrays are found replaced or edited)."""
        ts, ys = self.data
        stamp = self._data_stamp(ts, ys)
        cols = getattr(self, "_columns", None)
        if cols is None or cols[0] != stamp:
            models = [StateSpaceGP((ts, np.ascontiguousarray(ys[:, j:j + 1])), self.kernel, self.noise_variance,
                                   parallel=self.parallel, max_parallel=self.max_parallel) for j in range(ys.shape[1])]
            cols = self._columns = (stamp, models)
        for m in cols[1]:
            m.kernel = self.kernel
            m.noise_variance = self.noise_variance
        return cols[1]

    def log_likelihood_columns(self):
        """The marginal log-likelihood of every output column, (M,); maximum_log_likelihood_objective() is their sum."""
        if self.num_latent_gps == 1:
            return np.asarray([self.maximum_log_likelihood_objective()], dtype=config.default_float())
        fused = self._fused_route(complete_rows=True)
        if fused is not None:
            sde, form = fused
            ts, Y = self.data
            return _backend.gp_ll_multi(form, sde.P0, sde.H, self.noise_variance, ts.reshape(-1), Y)
        return np.asarray([m.maximum_log_likelihood_objective() for m in self._column_models()], dtype=config.default_float())

    def _multi_objective(self):
        return config.default_float()(np.sum(self.log_likelihood_columns()))

    def _multi_predict_f(self, Xnew, full_cov=False, full_output_cov=False):
        """predict_f for M > 1: mean (K, M) and var (K, M) (on the fused route one variance, repeated, as GPflow returns
        it); full_cov=True: mean (K, M) and cov (M, K, K) -- computed once on the single-output path and broadcast (a read-only
        view) when the columns share their missing rows, per column otherwise."""
        del full_output_cov
        tq = np.asarray(Xnew, dtype=config.default_float()).reshape(-1)
        M = self.num_latent_gps
        if full_cov:
            mean, _ = self._multi_predict_f(Xnew)
            cols = self._column_models()
            if self._rows_all_or_none():
                cov = cols[0].predict_f(Xnew, full_cov=True)[1]
                return mean, np.broadcast_to(cov, (M,) + cov.shape[1:])
            return mean, np.concatenate([m.predict_f(Xnew, full_cov=True)[1] for m in cols], axis=0)
        fused = self._fused_route(tq, complete_rows=True)
        if fused is not None:
            sde, form = fused
            ts, Y = self.data
            mean, var, _ = _backend.gp_predict_multi(form, sde.P0, sde.H, self.noise_variance, ts.reshape(-1), Y, tq)
            return mean, np.repeat(var[:, None], M, axis=1)
        out = [m.predict_f(Xnew) for m in self._column_models()]
        return np.concatenate([o[0] for o in out], axis=1), np.concatenate([o[1] for o in out], axis=1)

    def _multi_ll_and_grad(self, wrt=None, method=None):
        """log_likelihood_and_grad for M > 1.  The fused route with complete rows and method "adjoint", or method None where
        _multi_grad_pays() says so: ONE call of _backend.gp_ll_grad_multi returns the columns' log-likelihoods and the model's
        adjoints summed over the columns (csrc/pgps_multi_grad.hip.h), contracted by _host_adjoint_grad.  Everything else: the
        sum of the per-column results (exact; M passes)."""
        fused = self._fused_route(complete_rows=True) if method in (None, "adjoint") else None
        if fused is not None and (method == "adjoint" or self._multi_grad_pays(self.data[0].shape[0], self.num_latent_gps)):
            sde, form = fused
            ts, Y = self.data
            stats = _backend.gp_ll_grad_multi(form, np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1),
                                              self.noise_variance, ts.reshape(-1), Y)
            return config.default_float()(np.sum(stats[0])), self._host_adjoint_grad(fused, stats, wrt)
        out = [m.log_likelihood_and_grad(wrt=wrt, method=method) for m in self._column_models()]
        return config.default_float()(np.sum([o[0] for o in out])), np.sum([o[1] for o in out], axis=0)

    # -- per-observation noise variances (class docstring) --------------------------------------------
    def _het_step_variances(self, dtype):
        """R_k = noise_variance + s_k of every step (the host twin's per-step argument; NaN wherever s is)."""
        return (np.float64(self.noise_variance) + self._obs_var).astype(dtype)

    def _het_objective(self):
        ts, Y = self.data
        fused = self._fused_route()
        if fused is not None:
            sde, form = fused
            return np.float64(_backend.gp_ll_het(form, sde.P0, sde.H, self.noise_variance, ts.reshape(-1), Y.reshape(-1),
                                                 self._obs_var))
        ssm = self._make_model(ts)
        return kf(ssm, Y, return_loglikelihood=True, observation_variances=self._het_step_variances(Y.dtype))[2]

    def _het_predict_f(self, Xnew):
        ts, ys = self.data
        tq = np.asarray(Xnew, dtype=config.default_float()).reshape(-1)
        squeezed_ts = ts.reshape(-1)
        fused = self._fused_route(tq)
        if fused is not None:
            sde, form = fused
            mean, var, _ = _backend.gp_predict_het(form, sde.P0, sde.H, self.noise_variance, squeezed_ts, ys.reshape(-1),
                                                   self._obs_var, tq)
            return mean[:, None], var[:, None]
        all_ts, all_ys, all_Rs, all_flags = _merge_queries(
            squeezed_ts, ys, tq, (self._het_step_variances(ys.dtype), np.full(tq.shape, np.nan, dtype=ys.dtype)))
        ssm = self._make_model(all_ts[:, None])
        sms, sPs = kfs(ssm, all_ys, observation_variances=all_Rs)
        return _project(sms, sPs, all_flags, np.asarray(ssm.H))

    def _het_ll_and_grad(self, wrt=None, method=None):
        """log_likelihood_and_grad with observation_variances set: the adjoint pass of the per-observation flavour
        (_backend.gp_ll_grad_adj_het; d ll / d noise_variance = Rbar = sum_k d ll / d R_k), contracted by _host_adjoint_grad.
        The fused route and method None / "adjoint" only; nothing falls back to differences."""
        if method not in (None, "adjoint"):
            raise NotImplementedError(f"method = {method!r} is not available with observation_variances set (None or 'adjoint')")
        fused = self._fused_route()
        if fused is None:
            raise NotImplementedError("gradients with observation_variances set need parallel=True, a single Matern-1/2, -3/2 or "
                                      "-5/2 kernel, float64 data and sorted times")
        sde, form = fused
        ts, Y = self.data
        stats = _backend.gp_ll_grad_adj_het(form, np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1),
                                            self.noise_variance, ts.reshape(-1), Y.reshape(-1), self._obs_var)
        return config.default_float()(stats[0]), self._host_adjoint_grad(fused, stats, wrt)

    # -- the public evaluations ------------------------------------------------------------------------
    @_mean_function_route("_trend_predict_f")
    @_multi_output("_multi_predict_f")
    @_public_evaluation
    def predict_f(self, Xnew, full_cov=False, full_output_cov=False):
        """Posterior mean (K, 1) and variance (K, 1) at `Xnew` (pssgp/model.py:92-111):
        merge train and query times, mark queries as missing, smooth, keep the query rows,
        project through H.  full_cov=True: the mean (K, 1) and the joint posterior covariance (1, K, K) of f(Xnew)
        (GPflow's [num_latent, K, K]; _predict_f_full_cov) -- the law of predict_f_samples' draws."""
        if self._obs_var is not None:
            if full_cov:
                raise NotImplementedError("predict_f(full_cov=True) is not available with observation_variances set")
            return self._het_predict_f(Xnew)
        if full_cov:
            return self._predict_f_full_cov(Xnew)
        ts, ys = self.data
        dtype = config.default_float()
        Xnew = np.asarray(Xnew, dtype=dtype)
        squeezed_ts = ts.reshape(-1)
        squeezed_Xnew = Xnew.reshape(-1)
        fused, lti = self._device_forms()
        # merge, missing-marking, filter + smoother and the projection through H at the query rows all on the device: K
        # means and variances come back, nothing else -- for sorted queries (and, on host arrays, sorted training times)
        device = (fused is not None or lti is not None) and squeezed_Xnew.size > 0 and _is_sorted(squeezed_Xnew)
        if device and fused is not None and dtype == np.float64:
            ser = self._device_series()
            if ser is not None:
                # series and query grid resident on the device (merged once): the call sends the model
                ser.set_queries(squeezed_Xnew)
                mean, var, ll = ser.gp_predict(self._packed_fused(fused), self.noise_variance)
                self._memoise_ll(ser, np.float64(ll))
                return mean[:, None], var[:, None]
        if device and fused is not None and _is_sorted(squeezed_ts):
            sde, form = fused
            mean, var, _ = _backend.gp_predict(form, sde.P0, sde.H, self.noise_variance, squeezed_ts, ys.reshape(-1),
                                               squeezed_Xnew)
            return mean[:, None], var[:, None]
        if device and lti is not None and _is_sorted(squeezed_ts):
            # kernels without the closed-form discretisation (RBF, Periodic, sums, products): the discretisation on the
            # device as well -- on the resident series where there is one
            ser = self._device_series() if squeezed_ts.dtype == np.float64 else None
            if ser is not None and ser.has_lti:
                ser.set_queries(squeezed_Xnew)
                mean, var, ll = ser.lti_predict(lti.F, lti.P0, lti.H, self.noise_variance)
                self._memoise_ll(ser, config.default_float()(ll))
                return mean[:, None].astype(dtype), var[:, None].astype(dtype)
            mean, var, _ = _backend.lti_predict(lti.F, lti.P0, lti.H, self.noise_variance, squeezed_ts, ys.reshape(-1),
                                                squeezed_Xnew)
            return mean[:, None].astype(dtype), var[:, None].astype(dtype)
        all_ts, all_ys, all_flags = _merge_queries(squeezed_ts, ys, squeezed_Xnew)
        if fused is not None:
            # times and observations straight into the scan kernels (Fs / Qs never materialised)
            sde, form = fused
            res = _backend.gp(form, sde.P0, sde.H, self.noise_variance, all_ts.astype(dtype), all_ys.reshape(-1),
                              want_smoothed=True)
            sms, sPs = res["sms"], res["sPs"]
            H = np.asarray(sde.H, dtype=dtype).reshape(1, -1)
        else:
            ssm = self._make_model(all_ts[:, None])
            sms, sPs = self._kfs(ssm, all_ys)
            H = np.asarray(ssm.H)
        return _project(sms, sPs, all_flags, H)

    def _host_smoothed(self, tq, data=None):
        """Merge with the (sorted) queries tq, discretisation (_host_discretise), sequential filter + smoother at the model's
        current setting on the host alone, fp64.  (ssm, h, fPs, sms, sPs, ll, flags): the query rows are missing
        observations and add nothing to the log-likelihood.  `data`: (ts, ys) to run on in place of the model's (a sorted
        copy of them)."""
        ts, ys = self.data if data is None else data
        all_ts, all_ys, all_flags = _merge_queries(np.asarray(ts, np.float64).reshape(-1), np.asarray(ys, np.float64),
                                                   np.asarray(tq, np.float64))
        sde = self.kernel.get_sde()
        h = np.asarray(sde.H, np.float64).reshape(-1)
        P0 = np.asarray(sde.P0, np.float64)
        Fs, Qs = _host_discretise(sde.F, P0, all_ts)
        ssm = (P0, Fs, Qs, h[None, :], np.reshape(np.float64(self.noise_variance), (1, 1)))
        fms, fPs, ll, mps, Pps = kf(ssm, all_ys, return_loglikelihood=True, return_predicted=True)
        sms, sPs = sequential.ks(ssm, fms, fPs, mps, Pps)
        return ssm, h, fPs, sms, sPs, float(ll), all_flags

    def _predict_f_host(self, tq):
        """predict_f and the training log-likelihood on the host alone (_host_smoothed): (mean (K,), var (K,), ll)."""
        _, h, _, sms, sPs, ll, flags = self._host_smoothed(tq)
        return _project(sms, sPs, flags, h) + (ll,)

    def _predict_f_full_cov(self, Xnew):
        """predict_f(Xnew, full_cov=True): mean (K, 1) and covariance (1, K, K), symmetric bit for bit, its diagonal the
        variances.  Cov(x_i, x_j | ys) = E_i .. E_{j-1} sP_j between query rows i < j of the merged series (E the smoother
        gains): no dense algebra over the training points.  parallel=True: merge, discretisation, filter +
        smoother, the products of the gains between the query rows and the fill on the device for any kernel with d <= 6
        (pgps_lti_predict_cov_f64; larger d raises PgpsError); parallel=False: _host_smoothed and sequential.ks_cov on the
        host, any d, no device needed.  Computed in fp64 and rounded to the default float.  Any order of Xnew; equal query
        times give equal rows and columns."""
        dtype = config.default_float()
        xq = np.asarray(Xnew, dtype=np.float64).reshape(-1)
        if xq.size == 0:
            return np.zeros((0, 1), dtype), np.zeros((1, 0, 0), dtype)
        tq, inverse = np.unique(xq, return_inverse=True)          # sorted, each time once
        if self.parallel:
            ts, ys = self.data
            sde = self.kernel.get_sde()
            mean, cov, ll = _backend.lti_predict_cov(sde.F, sde.P0, sde.H, self.noise_variance,
                                                     np.asarray(ts, np.float64).reshape(-1),
                                                     np.asarray(ys, np.float64).reshape(-1), tq)
        else:
            ssm, h, fPs, sms, sPs, _, flags = self._host_smoothed(tq)
            rows = np.flatnonzero(flags)
            mean = sms[rows] @ h
            cov = sequential.ks_cov(ssm, fPs, sPs, rows, H=h)
        return mean[inverse][:, None].astype(dtype), cov[np.ix_(inverse, inverse)][None].astype(dtype)

    @_mean_function_route("_trend_predict_f_samples")
    @_single_output_evaluation
    def predict_f_samples(self, Xnew, num_samples=None, full_cov=True, full_output_cov=False, seed=None):
        """Joint posterior draws of f at `Xnew` (GPflow's predict_f_samples): (S, K, 1), or (K, 1) when num_samples is
        None.  parallel=True: merge, discretisation, filter and a backward-sampling scan on the device for any kernel
        with d <= 6 (pgps_lti_sample_f64; larger d raises PgpsError); parallel=False: the host filter and its
        backward-sampling twin, any d.  Both use the library's draws under `seed` (None: a fresh 64-bit seed per call), so
        the two modes give the same samples at the same seed.  full_cov=False: independent draws from predict_f's
        marginals.  Any order of Xnew; equal query times get equal values.  The law of the joint draws is
        N(mean, cov) of predict_f(Xnew, full_cov=True), which the library returns without Monte Carlo."""
        del full_output_cov                 # (single output)
        dtype = config.default_float()
        S = 1 if num_samples is None else int(num_samples)
        if S < 1:
            raise ValueError(f"num_samples must be >= 1, got {num_samples}")
        if seed is None:
            seed = int(np.random.default_rng().integers(0, 2 ** 64, dtype=np.uint64))
        xq = np.asarray(Xnew, dtype=np.float64).reshape(-1)
        if not full_cov:
            mean, var = self.predict_f(Xnew)
            z = sequential.sample_normals(xq.shape[0], 1, S, seed)[:, :, 0]
            f = np.asarray(mean, np.float64)[:, 0] + np.sqrt(np.maximum(np.asarray(var, np.float64)[:, 0], 0.0)) * z
        else:
            tq, inverse = np.unique(xq, return_inverse=True)          # sorted, each time once
            ts, ys = self.data
            squeezed_ts = np.asarray(ts, np.float64).reshape(-1)
            if self.parallel:
                sde = self.kernel.get_sde()
                fq = _backend.lti_sample(sde.F, sde.P0, sde.H, self.noise_variance, squeezed_ts,
                                         np.asarray(ys, np.float64).reshape(-1), tq, S, seed)
            else:
                all_ts, all_ys, all_flags = _merge_queries(squeezed_ts, np.asarray(ys, np.float64), tq)
                ssm = self.kernel.get_ssm(all_ts[:, None], np.reshape(self.noise_variance, (1, 1)))
                ssm = tuple(np.asarray(a, np.float64) for a in ssm)
                fms, fPs = kf(ssm, all_ys)
                fq = sequential.ks_sample(ssm, fms, fPs, S, seed, H=np.asarray(ssm[3]).reshape(-1))[:, all_flags]
            f = fq[:, inverse]
        out = f[:, :, None].astype(dtype)
        return out[0] if num_samples is None else out

    @_mean_function_route("_trend_objective")
    @_multi_output("_multi_objective")
    @_public_evaluation
    def maximum_log_likelihood_objective(self):
        if self._obs_var is not None:
            return self._het_objective()
        ts, Y = self.data
        fused, lti = self._device_forms()
        if fused is not None:
            ser = self._device_series() if ts.dtype == np.float64 else None
            if ser is not None:
                ll = self._memoised_ll(ser)
                return np.float64(ser.gp_ll(self._packed_fused(fused), self.noise_variance)) if ll is None else ll
            sde, form = fused
            return _backend.gp(form, sde.P0, sde.H, self.noise_variance, ts.reshape(-1), Y.reshape(-1))["ll"]
        if lti is not None:
            ser = self._device_series() if ts.dtype == np.float64 else None
            if ser is not None and ser.has_lti:
                ll = self._memoised_ll(ser)
                return config.default_float()(ser.lti_ll(lti.F, lti.P0, lti.H, self.noise_variance)) if ll is None else ll
            ll = _backend.lti_ll(lti.F, lti.P0, lti.H, self.noise_variance, ts.reshape(-1), Y.reshape(-1))
            return config.default_float()(ll)
        ssm = self._make_model(ts)
        _, _, ll = self._kf(ssm, Y)
        return ll

    def trainable_parameters(self):
        """[(owner, attribute name)] in the order the gradient is returned: every leaf kernel's variance,
        lengthscale and period (the reference's gpflow Parameters: the Matern / RBF kernels' variance /
        lengthscales, Periodic's period and its base kernel's parameters, the leaves of sums and products in order),
        then the observation-noise variance (pssgp/model.py:68)."""
        self._param_key()                           # (validates the memoised structure of the kernel)
        params = list(self._struct_memo[2]) + [(self, "noise_variance")]
        if self._mean_function is not None:
            # ... then the mean function's coefficients, (owner, "beta", j): entries of one array
            params += [(self._mean_function, "beta", j) for j in range(np.shape(self._mean_function.beta)[0])]
        return params

    @_mean_function_route("_trend_ll_and_grad")
    @_multi_output("_multi_ll_and_grad")
    @_public_evaluation
    def log_likelihood_and_grad(self, wrt=None, method=None):
        """(ll, grad): the marginal log-likelihood and its gradient with respect to
        `trainable_parameters()` -- what the reference obtains from tf.GradientTape over
        maximum_log_likelihood_objective (tests/test_gp_vs_kfs.py:53-78).  parallel=True.  Matern family (d <= 3):
        ONE pass of the parallel filter on dual numbers, exact (Matern-5/2 above 2048 points: the adjoint pass, which
        is cheaper there).  Every other kernel (RBF, Periodic, sums, products,
        2 <= d <= 32): the ADJOINT pass -- one filter pass and one reverse pass on the device, exact, whatever the number
        of parameters (`_adjoint_ll_and_grad`).  `method`: None = automatic, "adjoint", "dual" (sums / products of Matern
        kernels up to d = 6 on dual numbers) or "differences" (Richardson central differences of batched likelihoods:
        the cross-checks of the tests); `wrt`: only these parameter indices, the others get 0."""
        if not self.parallel:
            raise NotImplementedError("gradients run on the parallel (HIP) path: construct with parallel=True")
        if method not in (None, "adjoint", "dual", "differences"):
            raise ValueError(f"method = {method!r}: None (automatic), 'adjoint', 'dual' or 'differences'")
        if self._obs_var is not None:
            return self._het_ll_and_grad(wrt, method)
        ts, Y = self.data
        fused, lti = self._device_forms()
        if method == "differences":
            # asked for by name: Richardson differences of batched likelihoods whatever the kernel (one evaluation at a
            # time where no batched entry point covers the state dimension)
            return self._lti_ll_and_grad(batched=(fused is not None or lti is not None), wrt=wrt)
        if fused is None and lti is not None and method in (None, "adjoint"):
            # every kernel without the closed-form discretisation: the adjoint pass (two passes whatever the number of
            # parameters); None when the kernel has no derivative rule or the library no such entry point
            out = self._adjoint_ll_and_grad(wrt)
            if out is not None:
                return out
            if method == "adjoint":
                raise NotImplementedError("no adjoint gradient for this kernel / library")
        if fused is None:
            # sums / products of Matern kernels (block-nilpotent drift, d <= 6): exact, dual numbers through the scan
            rows, sizes = (None, None)
            if (method in (None, "dual") and lti is not None and lti.F.shape[0] <= _backend.GRAD_BLOCKS_DIM_MAX
                    and not getattr(self, "_no_composite", False)):
                rows, sizes = self._grad_rows_composite()
            if rows is not None:
                ll, g = _backend.gp_ll_grad_blocks(rows, sizes, ts.reshape(-1), Y.reshape(-1))
                return ll, mask_wrt(g, wrt)
            if method == "dual":
                raise NotImplementedError("method = 'dual': this kernel is no sum / product of Matern kernels of d <= "
                                          f"{_backend.GRAD_BLOCKS_DIM_MAX} (use 'adjoint' or 'differences')")
            if method == "adjoint":
                raise NotImplementedError("no adjoint gradient for this kernel / library")
            # no dual-number path: batched differences on the general-LTI kernels (d <= 16), one evaluation at a
            # time above that (e.g. the CO2 kernel at its reference order, d = 18)
            return self._lti_ll_and_grad(batched=lti is not None, wrt=wrt)
        if method in (None, "adjoint") and ts.dtype == np.float64 and (method == "adjoint" or self._fused_adjoint_pays(ts.shape[0])):
            # the adjoint pass on the fused path's own kernels (csrc/pgps_gpadj.hip.h)
            out = self._fused_adjoint_ll_and_grad(fused, wrt)
            if out is not None:
                return out
        if (method in (None, "adjoint") and type(self.kernel).__name__ == "Matern52" and ts.dtype == np.float64
                and ts.shape[0] > self._MATERN52_ADJOINT_FROM):
            out = self._adjoint_ll_and_grad(wrt, prepared=self._matern_prepared(fused))
            if out is not None:
                return out
        if method == "adjoint":
            # asked for by name and not available on the fused path (float32 data, a library without the entry point, a series
            # that cannot be made resident): the general adjoint pass on the same model, or an error -- never silently duals
            out = self._adjoint_ll_and_grad(wrt, prepared=self._matern_prepared(fused))
            if out is not None:
                return out
            raise NotImplementedError("method = 'adjoint' is not available for this model / library")
        ser = self._device_series() if ts.dtype == np.float64 else None
        if ser is not None:
            model, d, npar = _backend.pack_grad_model(self._grad_blocks())
            ll, g = ser.gp_ll_grad(model, d, npar)
        else:
            ll, g = _backend.gp_ll_grad(self._grad_blocks(), ts.reshape(-1), Y.reshape(-1))
        return ll, mask_wrt(g, wrt)

    def log_posterior_density(self):
        return self.maximum_log_likelihood_objective()

    def training_loss(self):
        return -self.maximum_log_likelihood_objective()
