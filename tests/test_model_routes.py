"""Route census of StateSpaceGP: which C entry points each model call makes, in order.

Every ctypes call of pssgp._backend hands its symbol name to `_backend.check(ctx, code, what)`; the census wraps `check`, runs
each scenario below on fresh models and compares the recorded symbols with the literal table ROUTES.  A call that raises
records its exception type instead of a list.  Series are irregular and sorted, N = 96 and K = 24, unless a scenario says
otherwise.  The table was recorded from the model layer as it stood before its split into modules; a change of a route has
to change the table here, in the open.  (The route spies of test_gpu_het_noise, test_gpu_multi_output, test_gpu_multi_grad,
test_gpu_lti and test_gpu_adjoint check what they check; this file pins the whole map.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, K = 96, 24
R = 0.1
THETAS = np.array([[1.3, 0.7, 0.1], [0.9, 1.1, 0.2]])


def _kernel(name):
    from pssgp.kernels import Matern12, Matern32, Matern52, Periodic, RBF, SquaredExponential
    if name == "RBF":
        return RBF(variance=1.2, lengthscales=0.8, order=4, balancing_iter=5)
    if name == "Periodic":                                  # the general-LTI path without RBF's scaling shortcut
        return Periodic(SquaredExponential(1.1, 0.9), period=1.5, order=2)
    if name == "Matern32+Matern52":                          # d = 5: the composite dual-number gradient
        return Matern32(1.0, 0.8) + Matern52(0.6, 1.7)
    if name == "Periodic*Matern32+Matern52":                 # d = 4 * 2 + 3 = 11
        return Periodic(SquaredExponential(1.0, 1.0), period=2.0, order=1) * Matern32(1.0, 3.0) + Matern52(0.5, 1.2)
    return {"Matern12": Matern12, "Matern32": Matern32, "Matern52": Matern52}[name](variance=1.3, lengthscales=0.7)


def _data(n=N, m=1, seed=0):
    rng = np.random.RandomState(seed)
    t = np.cumsum(rng.uniform(0.02, 0.08, n))
    Y = np.sin(2.0 * t)[:, None] * rng.uniform(0.5, 2.0, (1, m)) + 0.2 * rng.randn(n, m)
    tq = np.sort(rng.uniform(t[0], t[-1], K))
    return t, Y, tq


def _model(kernel, t, Y, **kwargs):
    from pssgp.model import StateSpaceGP
    return StateSpaceGP((t, Y), _kernel(kernel), noise_variance=R, parallel=True, **kwargs)


def _twice(rec, label, make, call):
    """`call` on one fresh model: its first evaluation (host arrays) and its second (the series resident where it can be)."""
    m = make()
    rec(label + " #1", lambda: call(m))
    rec(label + " #2", lambda: call(m))


def _fused_path(rec, kernel):
    t, Y, tq = _data()
    m = _model(kernel, t, Y)
    rec("objective #1", m.maximum_log_likelihood_objective)
    rec("predict_f #2", lambda: m.predict_f(tq[:, None]))
    rec("objective #3 (memo)", m.maximum_log_likelihood_objective)
    m = _model(kernel, t, Y)
    rec("predict_f #1", lambda: m.predict_f(tq[:, None]))
    rec("objective #2", m.maximum_log_likelihood_objective)


def _gradients(rec, kernel, n=N, methods=(None, "adjoint", "dual", "differences")):
    t, Y, _ = _data(n)
    for method in methods:
        _twice(rec, f"grad {method}", lambda: _model(kernel, t, Y), lambda m: m.log_likelihood_and_grad(method=method))


def _other_kernel(rec, kernel, d):
    t, Y, tq = _data()
    assert _kernel(kernel).get_sde().F.shape[0] == d
    make = lambda: _model(kernel, t, Y)                                                     # noqa: E731
    _twice(rec, "objective", make, lambda m: m.maximum_log_likelihood_objective())
    _twice(rec, "predict_f", make, lambda m: m.predict_f(tq[:, None]))
    _twice(rec, "grad None", make, lambda m: m.log_likelihood_and_grad())
    _twice(rec, "grad dual", make, lambda m: m.log_likelihood_and_grad(method="dual"))


def _refused(rec, what):
    from pssgp import config
    t, Y, tq = _data()
    if what == "float32":
        config.set_default_float(np.float32)
    elif what == "unsorted ts":
        t = t[::-1].copy()
    elif what == "unsorted Xnew":
        tq = tq[::-1].copy()
    try:
        make = lambda: _model("Matern32", t, Y)                                             # noqa: E731
        _twice(rec, "objective", make, lambda m: m.maximum_log_likelihood_objective())
        _twice(rec, "predict_f", make, lambda m: m.predict_f(tq[:, None]))
        _twice(rec, "grad None", make, lambda m: m.log_likelihood_and_grad())
    finally:
        config.set_default_float(np.float64)


def _joint(rec):
    t, Y, tq = _data()
    make = lambda: _model("Matern32", t, Y)                                                 # noqa: E731
    _twice(rec, "predict_f full_cov", make, lambda m: m.predict_f(tq[:, None], full_cov=True))
    _twice(rec, "predict_f_samples", make, lambda m: m.predict_f_samples(tq[:, None], num_samples=2, seed=1))


def _batches(rec, kernel, B):
    t, Y, tq = _data()
    make = lambda: _model(kernel, t, Y)                                                     # noqa: E731
    _twice(rec, "log_likelihood_batch", make, lambda m: m.log_likelihood_batch(THETAS[:B]))
    _twice(rec, "predict_f_batch", make, lambda m: m.predict_f_batch(tq[:, None], THETAS[:B]))
    _twice(rec, "log_likelihood_and_grad_batch", make, lambda m: m.log_likelihood_and_grad_batch(THETAS[:B]))


def _multi(rec, kernel, M, rows, methods):
    """rows "complete": a few rows NaN in all columns; "mixed": one row NaN in one column only."""
    t, Y, tq = _data(m=M)
    if rows == "complete":
        Y[[5, 40, 41]] = np.nan
    else:
        Y[17, 1] = np.nan
    make = lambda: _model(kernel, t, Y)                                                     # noqa: E731
    _twice(rec, "objective", make, lambda m: m.maximum_log_likelihood_objective())
    _twice(rec, "predict_f", make, lambda m: m.predict_f(tq[:, None]))
    for method in methods:
        _twice(rec, f"grad {method}", make, lambda m: m.log_likelihood_and_grad(method=method))


def _het(rec, kernel):
    t, Y, tq = _data()
    s = np.random.RandomState(7).uniform(0.0, 0.3, N)
    make = lambda: _model(kernel, t, Y, observation_variances=s)                            # noqa: E731
    _twice(rec, "objective", make, lambda m: m.maximum_log_likelihood_objective())
    _twice(rec, "predict_f", make, lambda m: m.predict_f(tq[:, None]))
    _twice(rec, "grad None", make, lambda m: m.log_likelihood_and_grad())


SCENARIOS = {
    "fused path, Matern12": (_fused_path, "Matern12"),
    "fused path, Matern32": (_fused_path, "Matern32"),
    "fused path, Matern52": (_fused_path, "Matern52"),
    "gradients, Matern12": (_gradients, "Matern12"),
    "gradients, Matern32": (_gradients, "Matern32"),
    "gradients, Matern52": (_gradients, "Matern52"),
    "gradients, Matern32, N = 2048": (_gradients, "Matern32", 2048, (None,)),
    "gradients, Matern32, N = 2049": (_gradients, "Matern32", 2049, (None,)),
    "other kernels, RBF": (_other_kernel, "RBF", 4),
    "other kernels, Periodic": (_other_kernel, "Periodic", 6),
    "other kernels, Matern32+Matern52": (_other_kernel, "Matern32+Matern52", 5),
    "other kernels, Periodic*Matern32+Matern52": (_other_kernel, "Periodic*Matern32+Matern52", 11),
    "refused, float32 data": (_refused, "float32"),
    "refused, unsorted ts": (_refused, "unsorted ts"),
    "refused, unsorted Xnew": (_refused, "unsorted Xnew"),
    "joint covariance and draws": (_joint,),
    "batches, Matern32, B = 1": (_batches, "Matern32", 1),
    "batches, Matern32, B = 2": (_batches, "Matern32", 2),
    "batches, RBF, B = 2": (_batches, "RBF", 2),
    "multi-output, complete rows, M = 3, Matern32": (_multi, "Matern32", 3, "complete", (None, "adjoint", "dual")),
    "multi-output, complete rows, M = 2, Matern32": (_multi, "Matern32", 2, "complete", (None, "adjoint", "dual")),
    "multi-output, complete rows, M = 2, Matern52": (_multi, "Matern52", 2, "complete", (None, "adjoint", "dual")),
    "multi-output, mixed rows, M = 3, Matern32": (_multi, "Matern32", 3, "mixed", (None, "adjoint")),
    "per-observation noise, Matern32": (_het, "Matern32"),
    "per-observation noise, RBF": (_het, "RBF"),
}


def census(name, patch):
    """{step: [symbols] or exception type name} of one scenario; `patch(module, attribute, value)` replaces `check`."""
    from pssgp import _backend
    _backend.get_context()                      # (made outside the recording)
    real, calls, out = _backend.check, [], {}

    def spy(ctx, code, what):
        calls.append(what)
        return real(ctx, code, what)

    def rec(label, fn):
        del calls[:]
        try:
            fn()
            out[label] = list(calls)
        except Exception as e:                  # noqa: BLE001 -- the census records which one
            out[label] = type(e).__name__

    patch(_backend, "check", spy)
    fn, *args = SCENARIOS[name]
    fn(rec, *args)
    return out


ROUTES = {"fused path, Matern12": {"objective #1": ["pgps_gp_f64"],
                          "predict_f #2": ["pgps_series_create_f64",
                                           "pgps_series_set_queries_f64",
                                           "pgps_series_gp_predict_f64"],
                          "objective #3 (memo)": [],
                          "predict_f #1": ["pgps_gp_predict_f64"],
                          "objective #2": ["pgps_series_create_f64", "pgps_series_gp_ll_f64"]},
 "fused path, Matern32": {"objective #1": ["pgps_gp_f64"],
                          "predict_f #2": ["pgps_series_create_f64",
                                           "pgps_series_set_queries_f64",
                                           "pgps_series_gp_predict_f64"],
                          "objective #3 (memo)": [],
                          "predict_f #1": ["pgps_gp_predict_f64"],
                          "objective #2": ["pgps_series_create_f64", "pgps_series_gp_ll_f64"]},
 "fused path, Matern52": {"objective #1": ["pgps_gp_f64"],
                          "predict_f #2": ["pgps_series_create_f64",
                                           "pgps_series_set_queries_f64",
                                           "pgps_series_gp_predict_f64"],
                          "objective #3 (memo)": [],
                          "predict_f #1": ["pgps_gp_predict_f64"],
                          "objective #2": ["pgps_series_create_f64", "pgps_series_gp_ll_f64"]},
 "gradients, Matern12": {"grad None #1": ["pgps_gp_ll_grad_f64"],
                         "grad None #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_f64"],
                         "grad adjoint #1": "ValueError",  # known oddity: d = 1 is below the general adjoint pass
                         "grad adjoint #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_adj_f64"],
                         "grad dual #1": ["pgps_gp_ll_grad_f64"],
                         "grad dual #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_f64"],
                         "grad differences #1": ["pgps_gp_ll_batch_f64"],
                         "grad differences #2": ["pgps_gp_ll_batch_f64"]},
 "gradients, Matern32": {"grad None #1": ["pgps_gp_ll_grad_f64"],
                         "grad None #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_f64"],
                         "grad adjoint #1": ["pgps_lti_ll_grad_f64"],
                         "grad adjoint #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_adj_f64"],
                         "grad dual #1": ["pgps_gp_ll_grad_f64"],
                         "grad dual #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_f64"],
                         "grad differences #1": ["pgps_gp_ll_batch_f64"],
                         "grad differences #2": ["pgps_gp_ll_batch_f64"]},
 "gradients, Matern52": {"grad None #1": ["pgps_gp_ll_grad_f64"],
                         "grad None #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_adj_f64"],
                         "grad adjoint #1": ["pgps_lti_ll_grad_f64"],
                         "grad adjoint #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_adj_f64"],
                         "grad dual #1": ["pgps_gp_ll_grad_f64"],
                         "grad dual #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_f64"],
                         "grad differences #1": ["pgps_gp_ll_batch_f64"],
                         "grad differences #2": ["pgps_gp_ll_batch_f64"]},
 "gradients, Matern32, N = 2048": {"grad None #1": ["pgps_gp_ll_grad_f64"],
                                   "grad None #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_f64"]},
 "gradients, Matern32, N = 2049": {"grad None #1": ["pgps_gp_ll_grad_f64"],
                                   "grad None #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_adj_f64"]},
 "other kernels, RBF": {"objective #1": ["pgps_lti_ll_f64"],
                        "objective #2": ["pgps_series_create_f64", "pgps_series_lti_ll_f64"],
                        "predict_f #1": ["pgps_lti_predict_f64"],
                        "predict_f #2": ["pgps_series_create_f64",
                                         "pgps_series_set_queries_f64",
                                         "pgps_series_lti_predict_f64"],
                        "grad None #1": ["pgps_lti_ll_grad_f64"],
                        "grad None #2": ["pgps_series_create_f64", "pgps_series_lti_ll_grad_f64"],
                        "grad dual #1": "NotImplementedError",
                        "grad dual #2": "NotImplementedError"},
 "other kernels, Periodic": {"objective #1": ["pgps_lti_ll_f64"],
                             "objective #2": ["pgps_series_create_f64", "pgps_series_lti_ll_f64"],
                             "predict_f #1": ["pgps_lti_predict_f64"],
                             "predict_f #2": ["pgps_series_create_f64",
                                              "pgps_series_set_queries_f64",
                                              "pgps_series_lti_predict_f64"],
                             "grad None #1": ["pgps_lti_ll_grad_f64"],
                             "grad None #2": ["pgps_series_create_f64", "pgps_series_lti_ll_grad_f64"],
                             "grad dual #1": "NotImplementedError",
                             "grad dual #2": "NotImplementedError"},
 "other kernels, Matern32+Matern52": {"objective #1": ["pgps_lti_ll_f64"],
                                      "objective #2": ["pgps_series_create_f64", "pgps_series_lti_ll_f64"],
                                      "predict_f #1": ["pgps_lti_predict_f64"],
                                      "predict_f #2": ["pgps_series_create_f64",
                                                       "pgps_series_set_queries_f64",
                                                       "pgps_series_lti_predict_f64"],
                                      "grad None #1": ["pgps_lti_ll_grad_f64"],
                                      "grad None #2": ["pgps_series_create_f64", "pgps_series_lti_ll_grad_f64"],
                                      "grad dual #1": ["pgps_gp_ll_grad_blocks_f64"],
                                      "grad dual #2": ["pgps_gp_ll_grad_blocks_f64"]},
 "other kernels, Periodic*Matern32+Matern52": {"objective #1": ["pgps_lti_ll_f64"],
                                               "objective #2": ["pgps_series_create_f64", "pgps_series_lti_ll_f64"],
                                               "predict_f #1": ["pgps_lti_predict_f64"],
                                               "predict_f #2": ["pgps_series_create_f64",
                                                                "pgps_series_set_queries_f64",
                                                                "pgps_series_lti_predict_f64"],
                                               "grad None #1": ["pgps_lti_ll_grad_f64"],
                                               "grad None #2": ["pgps_series_create_f64", "pgps_series_lti_ll_grad_f64"],
                                               "grad dual #1": "NotImplementedError",
                                               "grad dual #2": "NotImplementedError"},
 "refused, float32 data": {"objective #1": ["pgps_gp_f32"],
                           "objective #2": ["pgps_gp_f32"],
                           "predict_f #1": ["pgps_gp_predict_f32"],
                           "predict_f #2": ["pgps_gp_predict_f32"],
                           "grad None #1": ["pgps_gp_ll_grad_f64"],
                           "grad None #2": ["pgps_gp_ll_grad_f64"]},
 "refused, unsorted ts": {"objective #1": "PgpsError",
                          "objective #2": "PgpsError",
                          "predict_f #1": "PgpsError",
                          "predict_f #2": "PgpsError",
                          "grad None #1": "PgpsError",
                          "grad None #2": "PgpsError"},
 "refused, unsorted Xnew": {"objective #1": ["pgps_gp_f64"],
                            "objective #2": ["pgps_series_create_f64", "pgps_series_gp_ll_f64"],
                            "predict_f #1": "ValueError",
                            "predict_f #2": "ValueError",
                            "grad None #1": ["pgps_gp_ll_grad_f64"],
                            "grad None #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_f64"]},
 "joint covariance and draws": {"predict_f full_cov #1": ["pgps_lti_predict_cov_f64"],
                                "predict_f full_cov #2": ["pgps_lti_predict_cov_f64"],
                                "predict_f_samples #1": ["pgps_lti_sample_f64"],
                                "predict_f_samples #2": ["pgps_lti_sample_f64"]},
 "batches, Matern32, B = 1": {"log_likelihood_batch #1": ["pgps_gp_ll_batch_f64"],
                              "log_likelihood_batch #2": ["pgps_gp_ll_batch_f64"],
                              "predict_f_batch #1": ["pgps_gp_predict_f64"],
                              "predict_f_batch #2": ["pgps_series_create_f64",
                                                     "pgps_series_set_queries_f64",
                                                     "pgps_series_gp_predict_f64"],
                              "log_likelihood_and_grad_batch #1": ["pgps_gp_ll_grad_f64"],
                              "log_likelihood_and_grad_batch #2": ["pgps_series_create_f64", "pgps_series_gp_ll_grad_f64"]},
 "batches, Matern32, B = 2": {"log_likelihood_batch #1": ["pgps_gp_ll_batch_f64"],
                              "log_likelihood_batch #2": ["pgps_gp_ll_batch_f64"],
                              "predict_f_batch #1": ["pgps_gp_predict_batch_f64"],
                              "predict_f_batch #2": ["pgps_series_create_f64",
                                                     "pgps_series_set_queries_f64",
                                                     "pgps_series_gp_predict_batch_f64"],
                              "log_likelihood_and_grad_batch #1": ["pgps_gp_ll_grad_adj_batch_f64"],
                              "log_likelihood_and_grad_batch #2": ["pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_adj_batch_f64"]},
 "batches, RBF, B = 2": {"log_likelihood_batch #1": ["pgps_lti_ll_batch_f64"],
                         "log_likelihood_batch #2": ["pgps_series_create_f64", "pgps_series_lti_ll_batch_f64"],
                         "predict_f_batch #1": ["pgps_lti_predict_batch_f64"],
                         "predict_f_batch #2": ["pgps_series_create_f64",
                                                "pgps_series_set_queries_f64",
                                                "pgps_series_lti_predict_batch_f64"],
                         "log_likelihood_and_grad_batch #1": ["pgps_lti_ll_grad_batch_f64"],
                         "log_likelihood_and_grad_batch #2": ["pgps_series_create_f64",
                                                              "pgps_series_lti_ll_grad_batch_f64"]},
 "multi-output, complete rows, M = 3, Matern32": {"objective #1": ["pgps_gp_ll_multi_f64"],
                                                  "objective #2": ["pgps_gp_ll_multi_f64"],
                                                  "predict_f #1": ["pgps_gp_predict_multi_f64"],
                                                  "predict_f #2": ["pgps_gp_predict_multi_f64"],
                                                  "grad None #1": ["pgps_gp_ll_grad_multi_f64"],
                                                  "grad None #2": ["pgps_gp_ll_grad_multi_f64"],
                                                  "grad adjoint #1": ["pgps_gp_ll_grad_multi_f64"],
                                                  "grad adjoint #2": ["pgps_gp_ll_grad_multi_f64"],
                                                  "grad dual #1": ["pgps_gp_ll_grad_f64",
                                                                   "pgps_gp_ll_grad_f64",
                                                                   "pgps_gp_ll_grad_f64"],
                                                  "grad dual #2": ["pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_f64",
                                                                   "pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_f64",
                                                                   "pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_f64"]},
 "multi-output, complete rows, M = 2, Matern32": {"objective #1": ["pgps_gp_ll_multi_f64"],
                                                  "objective #2": ["pgps_gp_ll_multi_f64"],
                                                  "predict_f #1": ["pgps_gp_predict_multi_f64"],
                                                  "predict_f #2": ["pgps_gp_predict_multi_f64"],
                                                  "grad None #1": ["pgps_gp_ll_grad_f64", "pgps_gp_ll_grad_f64"],
                                                  "grad None #2": ["pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_f64",
                                                                   "pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_f64"],
                                                  "grad adjoint #1": ["pgps_gp_ll_grad_multi_f64"],
                                                  "grad adjoint #2": ["pgps_gp_ll_grad_multi_f64"],
                                                  "grad dual #1": ["pgps_gp_ll_grad_f64", "pgps_gp_ll_grad_f64"],
                                                  "grad dual #2": ["pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_f64",
                                                                   "pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_f64"]},
 "multi-output, complete rows, M = 2, Matern52": {"objective #1": ["pgps_gp_ll_multi_f64"],
                                                  "objective #2": ["pgps_gp_ll_multi_f64"],
                                                  "predict_f #1": ["pgps_gp_predict_multi_f64"],
                                                  "predict_f #2": ["pgps_gp_predict_multi_f64"],
                                                  "grad None #1": ["pgps_gp_ll_grad_multi_f64"],
                                                  "grad None #2": ["pgps_gp_ll_grad_multi_f64"],
                                                  "grad adjoint #1": ["pgps_gp_ll_grad_multi_f64"],
                                                  "grad adjoint #2": ["pgps_gp_ll_grad_multi_f64"],
                                                  "grad dual #1": ["pgps_gp_ll_grad_f64", "pgps_gp_ll_grad_f64"],
                                                  "grad dual #2": ["pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_f64",
                                                                   "pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_f64"]},
 "multi-output, mixed rows, M = 3, Matern32": {"objective #1": ["pgps_gp_f64", "pgps_gp_f64", "pgps_gp_f64"],
                                               "objective #2": ["pgps_series_create_f64",
                                                                "pgps_series_gp_ll_f64",
                                                                "pgps_series_create_f64",
                                                                "pgps_series_gp_ll_f64",
                                                                "pgps_series_create_f64",
                                                                "pgps_series_gp_ll_f64"],
                                               "predict_f #1": ["pgps_gp_predict_f64",
                                                                "pgps_gp_predict_f64",
                                                                "pgps_gp_predict_f64"],
                                               "predict_f #2": ["pgps_series_create_f64",
                                                                "pgps_series_set_queries_f64",
                                                                "pgps_series_gp_predict_f64",
                                                                "pgps_series_create_f64",
                                                                "pgps_series_set_queries_f64",
                                                                "pgps_series_gp_predict_f64",
                                                                "pgps_series_create_f64",
                                                                "pgps_series_set_queries_f64",
                                                                "pgps_series_gp_predict_f64"],
                                               "grad None #1": ["pgps_gp_ll_grad_f64",
                                                                "pgps_gp_ll_grad_f64",
                                                                "pgps_gp_ll_grad_f64"],
                                               "grad None #2": ["pgps_series_create_f64",
                                                                "pgps_series_gp_ll_grad_f64",
                                                                "pgps_series_create_f64",
                                                                "pgps_series_gp_ll_grad_f64",
                                                                "pgps_series_create_f64",
                                                                "pgps_series_gp_ll_grad_f64"],
                                               "grad adjoint #1": ["pgps_lti_ll_grad_f64",
                                                                   "pgps_lti_ll_grad_f64",
                                                                   "pgps_lti_ll_grad_f64"],
                                               "grad adjoint #2": ["pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_adj_f64",
                                                                   "pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_adj_f64",
                                                                   "pgps_series_create_f64",
                                                                   "pgps_series_gp_ll_grad_adj_f64"]},
 "per-observation noise, Matern32": {"objective #1": ["pgps_gp_ll_het_f64"],
                                     "objective #2": ["pgps_gp_ll_het_f64"],
                                     "predict_f #1": ["pgps_gp_predict_het_f64"],
                                     "predict_f #2": ["pgps_gp_predict_het_f64"],
                                     "grad None #1": ["pgps_gp_ll_grad_adj_het_f64"],
                                     "grad None #2": ["pgps_gp_ll_grad_adj_het_f64"]},
 "per-observation noise, RBF": {"objective #1": ["pgps_discretise_f64", "pgps_seq_kf_het"],  # known oddity: get_ssm discretises on the device
                                "objective #2": ["pgps_discretise_f64", "pgps_seq_kf_het"],
                                "predict_f #1": ["pgps_discretise_f64", "pgps_seq_kf_het", "pgps_seq_ks"],
                                "predict_f #2": ["pgps_discretise_f64", "pgps_seq_kf_het", "pgps_seq_ks"],
                                "grad None #1": "NotImplementedError",
                                "grad None #2": "NotImplementedError"}}


def test_table_covers_every_scenario():
    assert sorted(ROUTES) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_routes(name, monkeypatch):
    got = census(name, monkeypatch.setattr)
    want = ROUTES[name]
    moved = {step: (got.get(step), want.get(step)) for step in list(got) + list(want) if got.get(step) != want.get(step)}
    assert not moved, f"{name}: (recorded, table) {moved}"
