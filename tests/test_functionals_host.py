"""Linear functionals of the state without a GPU: the kernels' component / derivative rows, and the host twin of
StateSpaceGP.predict_components / predict_f_derivative / predict_functionals (parallel=False) against the dense GP."""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import functional_refs as R


def _sum_kernels():
    from pssgp.kernels import Matern32, Matern52, Periodic, SquaredExponential
    return {
        "m32+m52": Matern32(1.3, 0.4) + Matern52(0.7, 0.9),
        "nested": (Matern32(1.0, 0.5) + Matern52(1.0, 0.5)) + (Matern52(0.5, 2.0) + Matern32(0.6, 1.1)),
        "qp+m32": Periodic(SquaredExponential(1., 1.), period=1., order=3) * Matern32(0.5, 5.) + Matern32(1., 2.),
    }


@pytest.mark.parametrize("name", ["m32+m52", "nested", "qp+m32"])
def test_component_rows_sum_to_H_with_disjoint_supports(name):
    k = _sum_kernels()[name]
    names, C = k.component_functionals()
    sde = k.get_sde()
    H = np.asarray(sde.H, np.float64).reshape(-1)
    assert C.shape == (len(k.kernels), H.shape[0]) and len(names) == C.shape[0]
    assert np.array_equal(C.sum(axis=0), H)                         # exactly: every column belongs to one row
    assert np.all(np.sum(C != 0.0, axis=0) <= 1)                    # disjoint supports
    dims = [np.asarray(p.get_sde().F).shape[0] for p in k.kernels]
    start = 0
    for j, dj in enumerate(dims):                                   # row j lives in block j's columns
        assert not np.any(C[j, :start]) and not np.any(C[j, start + dj:])
        start += dj
    assert len(set(names)) == len(names)


def test_component_names_and_single_kernels():
    from pssgp.kernels import Matern32, Matern52
    from pssgp.kernels.base import SDESum
    k = SDESum([Matern32(1., 1.), Matern52(1., 1.)])
    k.kernels[0].name = "fast"
    assert k.component_functionals()[0] == ["fast", "Matern521"]
    for single in (Matern32(1.2, 0.7), Matern32(1., 1.) * Matern52(1., 1.)):
        names, C = single.component_functionals()
        assert len(names) == 1 and np.array_equal(C, np.asarray(single.get_sde().H, np.float64).reshape(1, -1))


def test_derivative_order_zero_is_H():
    for k in _sum_kernels().values():
        assert np.array_equal(k.derivative_functional(0), np.asarray(k.get_sde().H, np.float64).reshape(-1))


def test_derivative_beyond_the_kernels_smoothness_raises():
    from pssgp.kernels import Matern12, Matern32, Matern52, RBF, Periodic, SquaredExponential
    for kernel, order in ((Matern12(1., 1.), 1), (Matern32(1., 1.), 2), (Matern52(1., 1.), 3),
                          (Matern52(1., 1.) + Matern32(1., 1.), 2), (RBF(1., 1., order=6, balancing_iter=5) + Matern32(1., 1.), 2),
                          (Matern32(1., 1.) * Matern52(1., 1.), 2)):
        with pytest.raises(ValueError, match="mean-square differentiable"):
            kernel.derivative_functional(order)
    # ... and what is smooth enough passes: Matern by its order, RBF (order 6: five derivatives), Periodic (any), products
    Matern32(1., 1.).derivative_functional(1)
    Matern52(1., 1.).derivative_functional(2)
    RBF(1., 1., order=6, balancing_iter=5).derivative_functional(3)
    Periodic(SquaredExponential(1., 1.), period=1., order=3).derivative_functional(4)
    (Matern32(1., 1.) * Matern52(1., 1.)).derivative_functional(1)
    (Periodic(SquaredExponential(1., 1.), period=1., order=2) * Matern32(1., 1.) + Matern52(1., 1.)).derivative_functional(1)


def test_derivative_prior_variance_is_minus_k_second_at_zero():
    """c Pinf c^T = Var f'(t) = -k''(0) and c Pinf H^T = Cov(f', f) = 0 for a stationary process."""
    from pssgp.kernels import Matern32, Matern52
    v3, l3, v5, l5 = 1.3, 0.4, 0.7, 0.9
    cases = [(Matern32(v3, l3), 3 * v3 / l3 ** 2), (Matern52(v5, l5), 5 * v5 / (3 * l5 ** 2)),
             (Matern52(v5, l5, balancing_iter=10), 5 * v5 / (3 * l5 ** 2)),
             (Matern32(v3, l3) + Matern52(v5, l5), 3 * v3 / l3 ** 2 + 5 * v5 / (3 * l5 ** 2))]
    for k, want in cases:
        sde = k.get_sde()
        P = np.asarray(sde.P0, np.float64)
        H = np.asarray(sde.H, np.float64).reshape(-1)
        c = k.derivative_functional(1)
        assert abs(c @ P @ c - want) < 1e-10 * want
        assert abs(c @ P @ H) < 1e-12


def _toy(n=60, k=40, seed=3):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, 4.0, n))
    y = np.sin(2.0 * t) + 0.4 * np.cos(5.0 * t) + 0.2 * rng.standard_normal(n)
    tq = np.sort(rng.uniform(-0.3, 4.3, k))
    return t, y, tq


def _model(kernel, t, y, noise=0.1, **kw):
    from pssgp.model import StateSpaceGP
    return StateSpaceGP((t[:, None], y[:, None]), kernel, noise_variance=noise, parallel=False, **kw)


def test_host_components_vs_dense_gp():
    from pssgp.kernels import Matern32, Matern52
    t, y, tq = _toy()
    m = _model(Matern32(1.3, 0.4) + Matern52(0.7, 0.9), t, y)
    specs = [("matern32", 1.3, 0.4), ("matern52", 0.7, 0.9)]
    mean_o, cov_o = R.dense_components(specs, t, y, 0.1, tq)
    mean, cov = m.predict_components(tq[:, None], cross_cov=True)
    assert mean.shape == (40, 2) and cov.shape == (40, 2, 2)
    R.assert_close(mean, mean_o, 1e-8, "component means")
    R.assert_close(cov, cov_o, 1e-8, "component covariances")
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    mean2, var = m.predict_components(tq[:, None])
    assert np.array_equal(mean2, mean) and np.array_equal(var, np.diagonal(cov, axis1=1, axis2=2))
    # the parts add up to predict_f
    pm, pv, _ = m._predict_f_host(tq)                               # (predict_f's host twin: no device for the discretisation)
    R.assert_close(mean.sum(axis=1), pm, 1e-9, "sum of the means")
    R.assert_close(cov.sum(axis=(1, 2)), pv, 1e-9, "1^T cov 1")
    assert m.component_names() == ["Matern320", "Matern521"]


def test_closed_form_derivative_kernels_vs_central_differences():
    """The closed forms the dense references below are built from, against central differences of kernel.K at lags well away
    from 0 (where |tau| has its kink)."""
    from pssgp.kernels import Matern32, Matern52
    tau = np.array([-1.7, -0.6, 0.35, 0.9, 2.2])
    # second-order central stencils: the error is h^2 k^(n+2) / 6 .. / 4 plus 2^n eps / h^n of rounding.  With lambda <= 4.4
    # (k^(n+2) ~ lambda^2 k^(n)): h = 1e-3 gives < 1e-5 relative for n <= 2, h = 1e-2 gives < 1e-3 for n = 3, 4.
    stencils = {1: ((-1, 1), (-0.5, 0.5)), 2: ((-1, 0, 1), (1.0, -2.0, 1.0)),
                3: ((-2, -1, 1, 2), (-0.5, 1.0, -1.0, 0.5)), 4: ((-2, -1, 0, 1, 2), (1.0, -4.0, 6.0, -4.0, 1.0))}
    for nu2, k, orders in ((3, Matern32(1.3, 0.4), (1, 2)), (5, Matern52(0.7, 0.9), (1, 2, 3, 4))):
        f = lambda x: k.K(x, np.zeros(1))[:, 0]                     # noqa: E731 -- k(tau) = K(tau, 0)
        for n in orders:
            h, tol = (1e-3, 1e-4) if n <= 2 else (1e-2, 2e-3)
            offs, w = stencils[n]
            fd = sum(wi * f(tau + o * h) for o, wi in zip(offs, w)) / h ** n
            got = R.matern_dk(nu2, k.variance, k.lengthscales, tau, n, 0)
            scale = float(np.max(np.abs(got)))
            print(f"Matern-{nu2}/2 k^({n}): max |closed - differences| / scale = {np.max(np.abs(got - fd)) / scale:.2e}")
            assert np.max(np.abs(got - fd)) < tol * scale, (nu2, n, got, fd)
            # d/dt = -d/dtau
            assert np.array_equal(R.matern_dk(nu2, k.variance, k.lengthscales, tau, 0, n), (-1.0) ** n * got)


@pytest.mark.parametrize("nu2,order", [(3, 1), (5, 1), (5, 2)])
def test_host_derivative_vs_dense_gp(nu2, order):
    from pssgp.kernels import Matern32, Matern52
    t, y, tq = _toy()
    v, ell = (1.3, 0.4) if nu2 == 3 else (0.7, 0.9)
    kernel = Matern32(v, ell) if nu2 == 3 else Matern52(v, ell)
    mean_o, var_o = R.dense_derivative(nu2, v, ell, t, y, 0.1, tq, order)
    mean, var = _model(kernel, t, y).predict_f_derivative(tq[:, None], order=order)
    assert mean.shape == (40, 1) and var.shape == (40, 1)
    R.assert_close(mean[:, 0], mean_o, 1e-8, f"mean of f^({order})")
    R.assert_close(var[:, 0], var_o, 1e-8, f"variance of f^({order})")


def test_host_components_of_an_approximate_kernel_vs_dense_gp():
    """Periodic * Matern32 + Matern52: the periodic factor's state-space form is a truncated series, hence the 1e-2 the project
    uses for approximate kernels."""
    from pssgp.kernels import Matern32, Matern52, Periodic, SquaredExponential
    t, y, tq = _toy()
    kernel = Periodic(SquaredExponential(1., 1.), period=1., order=6) * Matern32(1., 1.5) + Matern52(0.8, 0.7)
    specs = [("prod", [("periodic", 1., 1., 1.), ("matern32", 1., 1.5)]), ("matern52", 0.8, 0.7)]
    mean_o, cov_o = R.dense_components(specs, t, y, 0.1, tq)
    mean, cov = _model(kernel, t, y).predict_components(tq[:, None], cross_cov=True)
    np.testing.assert_allclose(mean, mean_o, atol=1e-2, rtol=1e-2)
    np.testing.assert_allclose(cov, cov_o, atol=1e-2, rtol=1e-2)


def test_predict_functionals_orders_repeats_and_empty():
    from pssgp.kernels import Matern32, Matern52
    t, y, tq = _toy()
    k = Matern32(1.3, 0.4) + Matern52(0.7, 0.9)
    m = _model(k, t, y)
    C = np.vstack([k.component_functionals()[1], k.derivative_functional(1)])
    mean, cov = m.predict_functionals(tq[:, None], C)
    perm = np.random.default_rng(0).permutation(np.concatenate([np.arange(40), [3, 3, 17]]))
    mean_p, cov_p = m.predict_functionals(tq[perm][:, None], C)
    assert np.array_equal(mean_p, mean[perm]) and np.array_equal(cov_p, cov[perm])
    # times given out of order are sorted for the host twin
    shuffle = np.random.default_rng(1).permutation(t.shape[0])
    mean_s, cov_s = _model(k, t[shuffle], y[shuffle]).predict_functionals(tq[:, None], C)
    R.assert_close(mean_s, mean, 1e-12, "shuffled training rows, mean")
    R.assert_close(cov_s, cov, 1e-12, "shuffled training rows, cov")
    # empty Xnew
    mean_e, cov_e = m.predict_functionals(np.zeros((0, 1)), C)
    assert mean_e.shape == (0, 3) and cov_e.shape == (0, 3, 3)
    mean_e, var_e = m.predict_components(np.zeros((0, 1)))
    assert mean_e.shape == (0, 2) and var_e.shape == (0, 2)
    assert m.predict_components(np.zeros((0, 1)), cross_cov=True)[1].shape == (0, 2, 2)
    mean_e, var_e = m.predict_f_derivative(np.zeros((0, 1)))
    assert mean_e.shape == (0, 1) and var_e.shape == (0, 1)
    with pytest.raises(ValueError):
        m.predict_functionals(tq[:, None], np.ones((2, 4)))


def test_d1_kernel_takes_the_host_twin_in_parallel_mode(monkeypatch):
    """Matern-1/2 (d = 1) is below the device call's dimensions: parallel=True must not reach it."""
    from pssgp import _backend
    from pssgp.kernels import Matern12
    from pssgp.model import StateSpaceGP
    monkeypatch.setattr(_backend, "lti_predict_lin", lambda *a, **k: pytest.fail("device call for d = 1"))
    t, y, tq = _toy()
    m = StateSpaceGP((t[:, None], y[:, None]), Matern12(1., 0.8), noise_variance=0.1, parallel=True)
    mean, var = m.predict_components(tq[:, None])
    _, mean_o, var_o = O.dense_gp(("matern12", 1., 0.8), t, y, 0.1, tq)
    R.assert_close(mean[:, 0], mean_o, 1e-8, "d = 1 mean")
    R.assert_close(var[:, 0], var_o, 1e-8, "d = 1 variance")


def test_models_the_functionals_do_not_cover():
    from pssgp.kernels import Matern32
    from pssgp.mean_functions import Constant
    from pssgp.model import StateSpaceGP
    t, y, tq = _toy()
    k = Matern32(1., 0.5)
    models = [StateSpaceGP((t[:, None], np.stack([y, y], axis=1)), k, noise_variance=0.1),
              StateSpaceGP((t[:, None], y[:, None]), k, noise_variance=0.1, observation_variances=np.full(t.shape, 0.01)),
              StateSpaceGP((t[:, None], y[:, None]), k, noise_variance=0.1, mean_function=Constant())]
    for m in models:
        for call in (lambda: m.predict_components(tq[:, None]), lambda: m.predict_f_derivative(tq[:, None]),
                     lambda: m.predict_functionals(tq[:, None], np.eye(2))):
            with pytest.raises(NotImplementedError):
                call()


def test_float32_default_float_gives_float32():
    from pssgp import config
    from pssgp.kernels import Matern32, Matern52
    t, y, tq = _toy()
    k = Matern32(1.3, 0.4) + Matern52(0.7, 0.9)
    mean64, cov64 = _model(k, t, y).predict_components(tq[:, None], cross_cov=True)
    old = config.default_float()
    config.set_default_float(np.float32)
    try:
        m = _model(k, t.astype(np.float32), y.astype(np.float32))
        mean, cov = m.predict_components(tq[:, None].astype(np.float32), cross_cov=True)
    finally:
        config.set_default_float(old)
    assert mean.dtype == np.float32 and cov.dtype == np.float32
    R.assert_close(mean, mean64, 1e-3, "float32 means")
    R.assert_close(cov, cov64, 1e-3, "float32 covariances")
