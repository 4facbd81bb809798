"""CPU tests of Laplace inference (pssgp/likelihoods.py, pssgp/laplace.py with parallel=False: the host twin of the device
loop) against the references of laplace_refs.py.  No GPU."""
import warnings

import numpy as np
import pytest
from scipy.linalg import expm

import laplace_refs as LR

DENSE_TOL = 1e-6                # kernel_zoo's tolerance against the dense GP (tests/conftest.py), every kernel that has one


def _likelihood(lik):
    from pssgp.likelihoods import Bernoulli, Gaussian, Poisson
    return {"gaussian": lambda: Gaussian(LR.PARS["gaussian"]), "bernoulli": Bernoulli, "poisson": lambda: Poisson(LR.PARS["poisson"])}[lik]()


def _central(fn, f, h=1e-5):
    return (fn(f + h) - fn(f - h)) / (2.0 * h)


@pytest.mark.parametrize("lik", ["gaussian", "bernoulli", "poisson"])
def test_likelihood_derivatives_against_central_differences(lik):
    L = _likelihood(lik)
    rng = np.random.RandomState(3)
    f = rng.uniform(-3.0, 3.0, 200)
    y = {"gaussian": rng.randn(200), "bernoulli": (rng.rand(200) < 0.5).astype(float), "poisson": rng.poisson(3.0, 200).astype(float)}[lik]
    lp, g, W, d3 = L.log_prob_derivs(y, f)
    # the difference quotient's error at h = 1e-5: h^2 / 6 of the third derivative above (<= 30 here) + rounding 1e-16 / h of the
    # values (<= 100): below 1e-8 of the scale max(1, |value|)
    for name, got, fn in (("g", g, lambda x: L.log_prob_derivs(y, x)[0]), ("W", -W, lambda x: L.log_prob_derivs(y, x)[1]),
                          ("d3", d3, lambda x: -L.log_prob_derivs(y, x)[2])):
        want = _central(fn, f)
        e = np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))
        print(f"{lik} {name}: {e:.2e}")
        assert e <= 1e-8, (lik, name, e)
    # ... and the references' textbook formulas
    for got, want in zip((lp, g, W, d3), LR.lik_derivs(lik, LR.PARS[lik], y, f)):
        assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) <= 1e-12
    # the stable forms stay finite where the textbook ones do not, and the floor of W holds
    far = np.array([-800.0, -40.0, 40.0, 800.0])
    if lik == "bernoulli":
        for yy in (0.0, 1.0):
            out = L.log_prob_derivs(np.full(4, yy), far)
            assert all(np.all(np.isfinite(a)) for a in out) and np.all(out[2] >= LR.W_MIN)
            assert np.allclose(out[0], -np.maximum(-(2 * yy - 1) * far, 0.0), atol=1e-15)
    assert np.all(L.log_prob_derivs(y[:4], np.full(4, -60.0))[2] >= LR.W_MIN)


def _dense_case(lik, n=60, seed=1):
    rng = np.random.RandomState(seed)
    t = np.sort(rng.uniform(0.0, 10.0, n))
    K = LR.matern_K("m32", 2.0, 1.3, t, t) + 1e-12 * np.eye(n)
    latent = np.linalg.cholesky(K) @ rng.randn(n)
    y = (rng.rand(n) < 1.0 / (1.0 + np.exp(-latent))).astype(float) if lik == "bernoulli" else rng.poisson(np.exp(latent)).astype(float)
    return t, y


@pytest.mark.parametrize("lik", ["bernoulli", "poisson"])
def test_dense_reference_gradient_and_polarisation_identity(lik):
    """The reference's analytic gradient (R&W section 5.5.1) against central differences of its own evidence, and against the
    differences of G(z + w) - G(w) + G(0) at fixed sites: 1e-5 relative, the difference quotient's error at h = 1e-5."""
    t, y = _dense_case(lik)
    par, theta = LR.PARS[lik], np.array([2.0, 1.3])
    fit = LR.dense_fit("m32", theta[0], theta[1], t, y, lik, par, tol=1e-13, grad=True)
    z, s = fit["z"], fit["s"]
    w = 0.5 * fit["v"] * fit["d3"] / fit["W"]

    def G(x, th):
        C = LR.matern_K("m32", th[0], th[1], t, t) + np.diag(s)
        L = np.linalg.cholesky(C)
        return -0.5 * x @ np.linalg.solve(C, x) - np.sum(np.log(np.diag(L))) - 0.5 * x.size * LR.LOG2PI

    h = 1e-5
    for j in range(2):
        e = np.zeros(2)
        e[j] = h
        fd = (LR.dense_fit("m32", *(theta + e), t, y, lik, par, tol=1e-13)["evidence"]
              - LR.dense_fit("m32", *(theta - e), t, y, lik, par, tol=1e-13)["evidence"]) / (2.0 * h)
        T = lambda th: G(z + w, th) - G(w, th) + G(np.zeros_like(z), th)
        pol = (T(theta + e) - T(theta - e)) / (2.0 * h)
        scale = np.max(np.abs(fit["gradient"]))
        print(f"{lik} d/dtheta{j}: analytic {fit['gradient'][j]:.10f} differences {fd:.10f} polarisation {pol:.10f}")
        assert abs(fit["gradient"][j] - fd) <= 1e-5 * scale
        assert abs(fit["gradient"][j] - pol) <= 1e-5 * scale
    # the evidence as the Gaussian log-likelihood of the sites plus the per-step correction equals eq. 3.32
    _, _, _, corr = LR.sites_at(lik, par, y, fit["f"])
    assert abs(G(z, theta) + corr + LR.lik_constant(lik, y) - fit["evidence"]) <= 1e-12 * abs(fit["evidence"])


def _sde_covariance(sde, t):
    """The covariance function of the state-space model itself, H expm(F |dt|) P0 H^T: the dense twin of a kernel whose SDE is an
    approximation of it (RBF)."""
    F, P0, H = (np.asarray(a, np.float64) for a in (sde.F, sde.P0, sde.H))
    h = H.reshape(-1)
    K = np.empty((t.size, t.size))
    for i in range(t.size):
        for j in range(i + 1):
            K[i, j] = K[j, i] = h @ expm(F * (t[i] - t[j])) @ P0 @ h
    return K


@pytest.mark.parametrize("lik", ["bernoulli", "poisson"])
@pytest.mark.parametrize("kname", ["m32", "rbf"])
def test_host_twin_against_the_dense_reference(kname, lik):
    from pssgp.kernels import RBF
    from pssgp.laplace import LaplaceStateSpaceGP
    n = 120
    t, y = (np.array(a) for a in LR.case(lik, n))
    y[np.linspace(5, n - 5, 9).astype(int)] = np.nan
    assert np.isnan(y).sum() >= 9
    kernel = LR.matern("m32") if kname == "m32" else RBF(variance=1., lengthscales=0.5, order=6, balancing_iter=10)
    o = ~np.isnan(y)
    # Matern-3/2: the kernel's own dense covariance; RBF: the covariance of its order-6 SDE (the model the twin runs), which is
    # what the state-space recursion is exact for
    K = LR.matern_K("m32", 1.0, 0.5, t, t) if kname == "m32" else _sde_covariance(kernel.get_sde(), t)
    ref = LR.dense_laplace(K[np.ix_(o, o)], y[o], lik, LR.PARS[lik])
    assert not ref["diverged"]
    C = K[np.ix_(o, o)] + np.diag(ref["s"])
    f_all = K[:, o] @ ref["alpha"]
    v_all = np.diag(K) - np.sum(K[o, :] * np.linalg.solve(C, K[o, :]), axis=0)
    m = LaplaceStateSpaceGP((t[:, None], y[:, None]), kernel, _likelihood(lik), parallel=False)
    f, v = m.posterior_mode()
    ev = float(m.maximum_log_likelihood_objective())
    e = (LR.rel(f[:, 0], f_all), LR.rel(v[:, 0], v_all), abs(ev - ref["evidence"]) / abs(ref["evidence"]))
    print(f"{kname} {lik}: mode {e[0]:.2e} variance {e[1]:.2e} evidence {e[2]:.2e}; {m.fit_info}")
    assert m.fit_info["converged"] and max(e) <= DENSE_TOL
    with pytest.raises(NotImplementedError):
        m.log_likelihood_and_grad()


def test_gaussian_likelihood_is_the_gaussian_model():
    from pssgp.laplace import LaplaceStateSpaceGP
    from pssgp.model import StateSpaceGP
    t, y = LR.case("gaussian", 120)
    var = LR.PARS["gaussian"]
    gp = StateSpaceGP((t[:, None], y[:, None]), LR.matern("m32"), noise_variance=var, parallel=False)
    mean, v, ll = gp._predict_f_host(t)              # (the model's own host evaluation: no device needed)
    mean, v = mean[:, None], v[:, None]
    m = LaplaceStateSpaceGP((t[:, None], y[:, None]), LR.matern("m32"), _likelihood("gaussian"), parallel=False)
    f, fv = m.posterior_mode()
    ev = float(m.maximum_log_likelihood_objective())
    # one pass from f = 0 lands on the mode (the second moves nothing and stops the search)
    assert m.fit_info["converged"] and m.fit_info["iterations"] == 2 and m.fit_info["halvings"] == 0
    assert LR.rel(f, mean) <= 1e-10 and LR.rel(fv, v) <= 1e-10 and abs(ev - ll) <= 1e-10 * abs(ll)
    pm, pv = m.predict_y(t[:5, None])
    assert LR.rel(pv, v[:5] + var) <= 1e-10 and LR.rel(pm, mean[:5]) <= 1e-10


@pytest.fixture(scope="module")
def damping_case():
    """Poisson counts under a GP of variance 9, lengthscale 1, 200 times uniform on [0, 10]: Newton from f = 0 overshoots."""
    rng = np.random.default_rng(1)
    t = np.sort(rng.uniform(0.0, 10.0, 200))
    K = LR.matern_K("m32", 9.0, 1.0, t, t)
    latent = np.linalg.cholesky(K + 1e-10 * np.eye(200)) @ rng.standard_normal(200)
    return t, rng.poisson(np.exp(latent)).astype(float), K


def test_damping(damping_case):
    from pssgp.kernels import Matern32
    from pssgp.laplace import LaplaceStateSpaceGP
    from pssgp.likelihoods import Poisson
    t, y, K = damping_case
    assert LR.dense_laplace(K, y, "poisson", 1.0, damp=False)["diverged"]
    ref = LR.dense_laplace(K, y, "poisson", 1.0)
    assert not ref["diverged"] and ref["halvings"] > 0
    m = LaplaceStateSpaceGP((t[:, None], y[:, None]), Matern32(variance=9., lengthscales=1.), Poisson(), parallel=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        f, _ = m.posterior_mode()
    print(m.fit_info, ref["iterations"], ref["halvings"])
    assert m.fit_info["converged"] and m.fit_info["halvings"] > 0
    assert LR.rel(f[:, 0], ref["f"]) <= DENSE_TOL
    assert abs(float(m.maximum_log_likelihood_objective()) - ref["evidence"]) <= DENSE_TOL * abs(ref["evidence"])


def test_times_out_of_order_and_cache():
    from pssgp.laplace import LaplaceStateSpaceGP
    t, y = LR.case("poisson", 120)
    perm = np.random.RandomState(5).permutation(t.size)
    a = LaplaceStateSpaceGP((t[:, None], y[:, None]), LR.matern("m32"), _likelihood("poisson"), parallel=False)
    b = LaplaceStateSpaceGP((t[perm], y[perm]), LR.matern("m32"), _likelihood("poisson"), parallel=False)
    fa, va = a.posterior_mode()
    fb, vb = b.posterior_mode()
    assert np.array_equal(fa[perm], fb) and np.array_equal(va[perm], vb)
    assert a.maximum_log_likelihood_objective() == b.maximum_log_likelihood_objective()
    tq = np.array([0.9, 0.1, 0.5, 0.1])
    ma, _ = a.predict_f(tq[:, None])
    mb, _ = b.predict_f(tq[:, None])
    assert np.array_equal(ma, mb) and ma[1, 0] == ma[3, 0]
    # the search is cached until a parameter or the data is assigned
    fit = a.fit_mode()
    assert a.fit_mode() is fit
    a.kernel.lengthscales = 0.7
    assert a.fit_mode() is not fit
    fit = a.fit_mode()
    a.data = (t[:, None], y[:, None])
    assert a.fit_mode() is not fit
    assert [n for _, n in a.trainable_parameters()] == ["variance", "lengthscales"]
    # a search cut short warns and does not raise
    c = LaplaceStateSpaceGP((t[:, None], y[:, None]), LR.matern("m32"), _likelihood("poisson"), parallel=False, max_iter=1)
    with pytest.warns(RuntimeWarning, match="did not converge"):
        c.fit_mode()
    assert not c.fit_info["converged"] and c.fit_info["iterations"] == 1


def test_validate_errors():
    from pssgp.laplace import LaplaceStateSpaceGP
    from pssgp.likelihoods import Bernoulli, Gaussian, Poisson
    Bernoulli().validate(np.array([0.0, 1.0, np.nan]))
    Poisson().validate(np.array([0.0, 7.0, np.nan]))
    for L, bad in ((Bernoulli(), [0.0, 2.0]), (Bernoulli(), [0.5]), (Poisson(), [-1.0]), (Poisson(), [1.5]), (Poisson(), [np.inf])):
        with pytest.raises(ValueError):
            L.validate(np.array(bad))
    for make in (lambda: Gaussian(0.0), lambda: Gaussian(np.nan), lambda: Poisson(0.0), lambda: Poisson(-1.0)):
        with pytest.raises(ValueError):
            make()
    t = np.linspace(0.1, 1.0, 10)
    with pytest.raises(ValueError):
        LaplaceStateSpaceGP((t, np.full(10, 2.0)), LR.matern("m32"), Bernoulli(), parallel=False)
    with pytest.raises(ValueError):
        LaplaceStateSpaceGP((t, np.zeros((10, 2))), LR.matern("m32"), Bernoulli(), parallel=False)
    with pytest.raises(TypeError):
        LaplaceStateSpaceGP((t, np.zeros(10)), LR.matern("m32"), "bernoulli", parallel=False)


def _quadrature(fn, m, v, points=200):
    x, w = np.polynomial.hermite.hermgauss(points)
    return np.sum(fn(m[:, None] + np.sqrt(2.0 * v)[:, None] * x) * (w / np.sqrt(np.pi)), axis=1)


def test_predictive_laws_of_new_observations():
    from pssgp.laplace import LaplaceStateSpaceGP
    from pssgp.likelihoods import Bernoulli, Poisson
    t, y = LR.case("bernoulli", 120)
    m = LaplaceStateSpaceGP((t[:, None], y[:, None]), LR.matern("m32"), Bernoulli(), parallel=False)
    tq = np.linspace(0.0, 1.3, 40)
    mean, var = (a[:, 0] for a in m.predict_f(tq[:, None]))
    p, pv = (a[:, 0] for a in m.predict_y(tq[:, None]))
    want = _quadrature(lambda f: 1.0 / (1.0 + np.exp(-f)), mean, var)
    e = np.max(np.abs(p - want))
    print(f"Bernoulli predict_y against 200-point quadrature: {e:.2e} (variances up to {var.max():.3f})")
    assert e <= 1e-10 and np.allclose(pv, p * (1.0 - p), rtol=0, atol=1e-15)
    ynew = (np.arange(40) % 2).astype(float)
    ynew[3] = np.nan
    ld = m.predict_log_density((tq[:, None], ynew[:, None]))[:, 0]
    assert np.isnan(ld[3]) and np.max(np.abs(np.delete(ld, 3) - np.delete(np.log(np.where(ynew == 1.0, want, 1.0 - want)), 3))) <= 1e-9
    # Poisson: the closed forms are the log-normal moments of the rate
    L = Poisson(1.5)
    mm, vv = np.linspace(-1.0, 1.5, 30), np.linspace(0.01, 0.8, 30)
    pm, pvar = L.predict_mean_and_var(mm, vv)
    rate1 = _quadrature(lambda f: 1.5 * np.exp(f), mm, vv)
    rate2 = _quadrature(lambda f: (1.5 * np.exp(f)) ** 2, mm, vv)
    assert np.max(np.abs(pm / rate1 - 1.0)) <= 1e-10 and np.max(np.abs(pvar / (rate1 + rate2 - rate1 ** 2) - 1.0)) <= 1e-9
    # its log density: the 32-point rule the class documents, summed here directly instead of in the log domain
    from scipy.special import gammaln
    yy = np.arange(30.0) % 5
    want_ld = np.log(_quadrature(lambda f: np.exp(yy[:, None] * np.log(1.5 * np.exp(f)) - 1.5 * np.exp(f) - gammaln(yy + 1.0)[:, None]), mm, vv,
                                 points=32))
    assert np.max(np.abs(L.predict_log_density(mm, vv, yy) - want_ld)) <= 1e-12
