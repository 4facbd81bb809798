"""StateSpaceGPPanel.fit_each and its twin on the host (no GPU): pssgp.fitting.bfgs_box over the ORACLE's log-likelihood and
gradient (oracle.np_grad) converges on the series the GPU tests use; argument validation; the NotImplementedError of a panel
whose single models have no gradient; `wrt` keeps the fixed columns bit for bit."""
import warnings

import numpy as np
import pytest

import panel_fit_refs as R
from pssgp import fitting
from pssgp.kernels import Matern32
from pssgp.panel import StateSpaceGPPanel

# length -> seed of R.series: chosen so that the oracle's own searches converge (the two-row likelihood has flat directions; its
# search crawls along them for some draws)
SEEDS = {1: 0, 2: 2, 37: 2, 257: 4}


def _oracle_panel(name, lengths, unit):
    data = [R.series(n, SEEDS[n]) for n in lengths]
    n_obs = np.array([np.count_nonzero(~np.isnan(y)) for _, y, _ in data], np.float64)

    def lls_and_grads(thetas):
        out = [R.oracle_ll_and_grad(name, th, t, y, None, unit) for th, (t, y, _) in zip(thetas, data)]
        return np.array([o[0] for o in out]), np.stack([o[1] for o in out])

    return data, n_obs, lls_and_grads


@pytest.mark.parametrize("name", list(R.KERNELS))
def test_twin_converges_on_the_oracle(name):
    """Scalar noise, NaN rows, n in {1, 2, 37, 257} in lock step: status 0 within max_iter = 60 for every series, the
    log-likelihood does not fall, and (n >= 37) the Hessian of f in x at the optimum has lam_min >= 1e-3: the condition the
    GPU test's comparison of the two routes puts on its inputs."""
    lengths = (1, 2, 37, 257)
    data, n_obs, lls_and_grads = _oracle_panel(name, lengths, R.unit52())
    free = np.ones(3, bool)
    t0 = np.tile(np.array(R.START), (len(lengths), 1))
    x0, xlo, xhi = fitting.log_box(t0, t0 * 1e-4, t0 * 1e4, free)
    r = fitting.bfgs_box(lambda X: R.objective(lls_and_grads, np.exp(X), n_obs, free), x0, xlo, xhi, free, R.GTOL, R.MAX_ITER)
    print(name, "iterations", r.iterations, "evaluations", r.evaluations, "max |q|", r.grad_norm)
    assert np.all(r.status == fitting.STATUS_CONVERGED), r.status
    assert np.all(r.iterations <= R.MAX_ITER) and np.all(r.grad_norm <= R.GTOL)
    assert np.all(r.f <= r.f0)
    assert np.all(r.evaluations <= 1 + 2 * (fitting.FIT_MAX_HALVINGS + 1) * R.MAX_ITER)
    long_ = [i for i, n in enumerate(lengths) if n >= 37]
    lam_min = R.hessian_min_eigenvalues(lambda th: tuple(a[long_] for a in lls_and_grads(_rows(th, long_, t0))), np.exp(r.x)[long_],
                                        n_obs[long_], free)
    print(name, "lam_min", lam_min)
    assert np.all(lam_min >= 1e-3), lam_min


def _rows(th, rows, like):
    full = np.array(like, np.float64)
    full[rows] = th
    return full


def _host_panel(obs=False, noise=0.3):
    data = [R.series(n, SEEDS[n]) for n in (1, 2, 37)] + [R.series(5, 9, nan_only=True)]
    panel = StateSpaceGPPanel([(t, y) for t, y, _ in data], Matern32(variance=1.2, lengthscales=0.7), noise_variance=noise, parallel=False,
                              observation_variances=[s for _, _, s in data] if obs else None)
    return data, panel


def test_argument_validation():
    _, panel = _host_panel()
    S = panel.num_series
    ok = np.tile([1.0, 1.0, 0.5], (S, 1))
    bad_calls = [
        dict(thetas0=np.ones((S, 2))),                                  # shape
        dict(thetas0=np.ones((S + 1, 3))),
        dict(thetas0=_rows([0.0, 1.0, 1.0], 1, ok)),                    # a free start that is not > 0
        dict(thetas0=_rows([np.nan, 1.0, 1.0], 1, ok)),
        dict(thetas0=_rows([np.inf, 1.0, 1.0], 0, ok)),
        dict(wrt=[3]), dict(wrt=[-1]),
        dict(bounds=(np.ones(3),)),                                     # not a pair
        dict(bounds=(np.ones(2), np.ones(2))),                          # shape
        dict(bounds=(np.ones(3), np.ones(3))),                          # lower >= upper
        dict(bounds=(np.array([0.0, 0.1, 0.1]), 10.0 * np.ones(3))),    # a bound that is not > 0
        dict(bounds=(0.1 * np.ones(3), np.array([10.0, np.inf, 10.0]))),
        dict(gtol=-1e-6), dict(gtol=np.nan), dict(gtol=np.inf),
        dict(max_iter=0), dict(max_iter=fitting.FIT_MAX_ITER_CAP + 1), dict(max_iter=2.5),
        dict(thetas0=_rows([1.0, 1.0, 0.0], 2, ok), wrt=[0, 1]),        # noise_variance fixed at 0 without observation_variances
        dict(thetas0=_rows([1.0, -1.0, 0.5], 2, ok), wrt=[0, 2]),       # a fixed lengthscale that is not > 0
    ]
    for kwargs in bad_calls:
        with pytest.raises(ValueError):
            panel.fit_each(**kwargs)
    assert (panel.kernel.variance, panel.kernel.lengthscales, panel.noise_variance) == (1.2, 0.7, 0.3)


def test_no_gradient_raises_not_implemented():
    """parallel=False: the single models have no gradient; fit_each raises their NotImplementedError on either route, as
    log_likelihoods_and_grads does, and leaves the panel's parameters as they were."""
    _, panel = _host_panel()
    for in_kernel in (True, False):
        with pytest.raises(NotImplementedError):
            panel.fit_each(in_kernel=in_kernel)
    with pytest.raises(NotImplementedError):
        panel.log_likelihoods_and_grads()
    assert (panel.kernel.variance, panel.kernel.lengthscales, panel.noise_variance) == (1.2, 0.7, 0.3)


def test_wrt_keeps_fixed_columns_and_results_are_the_twins(monkeypatch):
    """fit_each over an evaluation handed in from outside (the oracle's, in place of the panel's own gradient call): rows are
    bfgs_box's; the columns that are not free come back bit for bit, whatever their value; a series without an observed row
    returns its start with status 0 and 0 iterations; ONE RuntimeWarning counts the series that did not converge."""
    data, panel = _host_panel()
    S = panel.num_series

    def lls_and_grads(thetas):
        out = [R.oracle_ll_and_grad("Matern32", th, t, y) for th, (t, y, _) in zip(thetas, data)]
        return np.array([o[0] for o in out]), np.stack([o[1] for o in out])

    monkeypatch.setattr(panel, "log_likelihoods_and_grads", lls_and_grads, raising=True)
    rng = np.random.RandomState(3)
    theta0 = np.exp(rng.uniform(-1.0, 1.0, (S, 3)))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fit = panel.fit_each(theta0, wrt=[0, 1], gtol=R.GTOL, max_iter=R.MAX_ITER)
    assert np.all(fit.status == fitting.STATUS_CONVERGED)
    assert np.array_equal(fit.thetas[:, 2], theta0[:, 2])               # bit for bit
    assert np.all(fit.thetas[2, :2] != theta0[2, :2])                   # (the free ones moved)
    assert np.array_equal(fit.thetas[3], theta0[3]) and fit.iterations[3] == 0 and fit.evaluations[3] == 1
    assert fit.log_likelihoods[3] == 0.0
    assert np.all(fit.log_likelihoods >= fit.start_log_likelihoods)
    lls, grads = lls_and_grads(fit.thetas)
    np.testing.assert_allclose(fit.log_likelihoods, lls, rtol=1e-12, atol=1e-12)
    n_obs = np.array([np.count_nonzero(~np.isnan(y)) for _, y, _ in data], np.float64)
    g = R.objective(lls_and_grads, fit.thetas, n_obs, [1, 1, 0])[1]
    assert np.all(R.projected_gradient_norm(g, fit.thetas, theta0 * 1e-4, theta0 * 1e4) <= R.GTOL)
    assert np.all(fit.thetas >= theta0 * 1e-4) and np.all(fit.thetas <= theta0 * 1e4)
    assert (panel.kernel.variance, panel.kernel.lengthscales, panel.noise_variance) == (1.2, 0.7, 0.3)

    # an upper bound on the lengthscale below its optimum: the fit ends ON the bound, bit for bit, converged
    cap = 0.5 * fit.thetas[2, 1]
    hi = theta0 * 1e4
    hi[:, 1] = np.where(np.arange(S) == 2, cap, hi[:, 1])
    start = theta0.copy()
    start[2, 1] = 0.25 * cap
    bounded = panel.fit_each(start, wrt=[0, 1], bounds=(np.minimum(theta0, start) * 1e-4, hi), gtol=R.GTOL, max_iter=R.MAX_ITER)
    assert bounded.status[2] == fitting.STATUS_CONVERGED and bounded.thetas[2, 1] == cap

    # ONE warning, with the count
    with pytest.warns(RuntimeWarning, match=r"fit_each: 3 of 4 series") as caught:
        one = panel.fit_each(theta0, max_iter=1)
    assert len(caught) == 1
    assert list(one.status) == [fitting.STATUS_MAX_ITER] * 3 + [fitting.STATUS_CONVERGED] and list(one.iterations) == [1, 1, 1, 0]
