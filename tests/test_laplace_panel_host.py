"""LaplaceStateSpaceGPPanel off the device route (no GPU): parallel=False, and a kernel the device route does not take.  There
the class IS the loop of single LaplaceStateSpaceGP models, so every method is held to that loop bit for bit: shapes, data order
restored for unsorted times, empty and repeated queries, per-series thetas and exposures, parameters restored after an exception,
a long series, argument errors, the single warning, an all-NaN series."""
import warnings

import numpy as np
import pytest

import laplace_panel_refs as PR
from laplace_panel_refs import likelihood, matern

LENGTHS = (37, 1, 120, 2)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _panel(lik, **kw):
    from pssgp.laplace_panel import LaplaceStateSpaceGPPanel
    cases = PR.panel(lik, LENGTHS)
    return cases, LaplaceStateSpaceGPPanel(list(cases), kw.pop("kernel", None) or matern("m32"), kw.pop("likelihood", None) or likelihood(lik),
                                           parallel=False, **kw)


def _one(t, y, kernel, lik_obj, **kw):
    from pssgp.laplace import LaplaceStateSpaceGP
    return LaplaceStateSpaceGP((np.asarray(t)[:, None], np.asarray(y)[:, None]), kernel, lik_obj, parallel=False, **kw)


@pytest.mark.parametrize("lik", PR.LIKELIHOODS)
def test_every_method_is_the_loop(lik):
    cases, p = _panel(lik)
    rng = np.random.RandomState(2)
    Xnews = [rng.uniform(t[0] - 0.2, t[-1] + 0.2, k) for (t, _), k in zip(cases, (11, 0, 5, 3))]
    Xnews[0] = np.concatenate([Xnews[0], Xnews[0][:3]])                 # (repeated queries, any order)
    fits, ev, modes = p.fit_modes(), p.log_evidences(), p.posterior_modes()
    pf, py = p.predict_f(Xnews), p.predict_y(Xnews)
    pd = p.predict_log_density([(x, np.ones(x.size)) for x in Xnews])
    assert ev.shape == (len(cases),) and len(p.fit_info) == len(cases)
    total = 0.0
    for s, (t, y) in enumerate(cases):
        one = _one(t, y, matern("m32"), likelihood(lik))
        want = one.fit_mode()
        for k in ("f", "v", "z", "s"):
            assert _same(fits[s][k], want[k]), (s, k)
        assert fits[s]["log_evidence"] == want["log_evidence"] and p.fit_info[s] == one.fit_info
        assert ev[s] == one.maximum_log_likelihood_objective()
        total += float(ev[s])
        wm = one.posterior_mode()
        assert _same(modes[s][0], wm[0]) and _same(modes[s][1], wm[1]) and modes[s][0].shape == (t.size, 1)
        if Xnews[s].size == 0:
            assert pf[s][0].shape == (0, 1) and py[s][1].shape == (0, 1) and pd[s].shape == (0, 1)
            continue
        wf, wy = one.predict_f(Xnews[s][:, None]), one.predict_y(Xnews[s][:, None])
        wd = one.predict_log_density((Xnews[s][:, None], np.ones((Xnews[s].size, 1))))
        assert _same(pf[s][0], wf[0]) and _same(pf[s][1], wf[1]) and _same(py[s][0], wy[0]) and _same(py[s][1], wy[1]) and _same(pd[s], wd)
    assert abs(float(p.maximum_log_likelihood_objective()) - total) <= 1e-12 * abs(total)
    assert p.training_loss() == -p.maximum_log_likelihood_objective()
    with pytest.raises(NotImplementedError):
        p.log_evidences_and_grads()
    with pytest.raises(NotImplementedError):
        p.log_likelihood_and_grad()


def test_a_kernel_off_the_device_route_and_unsorted_times():
    from pssgp.kernels import RBF
    from pssgp.laplace_panel import LaplaceStateSpaceGPPanel
    cases = PR.panel("poisson", LENGTHS)
    rng = np.random.RandomState(4)
    shuffled = []
    for t, y in cases:
        o = rng.permutation(t.size)
        shuffled.append((t[o], y[o]))
    kern = RBF(variance=1.0, lengthscales=0.5, order=6, balancing_iter=5)
    p = LaplaceStateSpaceGPPanel(shuffled, kern, likelihood("poisson"), parallel=True)     # (parallel, but no Matern: the loop)
    assert p._fused() is None
    modes, ev = p.posterior_modes(), p.log_evidences()
    for s, (t, y) in enumerate(shuffled):
        one = _one(t, y, kern, likelihood("poisson"))
        one.parallel = True
        wm = one.posterior_mode()
        assert _same(modes[s][0], wm[0]) and _same(modes[s][1], wm[1]) and ev[s] == one.maximum_log_likelihood_objective()


def test_per_series_thetas_and_exposures_and_parameters_restored():
    from pssgp.kernels import Matern32
    cases = PR.panel("poisson", LENGTHS)
    S = len(cases)
    expo = [0.7, 1.5, 2.5, 1.0]
    kern = Matern32(variance=1.0, lengthscales=0.5)
    _, p = _panel("poisson", kernel=kern, likelihood=[likelihood("poisson", e) for e in expo])
    names = [n for _, n in p.trainable_parameters()]
    thetas = np.column_stack([np.linspace(0.6, 1.8, S), np.linspace(0.3, 0.9, S)])
    ev = p.log_evidences(thetas)
    assert [float(getattr(kern, n)) for n in names] == [1.0, 0.5]
    for s, (t, y) in enumerate(cases):
        k = Matern32(**{n: thetas[s, j] for j, n in enumerate(names)})
        assert ev[s] == _one(t, y, k, likelihood("poisson", expo[s])).maximum_log_likelihood_objective()
    bad = thetas.copy()
    bad[2, 1] = -1.0
    with pytest.raises(Exception):
        p.log_evidences(bad)
    assert [float(getattr(kern, n)) for n in names] == [1.0, 0.5]
    with pytest.raises(ValueError):
        p.log_evidences(thetas[:2])


def test_a_long_series_is_spliced():
    from pssgp import _backend as Bk
    from pssgp.laplace_panel import LaplaceStateSpaceGPPanel
    long_case = PR.panel("bernoulli", (Bk.PANEL_MAX_STEPS + 1,))[0]
    short = PR.panel("bernoulli", LENGTHS)[0]
    p = LaplaceStateSpaceGPPanel([short, long_case], matern("m12"), likelihood("bernoulli"), parallel=False)
    assert p._long == [1] and p._short == [0]
    ev = p.log_evidences()
    for s, (t, y) in enumerate((short, long_case)):
        assert ev[s] == _one(t, y, matern("m12"), likelihood("bernoulli")).maximum_log_likelihood_objective()


def test_argument_errors():
    from pssgp.laplace_panel import LaplaceStateSpaceGPPanel
    cases = list(PR.panel("poisson", LENGTHS))
    k = matern("m32")
    with pytest.raises(ValueError):
        LaplaceStateSpaceGPPanel([], k, likelihood("poisson"))
    with pytest.raises(TypeError):
        LaplaceStateSpaceGPPanel(cases, k, "poisson")
    with pytest.raises(ValueError):
        LaplaceStateSpaceGPPanel(cases, k, [likelihood("poisson")] * 2)
    with pytest.raises(ValueError):
        LaplaceStateSpaceGPPanel(cases, k, [likelihood("poisson")] * 3 + [likelihood("bernoulli")])
    with pytest.raises(ValueError):
        LaplaceStateSpaceGPPanel(cases + [(np.zeros(3), np.zeros(2))], k, likelihood("poisson"))
    with pytest.raises(ValueError):
        LaplaceStateSpaceGPPanel([(np.zeros(2), np.array([0.5, 1.0]))], k, likelihood("poisson"))      # (no count)
    p = LaplaceStateSpaceGPPanel(cases, k, likelihood("poisson"), parallel=False)
    with pytest.raises(ValueError):
        p.predict_f([np.zeros(1)])
    with pytest.raises(ValueError):
        p.log_evidences(np.ones((len(cases), 5)))


def test_one_warning_and_an_all_nan_series():
    cases = list(PR.panel("poisson", LENGTHS))
    t = cases[0][0]
    from pssgp.laplace_panel import LaplaceStateSpaceGPPanel
    p = LaplaceStateSpaceGPPanel(cases + [(t, np.full(t.size, np.nan))], matern("m32"), likelihood("poisson"), parallel=False, max_iter=2)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fits = p.fit_modes()
        p.log_evidences()                       # (cached: no second search, no second warning)
    late = [s for s, i in enumerate(p.fit_info) if not i["converged"]]
    assert late and len(caught) == 1 and issubclass(caught[0].category, RuntimeWarning)
    assert f"{len(late)} of {len(cases) + 1}" in str(caught[0].message)
    one = _one(t, np.full(t.size, np.nan), matern("m32"), likelihood("poisson"), max_iter=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = one.fit_mode()
    assert _same(fits[-1]["f"], want["f"]) and _same(fits[-1]["v"], want["v"]) and fits[-1]["log_evidence"] == want["log_evidence"]
    assert p.fit_info[-1] == one.fit_info
