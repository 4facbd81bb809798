"""StateSpaceGPPanel on the host (parallel=False: the loop over S internal StateSpaceGP models, which is also the definition of
the panel): construction and validation, every output against the S single models, the caller's order of times and queries,
per-series thetas.  No GPU."""
import numpy as np
import pytest

from pssgp.kernels import RBF, Matern32
from pssgp.model import StateSpaceGP
from pssgp.panel import StateSpaceGPPanel

LENGTHS = (1, 2, 37, 120)
TOL = 1e-12
R = 0.1


@pytest.fixture(autouse=True)
def host_discretisation(monkeypatch):
    """StateSpaceGP's sequential path builds its LGSSM through _backend.discretise, which runs on the device even with
    parallel=False; these tests have no GPU, so that one call takes the model's own host discretisation (expm per step), as
    in test_het_noise_host.py."""
    from pssgp import _backend, model
    monkeypatch.setattr(_backend, "discretise", lambda F, Pinf, ts, t0=0.0, device=0: model._host_discretise(F, Pinf, ts, t0))


def _series(n, seed):
    """Sorted times, a noisy sine, 20 % of the rows NaN (from 10 rows on; never all), given variances s."""
    rng = np.random.RandomState(500 + 7 * n + seed)
    t = np.sort(rng.rand(n)) * 3.0 + 0.05
    s = R * 10.0 ** rng.uniform(-2.0, 0.0, n)
    y = np.sin(2.0 * t) + np.sqrt(R + s) * rng.randn(n)
    if n >= 10:
        y[rng.rand(n) < 0.2] = np.nan
        y[n // 2] = 0.3
    return t, y, s


def _queries(t, k, seed):
    rng = np.random.RandomState(90 + k + seed)
    return np.sort(rng.uniform(t[0] - 0.2, t[-1] + 0.2, k))


def _kernel(name):
    if name == "m32":
        return Matern32(variance=1.2, lengthscales=0.7)
    return RBF(variance=1.2, lengthscales=0.7, order=4, balancing_iter=5)


def _data():
    return [_series(n, i) for i, n in enumerate(LENGTHS)]


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b))), (a, b)


def test_construction_and_validation():
    data = _data()
    pairs = [(t, y) for t, y, _ in data]
    p = StateSpaceGPPanel(pairs, _kernel("m32"), noise_variance=R, parallel=False)
    assert p.num_series == 4 and len(p.data) == 4
    assert [name for _, name in p.trainable_parameters()] == ["variance", "lengthscales", "noise_variance"]
    assert p.trainable_parameters()[-1][0] is p
    # (n,) and (n, 1) are the same series
    q = StateSpaceGPPanel([(t[:, None], y[:, None]) for t, y in pairs], _kernel("m32"), noise_variance=R, parallel=False)
    assert np.array_equal(p.log_likelihoods(), q.log_likelihoods())
    with pytest.raises(ValueError):
        StateSpaceGPPanel([], _kernel("m32"), parallel=False)
    with pytest.raises(ValueError):
        StateSpaceGPPanel([(np.zeros((3, 2)), np.zeros(3))], _kernel("m32"), parallel=False)
    with pytest.raises(ValueError):
        StateSpaceGPPanel([(np.zeros(3), np.zeros(4))], _kernel("m32"), parallel=False)
    with pytest.raises(ValueError, match="empty"):
        StateSpaceGPPanel(pairs[:2] + [(np.zeros(0), np.zeros(0))], _kernel("m32"), parallel=False)
    # observation_variances: one entry per series, each as long as its series, finite and >= 0 where y is observed
    with pytest.raises(ValueError):
        StateSpaceGPPanel(pairs, _kernel("m32"), parallel=False, observation_variances=[s for _, _, s in data][:3])
    bad = [s for _, _, s in data]
    bad[2] = bad[2][:-1]
    with pytest.raises(ValueError):
        StateSpaceGPPanel(pairs, _kernel("m32"), parallel=False, observation_variances=bad)
    neg = [s.copy() for _, _, s in data]
    neg[3][np.flatnonzero(~np.isnan(data[3][1]))[0]] = -1.0
    with pytest.raises(ValueError):
        StateSpaceGPPanel(pairs, _kernel("m32"), parallel=False, observation_variances=neg)
    with pytest.raises(ValueError):
        p.log_likelihoods(thetas=np.ones((3, 3)))
    with pytest.raises(ValueError):
        p.predict_f([np.zeros(2)] * 3)


@pytest.mark.parametrize("kname", ["m32", "rbf4"])
@pytest.mark.parametrize("het", [False, True], ids=["scalar", "het"])
def test_every_output_equals_the_single_models(kname, het):
    data = _data()
    pairs = [(t, y) for t, y, _ in data]
    obs = [s for _, _, s in data] if het else None
    panel = StateSpaceGPPanel(pairs, _kernel(kname), noise_variance=R, parallel=False, observation_variances=obs)
    singles = [StateSpaceGP((t[:, None], y[:, None]), _kernel(kname), noise_variance=R, parallel=False,
                            observation_variances=s if het else None) for t, y, s in data]
    lls = panel.log_likelihoods()
    assert lls.shape == (4,)
    _close(lls, [m.maximum_log_likelihood_objective() for m in singles])
    _close(panel.maximum_log_likelihood_objective(), np.sum(lls))
    _close(panel.training_loss(), -np.sum(lls))
    Xnews = [_queries(t, k, i) for i, ((t, _, _), k) in enumerate(zip(data, (3, 0, 11, 20)))]
    out = panel.predict_f(Xnews)
    assert len(out) == 4
    for (mean, var), m, x in zip(out, singles, Xnews):
        assert mean.shape == (x.size, 1) and var.shape == (x.size, 1)
        if x.size:
            wm, wv = m.predict_f(x[:, None])
            _close(mean, wm)
            _close(var, wv)
    empty = panel.predict_f([np.zeros(0)] * 4)
    assert all(m.shape == (0, 1) and v.shape == (0, 1) for m, v in empty)
    # the single model has no gradient on the host: the panel raises its NotImplementedError
    with pytest.raises(NotImplementedError):
        panel.log_likelihoods_and_grads()
    with pytest.raises(NotImplementedError):
        panel.log_likelihood_and_grad()


def test_unsorted_times_and_repeated_unsorted_queries_come_back_in_the_callers_order():
    data = _data()
    rng = np.random.RandomState(3)
    perms = [rng.permutation(t.size) for t, _, _ in data]
    sorted_panel = StateSpaceGPPanel([(t, y) for t, y, _ in data], _kernel("m32"), noise_variance=R, parallel=False,
                                     observation_variances=[s for _, _, s in data])
    shuffled = StateSpaceGPPanel([(t[p], y[p]) for (t, y, _), p in zip(data, perms)], _kernel("m32"), noise_variance=R,
                                 parallel=False, observation_variances=[s[p] for (_, _, s), p in zip(data, perms)])
    _close(shuffled.log_likelihoods(), sorted_panel.log_likelihoods())
    base = [_queries(t, 9, i) for i, (t, _, _) in enumerate(data)]
    picks = [rng.randint(0, 9, 15) for _ in data]               # repeated and out of order
    want = sorted_panel.predict_f(base)
    got = shuffled.predict_f([b[p] for b, p in zip(base, picks)])
    for (wm, wv), (gm, gv), p in zip(want, got, picks):
        _close(gm, wm[p])
        _close(gv, wv[p])


def test_thetas_row_s_is_the_single_model_with_row_s_assigned():
    data = _data()
    pairs = [(t, y) for t, y, _ in data]
    panel = StateSpaceGPPanel(pairs, _kernel("m32"), noise_variance=R, parallel=False)
    rng = np.random.RandomState(11)
    thetas = np.stack([rng.uniform(0.5, 2.0, 4), rng.uniform(0.3, 1.5, 4), rng.uniform(0.05, 0.3, 4)], axis=1)
    Xnews = [_queries(t, 5, i) for i, (t, _, _) in enumerate(data)]
    lls = panel.log_likelihoods(thetas)
    out = panel.predict_f(Xnews, thetas)
    for s, (t, y) in enumerate(pairs):
        m = StateSpaceGP((t[:, None], y[:, None]), Matern32(variance=thetas[s, 0], lengthscales=thetas[s, 1]),
                         noise_variance=thetas[s, 2], parallel=False)
        _close(lls[s], m.maximum_log_likelihood_objective())
        wm, wv = m.predict_f(Xnews[s][:, None])
        _close(out[s][0], wm)
        _close(out[s][1], wv)
    assert np.ptp(lls - panel.log_likelihoods()) > 1e-3          # (the rows move the results)
    # the panel's own parameters are untouched
    assert (float(panel.kernel.variance), float(panel.kernel.lengthscales), panel.noise_variance) == (1.2, 0.7, R)
