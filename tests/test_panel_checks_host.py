"""The predictive checks of StateSpaceGPPanel on the host (parallel=False and kernels the device route does not take: the loop
over the S internal StateSpaceGP models, which is also the definition): one_step_ahead, leave_one_out and the leave-one-out
scores against the single models bit for bit, the caller's row order, NaN rows, observation_variances, per-series thetas, the
ValueError cases, and the argument checks of _backend.gp_panel_loo that need no device.  No GPU."""
import numpy as np
import pytest

from pssgp.kernels import RBF, Matern32
from pssgp.model import StateSpaceGP
from pssgp.panel import StateSpaceGPPanel

LENGTHS = (1, 2, 37, 120)
R = 0.1


@pytest.fixture(autouse=True)
def host_discretisation(monkeypatch):
    """As in test_panel_host.py: the sequential path's one device call takes the model's own host discretisation."""
    from pssgp import _backend, model
    monkeypatch.setattr(_backend, "discretise", lambda F, Pinf, ts, t0=0.0, device=0: model._host_discretise(F, Pinf, ts, t0))


def _series(n, seed):
    """Sorted times, a noisy sine, 20 % of the rows NaN (from 10 rows on; never all), given variances s."""
    rng = np.random.RandomState(700 + 7 * n + seed)
    t = np.sort(rng.rand(n)) * 3.0 + 0.05
    s = R * 10.0 ** rng.uniform(-2.0, 0.0, n)
    y = np.sin(2.0 * t) + np.sqrt(R + s) * rng.randn(n)
    if n >= 10:
        y[rng.rand(n) < 0.2] = np.nan
        y[n // 2] = 0.3
    return t, y, s


def _kernel(name):
    if name == "m32":
        return Matern32(variance=1.2, lengthscales=0.7)
    return RBF(variance=1.2, lengthscales=0.7, order=4, balancing_iter=5)


def _data():
    return [_series(n, i) for i, n in enumerate(LENGTHS)]


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


def _singles(data, kname, het, parallel=False):
    return [StateSpaceGP((t[:, None], y[:, None]), _kernel(kname), noise_variance=R, parallel=parallel,
                         observation_variances=s if het else None) for t, y, s in data]


def _check_equal_to_singles(panel, singles, what):
    osa, loo, lpd = panel.one_step_ahead(), panel.leave_one_out(), panel.loo_log_predictive_densities()
    assert len(osa) == len(loo) == len(singles) and lpd.shape == (len(singles),)
    for i, m in enumerate(singles):
        n = m.data[0].shape[0]
        for got, want, name in ((osa[i], m.one_step_ahead(), "one_step_ahead"), (loo[i], m.leave_one_out(), "leave_one_out")):
            assert len(got) == 3
            for g, w, part in zip(got, want, ("mean", "var", "log_density")):
                assert g.shape == (n, 1)
                _same_bits(g, w, (what, name, part, i))
        _same_bits(lpd[i], m.loo_log_predictive_density(), (what, "loo_lpd", i))
    _same_bits(panel.loo_log_predictive_density(), lpd.dtype.type(np.sum(lpd)), (what, "the sum"))


@pytest.mark.parametrize("kname,parallel", [("m32", False), ("rbf4", False), ("rbf4", True)],
                         ids=["m32-sequential", "rbf-sequential", "rbf-parallel-flag"])
@pytest.mark.parametrize("het", [False, True], ids=["scalar", "het"])
def test_every_entry_equals_the_single_models_bit_for_bit(kname, parallel, het):
    """parallel=False, and an RBF kernel (no device route for the checks in either mode: the single model takes its host
    twin)."""
    data = _data()
    panel = StateSpaceGPPanel([(t, y) for t, y, _ in data], _kernel(kname), noise_variance=R, parallel=parallel,
                              observation_variances=[s for _, _, s in data] if het else None)
    _check_equal_to_singles(panel, _singles(data, kname, het, parallel), f"{kname} parallel {parallel} het {het}")


@pytest.mark.parametrize("het", [False, True], ids=["scalar", "het"])
def test_rows_come_back_in_the_order_they_were_given_and_nan_rows(het):
    data = _data()
    rng = np.random.RandomState(3)
    perms = [rng.permutation(t.size) for t, _, _ in data]
    obs = lambda sel: [sel(s, p) for (_, _, s), p in zip(data, perms)] if het else None
    ordered = StateSpaceGPPanel([(t, y) for t, y, _ in data], _kernel("m32"), noise_variance=R, parallel=False,
                                observation_variances=obs(lambda s, p: s))
    shuffled = StateSpaceGPPanel([(t[p], y[p]) for (t, y, _), p in zip(data, perms)], _kernel("m32"), noise_variance=R,
                                 parallel=False, observation_variances=obs(lambda s, p: s[p]))
    assert any(o is not None for o in shuffled._orders)
    for name in ("one_step_ahead", "leave_one_out"):
        want, got = getattr(ordered, name)(), getattr(shuffled, name)()
        for i, ((t, y, _), p) in enumerate(zip(data, perms)):
            for g, w, part in zip(got[i], want[i], ("mean", "var", "log_density")):
                _same_bits(g, w[p], (name, part, i))
            # log_density is NaN exactly at the NaN rows of y (as given); mean and var are finite everywhere
            assert np.array_equal(np.isnan(got[i][2][:, 0]), np.isnan(y[p]))
            assert np.all(np.isfinite(got[i][0])) and np.all(got[i][1] > 0.0)
    _same_bits(shuffled.loo_log_predictive_densities(), ordered.loo_log_predictive_densities(), "scores")
    # the single model on the shuffled rows sorts and puts back by itself: the same bits
    i = 3
    t, y, s = data[i]
    m = StateSpaceGP((t[perms[i]][:, None], y[perms[i]][:, None]), _kernel("m32"), noise_variance=R, parallel=False,
                     observation_variances=s[perms[i]] if het else None)
    for g, w in zip(shuffled.leave_one_out()[i], m.leave_one_out()):
        _same_bits(g, w, "the single model on the shuffled rows")
    # the scores are the sums of the log densities over the observed rows, and the one-step-ahead ones sum to the likelihoods
    lpd, lls = ordered.loo_log_predictive_densities(), ordered.log_likelihoods()
    for i, (o, l) in enumerate(zip(ordered.one_step_ahead(), ordered.leave_one_out())):
        assert abs(np.nansum(l[2]) - lpd[i]) <= 1e-12 * abs(lpd[i])
        assert abs(np.nansum(o[2]) - lls[i]) <= 1e-10 * abs(lls[i])


def test_thetas_row_s_is_the_single_model_with_row_s_assigned():
    data = _data()
    pairs = [(t, y) for t, y, _ in data]
    panel = StateSpaceGPPanel(pairs, _kernel("m32"), noise_variance=R, parallel=False)
    rng = np.random.RandomState(11)
    thetas = np.stack([rng.uniform(0.5, 2.0, 4), rng.uniform(0.3, 1.5, 4), rng.uniform(0.05, 0.3, 4)], axis=1)
    osa, loo, lpd = panel.one_step_ahead(thetas), panel.leave_one_out(thetas), panel.loo_log_predictive_densities(thetas)
    for s, (t, y) in enumerate(pairs):
        m = StateSpaceGP((t[:, None], y[:, None]), Matern32(variance=thetas[s, 0], lengthscales=thetas[s, 1]),
                         noise_variance=thetas[s, 2], parallel=False)
        for g, w in zip(osa[s] + loo[s], m.one_step_ahead() + m.leave_one_out()):
            _same_bits(g, w, ("thetas", s))
        _same_bits(lpd[s], m.loo_log_predictive_density(), ("thetas score", s))
    assert np.ptp(lpd - panel.loo_log_predictive_densities()) > 1e-3         # (the rows move the results)
    # the panel's own parameters are left as they were
    assert (float(panel.kernel.variance), float(panel.kernel.lengthscales), panel.noise_variance) == (1.2, 0.7, R)
    with pytest.raises(ValueError):
        panel.leave_one_out(thetas[:3])


def test_value_errors():
    data = _data()
    pairs = [(t, y) for t, y, _ in data]
    free = StateSpaceGPPanel(pairs, _kernel("m32"), noise_variance=0.0, parallel=False)
    for call in (free.one_step_ahead, free.leave_one_out, free.loo_log_predictive_densities, free.loo_log_predictive_density):
        with pytest.raises(ValueError, match="noise_variance"):
            call()
    ok = StateSpaceGPPanel(pairs, _kernel("m32"), noise_variance=R, parallel=False)
    thetas = np.tile([1.2, 0.7, R], (4, 1))
    thetas[2, 2] = 0.0
    with pytest.raises(ValueError, match="noise_variance"):
        ok.leave_one_out(thetas)
    assert ok.noise_variance == R
    # with observation_variances: noise_variance + s_k must be > 0 wherever y is observed
    zeros = [np.zeros(t.size) for t, _ in pairs]
    het = StateSpaceGPPanel(pairs, _kernel("m32"), noise_variance=0.0, parallel=False, observation_variances=zeros)
    with pytest.raises(ValueError, match="observation_variances"):
        het.leave_one_out()
    # ... and only there: a zero at a missing row is no error
    t, y, s = data[3]
    s = s.copy()
    s[np.isnan(y)] = 0.0
    fine = StateSpaceGPPanel([(t, y)], _kernel("m32"), noise_variance=0.0, parallel=False, observation_variances=[s])
    assert np.all(np.isfinite(fine.leave_one_out()[0][0]))


def test_the_rule_of_the_device_route_is_the_single_models():
    """_check_noise, which the device route asks before its one call (no single model is asked there), on a panel that never
    touches a device."""
    data = _data()
    pairs = [(t, y) for t, y, _ in data]
    panel = StateSpaceGPPanel(pairs, _kernel("m32"), noise_variance=R, parallel=False)
    panel._check_noise(None)
    thetas = np.tile([1.2, 0.7, R], (4, 1))
    thetas[1, 2] = -0.5
    with pytest.raises(ValueError, match="noise_variance"):
        panel._check_noise(thetas)
    s = [c[2].copy() for c in data]
    s[3][np.flatnonzero(~np.isnan(data[3][1]))[5]] = 0.0            # one observed row of one series without noise of its own
    het = StateSpaceGPPanel(pairs, _kernel("m32"), noise_variance=R, parallel=False, observation_variances=s)
    het._check_noise(None)
    thetas[1, 2] = R
    thetas[3, 2] = 0.0
    with pytest.raises(ValueError, match="observation_variances"):
        het._check_noise(thetas)
    thetas[3, 2], thetas[0, 2] = R, 0.0                             # (series 0 has given variances > 0 everywhere)
    het._check_noise(thetas)


def test_backend_argument_checks_need_no_device():
    from pssgp import _backend as Bk
    sde = _kernel("m32").get_sde()
    model = (Bk.nilpotent_form(sde.F), np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1), R)
    t, y, s = _series(20, 0)
    offs = np.array([0, 12, 20])
    with pytest.raises(ValueError, match="offs"):
        Bk.gp_panel_loo([model], [3, 20], t, y)
    with pytest.raises(ValueError, match="offs"):
        Bk.gp_panel_loo([model], [0], t, y)
    with pytest.raises(ValueError, match="ys has"):
        Bk.gp_panel_loo([model], offs, t, y[:-1])
    with pytest.raises(ValueError, match="rs has"):
        Bk.gp_panel_loo([model], offs, t, y, s[:-1])
    with pytest.raises(ValueError, match="1 model"):
        Bk.gp_panel_loo([model] * 3, offs, t, y)
    assert Bk.panel.gp_panel_loo is Bk.gp_panel_loo and callable(Bk.panel.gp_panel_loo_dev)
