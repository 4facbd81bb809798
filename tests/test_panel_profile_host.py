"""StateSpaceGPPanel.profile_log_likelihoods_and_grads on the host (parallel=False: the loop -- every series' solve first, then the
residual model's gradient, which the single model does not have off the device): what it raises, in which order, and that betas
and the panel's parameters are left as they were.  No GPU."""
import numpy as np
import pytest

import panel_trend_refs as T
from het_refs import R, matern
from pssgp.mean_functions import Linear
from pssgp.panel import StateSpaceGPPanel

LENGTHS = (37, 12, 16)
HET = pytest.mark.parametrize("het", [False, True], ids=["scalar", "rs"])


@pytest.fixture(autouse=True)
def host_discretisation(monkeypatch):
    """As in test_panel_host.py: the sequential path's one device call takes the model's own host discretisation."""
    from pssgp import _backend, model
    monkeypatch.setattr(_backend, "discretise", lambda F, Pinf, ts, t0=0.0, device=0: model._host_discretise(F, Pinf, ts, t0))


def _panel(het, series=None, mean_function="linear"):
    cases = list(T.panel(LENGTHS)) if series is None else series
    return StateSpaceGPPanel([(t, y) for t, y, _ in cases], matern("m32"), noise_variance=R, parallel=False,
                             observation_variances=[s for _, _, s in cases] if het else None,
                             mean_function=None if mean_function is None else T.bases()[mean_function])


def _setting(panel):
    return float(panel.kernel.variance), float(panel.kernel.lengthscales), float(panel.noise_variance)


@HET
def test_off_the_device_the_single_models_error_comes_through_with_nothing_moved(het):
    panel = _panel(het)
    before = np.arange(6.0).reshape(3, 2)
    panel.betas = before
    setting = _setting(panel)
    thetas = np.stack([[1.0 + 0.1 * i, 0.5 * (1.0 + 0.05 * i), R * (1.0 + 0.1 * i)] for i in range(3)])
    for kw in ({}, {"thetas": thetas}, {"reduce": "sum"}):
        with pytest.raises(NotImplementedError):
            panel.profile_log_likelihoods_and_grads(**kw)
        assert np.array_equal(panel.betas, before) and _setting(panel) == setting


@HET
def test_what_is_refused(het):
    panel = _panel(het)
    setting = _setting(panel)
    thetas = np.tile(np.array([1.0, 0.5, R]), (3, 1))
    with pytest.raises(ValueError, match="thetas has shape"):
        panel.profile_log_likelihoods_and_grads(thetas[:2])
    with pytest.raises(ValueError, match="thetas has shape"):
        panel.profile_log_likelihoods_and_grads(thetas[:, :2])
    with pytest.raises(ValueError, match="thetas must be None"):
        panel.profile_log_likelihoods_and_grads(thetas, reduce="sum")
    for bad in ("mean", "none", 0):
        with pytest.raises(ValueError, match="reduce must be"):
            panel.profile_log_likelihoods_and_grads(reduce=bad)
    assert _setting(panel) == setting and np.array_equal(panel.betas, np.zeros((3, 2)))
    with pytest.raises(ValueError, match="no mean_function"):
        _panel(het, mean_function=None).profile_log_likelihoods_and_grads()


@HET
def test_a_rank_deficient_series_is_named_before_any_gradient_is_asked_for(het):
    """Two observed rows at ONE time under Linear in series 2.  Off the device the first gradient would raise
    NotImplementedError: the ValueError shows that every solve came first."""
    cases = list(T.panel(LENGTHS))
    cases[2] = (np.array([0.2, 0.4, 0.4, 0.7]), np.array([np.nan, 0.3, -0.1, np.nan]), np.full(4, 0.02))
    panel = StateSpaceGPPanel([(t, y) for t, y, _ in cases], matern("m32"), noise_variance=R, parallel=False,
                              observation_variances=[s for _, _, s in cases] if het else None, mean_function=Linear())
    setting = _setting(panel)
    thetas = np.tile(np.array([1.1, 0.6, 1.5 * R]), (3, 1))
    for kw in ({}, {"thetas": thetas}, {"reduce": "sum"}):
        with pytest.raises(ValueError, match="series 2"):
            panel.profile_log_likelihoods_and_grads(**kw)
    assert np.array_equal(panel.betas, np.zeros((3, 2))) and _setting(panel) == setting
