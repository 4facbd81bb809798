"""Mean functions of StateSpaceGPPanel on the host (parallel=False: the loop over the series -- a StateSpaceGP with the mean
function per series for scalar noise, panel_trend.whiten_host with observation_variances): the GLS coefficients and the
profile / flat-mean likelihoods against the references of panel_trend_refs.py, entry s against the single model, per-series
thetas, the caller's order of rows, a rank-deficient series, and mean_function=None.  No GPU."""
import numpy as np
import pytest

import panel_trend_refs as T
from het_refs import MATERNS, R, matern, sde_of
from pssgp.mean_functions import Linear
from pssgp.model import StateSpaceGP
from pssgp.panel import StateSpaceGPPanel

LENGTHS = (257, 12, 700, 37, 16)
TOL = 1e-12                     # (test_panel_host.py's: the panel against the single models)
TOL_SS = 1e-9                   # against the state-space reference
HET = pytest.mark.parametrize("het", [False, True], ids=["scalar", "rs"])
BASES = ("constant", "linear", "quadratic", "cubic")


@pytest.fixture(autouse=True)
def host_discretisation(monkeypatch):
    """As in test_panel_host.py: the sequential path's one device call takes the model's own host discretisation."""
    from pssgp import _backend, model
    monkeypatch.setattr(_backend, "discretise", lambda F, Pinf, ts, t0=0.0, device=0: model._host_discretise(F, Pinf, ts, t0))


def _panel(kname, het, basis, lengths=LENGTHS, order=None):
    cases = T.panel(lengths)
    order = [None] * len(cases) if order is None else order
    pick = lambda a, o: a if o is None else a[o]
    return StateSpaceGPPanel([(pick(t, o), pick(y, o)) for (t, y, _), o in zip(cases, order)], matern(kname), noise_variance=R,
                             parallel=False, observation_variances=[pick(s, o) for (_, _, s), o in zip(cases, order)] if het else None,
                             mean_function=T.bases()[basis])


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("kname", T.KNAMES)
@HET
@pytest.mark.parametrize("basis", BASES)
def test_gls_against_the_references(kname, het, basis):
    cases = T.panel(LENGTHS)
    refs = []
    for i, (t, y, s) in enumerate(cases):
        G, logdet, n_obs = T.ref_gram(kname, LENGTHS, i, het, basis)
        T.well_posed(G, logdet, n_obs, (kname, het, basis, i))          # (before anything is computed by the code under test)
        refs.append((T.gls_from_gram(G, logdet, n_obs), T.dense_gls(T.spec_of(kname), t, y, T.design(basis, t), R, s if het else None)))
    panel = _panel(kname, het, basis)
    betas, covs, profiles = panel.mean_coefficients()
    flats = panel.log_marginal_likelihoods_flat_mean()
    grams = panel.mean_grams()
    p = T.design(basis, np.zeros(1)).shape[1]
    assert betas.shape == (len(cases), p) and covs.shape == (len(cases), p, p) and profiles.shape == flats.shape == (len(cases),)
    assert np.array_equal(profiles, panel.profile_log_likelihoods())
    tol_d = MATERNS[kname][2]
    for i, (ss, dense) in enumerate(refs):
        G_ref, logdet_ref, n_ref = T.ref_gram(kname, LENGTHS, i, het, basis)
        dg = np.sqrt(np.diag(G_ref))
        e = [float(np.max(np.abs(grams[i].G - G_ref) / np.outer(dg, dg))), abs(grams[i].logdet - logdet_ref) / abs(logdet_ref),
             _rel(betas[i], ss[0]), _rel(covs[i], ss[1]), abs(profiles[i] - ss[2]) / abs(ss[2]), abs(flats[i] - ss[3]) / abs(ss[3])]
        print(f"{kname} rs {het} {basis} series {i} against the state-space reference: " + " ".join(f"{x:.2e}" for x in e))
        assert grams[i].n_obs == n_ref
        assert max(e) <= TOL_SS, (i, e)
        np.testing.assert_allclose(betas[i], dense[0], rtol=tol_d, atol=tol_d)
        np.testing.assert_allclose(covs[i], dense[1], rtol=tol_d, atol=tol_d)
        np.testing.assert_allclose([profiles[i], flats[i]], dense[2:], rtol=tol_d, atol=tol_d)


@pytest.mark.parametrize("basis", ("constant", "cubic"))
def test_scalar_noise_is_the_single_model(basis):
    """Entry s is StateSpaceGP(..., mean_function=...) on series s alone; so are the evaluations at the fitted betas."""
    cases = T.panel(LENGTHS)
    panel = _panel("m32", False, basis)
    betas, covs, profiles = panel.mean_coefficients()
    flats = panel.log_marginal_likelihoods_flat_mean()
    fitted = panel.fit_mean_functions()
    assert np.array_equal(fitted, betas) and np.array_equal(panel.betas, betas)
    lls = panel.log_likelihoods()
    Xnews = [np.linspace(0.0, 1.2, 7)] * len(cases)
    pred = panel.predict_f(Xnews)
    osa = panel.one_step_ahead()
    for i, (t, y, _) in enumerate(cases):
        m = StateSpaceGP((t[:, None], y[:, None]), matern("m32"), noise_variance=R, parallel=False, mean_function=T.bases()[basis])
        b, c, pr = m.mean_coefficients()
        for got, want in ((betas[i], b), (covs[i], c), (profiles[i], pr), (flats[i], m.log_marginal_likelihood_flat_mean())):
            assert np.all(np.abs(np.asarray(got) - np.asarray(want)) <= TOL * np.maximum(1.0, np.abs(want))), (i, got, want)
        m.fit_mean_function()
        w_mean, w_var = m.predict_f(Xnews[i][:, None])
        w_osa = m.one_step_ahead()
        for got, want in ((lls[i], m.maximum_log_likelihood_objective()), (pred[i][0], w_mean), (pred[i][1], w_var),
                          (osa[i][0], w_osa[0]), (osa[i][1], w_osa[1])):
            assert np.all(np.abs(np.asarray(got) - np.asarray(want)) <= 1e-10 * np.maximum(1.0, np.abs(want))), (i, got, want)
        # at beta_hat the plain likelihood of the residuals is the profile likelihood
        assert abs(lls[i] - profiles[i]) <= 1e-10 * abs(profiles[i])


@HET
def test_thetas_rows_and_restored_parameters(het):
    cases = T.panel(LENGTHS)
    S = len(cases)
    panel = _panel("m32", het, "linear")
    panel.betas = np.arange(2.0 * S).reshape(S, 2)
    rng = np.random.RandomState(3)
    thetas = np.stack([rng.uniform(0.5, 2.0, S), rng.uniform(0.3, 1.0, S), rng.uniform(0.05, 0.3, S)], axis=1)
    betas, covs, profiles = panel.mean_coefficients(thetas)
    flats = panel.log_marginal_likelihoods_flat_mean(thetas)
    import pssgp.kernels as Kn
    for i in (0, 1, 4):
        t, y, s = cases[i]
        kern = Kn.Matern32(variance=thetas[i, 0], lengthscales=thetas[i, 1])
        one = StateSpaceGPPanel([(t, y)], kern, noise_variance=thetas[i, 2], parallel=False,
                                observation_variances=[s] if het else None, mean_function=T.bases()["linear"])
        b, c, pr = one.mean_coefficients()
        assert np.array_equal(b[0], betas[i]) and np.array_equal(c[0], covs[i]) and pr[0] == profiles[i]
        assert one.log_marginal_likelihoods_flat_mean()[0] == flats[i]
    state = lambda: (float(panel.kernel.variance), float(panel.kernel.lengthscales), panel.noise_variance)
    assert state() == (1.0, 0.5, R)
    assert np.array_equal(panel.betas, np.arange(2.0 * S).reshape(S, 2))
    # ... on the error paths too: a row that is no setting of the kernel, thetas of the wrong shape
    bad = thetas.copy()
    bad[2, 1] = -1.0
    with pytest.raises(Exception):
        panel.mean_coefficients(bad)
    with pytest.raises(ValueError):
        panel.mean_grams(thetas[:-1])
    with pytest.raises(ValueError):
        panel.betas = np.zeros((S, 3))
    assert state() == (1.0, 0.5, R)
    assert np.array_equal(panel.betas, np.arange(2.0 * S).reshape(S, 2))
    # gradients run on the device: off it the single model's NotImplementedError comes through, and nothing has moved
    with pytest.raises(NotImplementedError):
        panel.profile_log_likelihood_and_grad()
    assert np.array_equal(panel.betas, np.arange(2.0 * S).reshape(S, 2)) and state() == (1.0, 0.5, R)


@HET
def test_unsorted_series_keep_the_order_given(het):
    cases = T.panel(LENGTHS)
    rng = np.random.RandomState(11)
    perms = [rng.permutation(c[0].size) for c in cases]
    sorted_panel, shuffled = _panel("m52", het, "quadratic"), _panel("m52", het, "quadratic", order=perms)
    b0, c0, p0 = sorted_panel.mean_coefficients()
    b1, c1, p1 = shuffled.mean_coefficients()
    assert np.array_equal(b0, b1) and np.array_equal(c0, c1) and np.array_equal(p0, p1)
    sorted_panel.betas = shuffled.betas = b0
    for name in ("one_step_ahead", "leave_one_out"):
        for (m0, v0, d0), (m1, v1, d1), perm in zip(getattr(sorted_panel, name)(), getattr(shuffled, name)(), perms):
            for a, b in ((m0, m1), (v0, v1), (d0, d1)):
                assert a.shape == b.shape == (perm.size, 1)
                np.testing.assert_allclose(b, a[perm], rtol=1e-12, atol=1e-12, equal_nan=True)


@HET
def test_a_rank_deficient_series_is_named(het):
    """Two observed rows at ONE time under Linear: the two basis functions are collinear on the observed rows."""
    cases = list(T.panel(LENGTHS))
    t = np.array([0.2, 0.4, 0.4, 0.7])
    y = np.array([np.nan, 0.3, -0.1, np.nan])
    s = np.full(4, 0.02)
    series = [(c[0], c[1]) for c in cases[:2]] + [(t, y)] + [(c[0], c[1]) for c in cases[3:]]
    obs = ([c[2] for c in cases[:2]] + [s] + [c[2] for c in cases[3:]]) if het else None
    panel = StateSpaceGPPanel(series, matern("m32"), noise_variance=R, parallel=False, observation_variances=obs,
                              mean_function=Linear())
    for call in (panel.mean_coefficients, panel.fit_mean_functions, panel.profile_log_likelihoods,
                 panel.log_marginal_likelihoods_flat_mean, panel.profile_log_likelihood_and_grad):
        with pytest.raises(ValueError, match="series 2"):
            call()
    assert len(panel.mean_grams()) == len(series)          # (the Gram matrices themselves exist)
    assert np.array_equal(panel.betas, np.zeros((len(series), 2)))


@HET
def test_without_a_mean_function_nothing_changes(het):
    cases = T.panel(LENGTHS)
    obs = [c[2] for c in cases] if het else None
    pairs = [(c[0], c[1]) for c in cases]
    a = StateSpaceGPPanel(pairs, matern("m32"), noise_variance=R, parallel=False, observation_variances=obs)
    b = StateSpaceGPPanel(pairs, matern("m32"), noise_variance=R, parallel=False, observation_variances=obs, mean_function=None)
    assert b.mean_function is None
    for name in ("mean_grams", "mean_coefficients", "fit_mean_functions", "profile_log_likelihoods",
                 "log_marginal_likelihoods_flat_mean", "profile_log_likelihood_and_grad"):
        with pytest.raises(ValueError, match="mean_function"):
            getattr(b, name)()
    with pytest.raises(ValueError, match="mean_function"):
        b.betas
    bits = lambda x: np.asarray(x, np.float64).view(np.uint64)
    Xnews = [np.linspace(0.0, 1.2, 5)] * len(cases)
    assert np.array_equal(bits(a.log_likelihoods()), bits(b.log_likelihoods()))
    for (m0, v0), (m1, v1) in zip(a.predict_f(Xnews), b.predict_f(Xnews)):
        assert np.array_equal(bits(m0), bits(m1)) and np.array_equal(bits(v0), bits(v1))
    for name in ("one_step_ahead", "leave_one_out"):
        for x, y in zip(getattr(a, name)(), getattr(b, name)()):
            for u, v in zip(x, y):
                assert np.array_equal(bits(u), bits(v))
    assert np.array_equal(bits(a.loo_log_predictive_densities()), bits(b.loo_log_predictive_densities()))
    with pytest.raises(TypeError):
        StateSpaceGPPanel(pairs, matern("m32"), parallel=False, mean_function=object())
