"""Host tests of the predictive checks of StateSpaceGP (one_step_ahead, leave_one_out, loo_log_predictive_density; predict_y,
predict_log_density) on the host twin (parallel=False: no device needed).  References (loo_refs.py): a numpy
Kalman filter + RTS smoother followed by the cavity formula, at the project's 1e-9 (max norm relative to the largest entry);
the dense leave-one-out formula with K_y^-1 for the Matern family, at kernel_zoo's tolerance against the dense GP (1e-6);
brute force (a row set to NaN, the existing predict_f asked there)."""
import numpy as np
import pytest

from loo_refs import FIELDS, MATERNS, R, TOL, case, dense_checks, err, gaps, log_density, matern, refs, rel, ss_checks

SIZES = (1, 2, 37, 300, 700)


@pytest.fixture(autouse=True)
def host_discretisation(monkeypatch):
    """predict_f's sequential path builds its LGSSM through _backend.discretise, which runs on the device even with
    parallel=False; these tests have no GPU, so that one call takes the model's own host discretisation, as in
    test_het_noise_host.py.  (The predictive checks themselves discretise on the host.)"""
    from pssgp import _backend, model
    monkeypatch.setattr(_backend, "discretise", lambda F, Pinf, ts, t0=0.0, device=0: model._host_discretise(F, Pinf, ts, t0))


def _model(kernel, t, y, noise=R, **kw):
    from pssgp.model import StateSpaceGP
    return StateSpaceGP((t[:, None], y[:, None]), kernel, noise_variance=noise, **kw)


def _all(m):
    """The dict layout of the references from the model's public methods."""
    (om, ov, ol), (lm, lv, ld) = m.one_step_ahead(), m.leave_one_out()
    out = {"osa_mean": om[:, 0], "osa_var": ov[:, 0], "osa_log_density": ol[:, 0], "loo_mean": lm[:, 0], "loo_var": lv[:, 0],
           "loo_log_density": ld[:, 0]}
    out["ll"] = float(np.nansum(ol))
    out["loo_lpd"] = float(m.loo_log_predictive_density())
    return out


def _other_kernel(name):
    from pssgp.kernels import Matern32, Periodic, RBF, SquaredExponential
    if name == "rbf4":
        return RBF(variance=1., lengthscales=0.5, order=4, balancing_iter=5)
    return Periodic(SquaredExponential(1., 0.5), period=0.5, order=2) * Matern32(variance=1., lengthscales=0.5)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
def test_matern_against_both_references(kname, n):
    t, y, _ = case(n)
    got = _all(_model(matern(kname), t, y))
    e_ss, e_dn = gaps(got, kname, n)
    print(f"{kname} N {n}: state-space {e_ss:.2e} dense {e_dn:.2e} (R - v) / R >= {refs(kname, n)[0]['gap']:.3f}")
    assert e_ss <= TOL and e_dn <= MATERNS[kname][2]
    assert abs(got["loo_lpd"] - np.nansum(got["loo_log_density"])) <= 1e-12 * abs(got["loo_lpd"])


@pytest.mark.parametrize("name", ["rbf4", "periodic*m32"])
def test_other_kernels_against_the_state_space_reference(name):
    k = _other_kernel(name)
    t, y, _ = case(200)
    got = _all(_model(k, t, y))
    ref = ss_checks(k.get_sde(), t, y, R)
    e = [err(got[f], ref[f]) for f in FIELDS] + [abs(got[s] - ref[s]) / abs(ref[s]) for s in ("ll", "loo_lpd")]
    print(f"{name}: " + " ".join(f"{x:.2e}" for x in e))
    assert max(e) <= TOL, e


@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
def test_the_two_references_agree_on_repeated_times(kname):
    """The case the GPU tests use with five dt = 0 steps: numpy filter + smoother against the dense formula, within 1e-9."""
    ss, dn = refs(kname, 300, None, True)
    obs = ~np.isnan(case(300, None, True)[1])
    e = [rel(ss[f][obs], dn[f]) for f in FIELDS] + [abs(ss[s] - dn[s]) / abs(dn[s]) for s in ("ll", "loo_lpd")]
    print(f"{kname}: " + " ".join(f"{x:.2e}" for x in e))
    assert max(e) <= TOL, e


@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
def test_brute_force_at_every_observed_row(kname):
    """Delete the row, then predict there with the existing predict_f (+ the noise): N = 37, every observed row."""
    t, y, _ = case(37)
    mean, var, _ = _model(matern(kname), t, y).leave_one_out()
    worst = 0.0
    for i in np.flatnonzero(~np.isnan(y)):
        yi = np.array(y)
        yi[i] = np.nan
        mf, vf = _model(matern(kname), t, yi).predict_f(t[i:i + 1, None])
        worst = max(worst, abs(mean[i, 0] - mf[0, 0]), abs(var[i, 0] - (vf[0, 0] + R)))
    print(f"{kname}: brute force {worst:.2e}")
    assert worst <= TOL * max(1.0, float(np.max(np.abs(mean))))


@pytest.mark.parametrize("name", ["m32", "rbf4"])
def test_one_step_ahead_sums_to_the_objective(name):
    k = matern(name) if name in MATERNS else _other_kernel(name)
    t, y, _ = case(300)
    m = _model(k, t, y)
    ll = float(m.maximum_log_likelihood_objective())
    total = float(np.nansum(m.one_step_ahead()[2]))
    assert abs(total - ll) <= 1e-12 * abs(ll), (total, ll)


@pytest.mark.parametrize("name", ["m52", "rbf4"])
def test_observation_variances(name):
    k = matern(name) if name in MATERNS else _other_kernel(name)
    t, y, s = case(200)
    got = _all(_model(k, t, y, observation_variances=s))
    ref = ss_checks(k.get_sde(), t, y, R + s)
    e = [err(got[f], ref[f]) for f in FIELDS] + [abs(got[x] - ref[x]) / abs(ref[x]) for x in ("ll", "loo_lpd")]
    print(f"{name} with s: " + " ".join(f"{x:.2e}" for x in e))
    assert max(e) <= TOL, e
    if name in MATERNS:
        dn = dense_checks(MATERNS[name][1], t, y, R + s)
        obs = ~np.isnan(y)
        assert max(rel(got[f][obs], dn[f]) for f in FIELDS) <= MATERNS[name][2]
    # a constant s = c is the scalar model at R + c
    c = 0.037
    const, plain = _all(_model(k, t, y, observation_variances=np.full(t.size, c))), _all(_model(k, t, y, noise=R + c))
    for f in FIELDS + ("ll", "loo_lpd"):
        assert err(const[f], plain[f]) <= 1e-12, f


def test_nan_rows_shapes_and_dtype():
    from pssgp import config
    t, y, _ = case(300)
    nan = np.isnan(y)
    assert 0.15 < nan.mean() < 0.25
    m = _model(matern("m32"), t, y)
    for out in (m.one_step_ahead(), m.leave_one_out()):
        assert len(out) == 3
        for a in out:
            assert a.shape == (300, 1) and a.dtype == config.default_float()
        mean, var, logd = out
        assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var)) and np.all(var > R * (1 - 1e-12))
        assert np.array_equal(np.isnan(logd[:, 0]), nan)
        assert np.array_equal(logd[~nan, 0], log_density(y[~nan], mean[~nan, 0], var[~nan, 0]))
    lpd = m.loo_log_predictive_density()
    assert np.ndim(lpd) == 0 and np.isfinite(lpd)
    assert abs(float(lpd) - float(np.sum(m.leave_one_out()[2][~nan]))) <= 1e-12 * abs(float(lpd))
    # at a NaN row nothing is left out: the law of an observation there given all data
    i = int(np.flatnonzero(nan)[3])
    mf, vf = m.predict_f(t[i:i + 1, None])
    mean, var, _ = m.leave_one_out()
    assert abs(mean[i, 0] - mf[0, 0]) <= TOL and abs(var[i, 0] - (vf[0, 0] + R)) <= TOL


def test_rows_out_of_order_come_back_in_the_order_of_the_data():
    t, y, _ = case(37)
    want = _all(_model(matern("m32"), t, y))
    perm = np.random.RandomState(5).permutation(37)
    got = _all(_model(matern("m32"), t[perm], y[perm]))
    for f in FIELDS:
        assert err(got[f], want[f][perm]) <= 1e-12, f
    assert abs(got["loo_lpd"] - want["loo_lpd"]) <= 1e-12 * abs(want["loo_lpd"])


def test_float32_models_are_computed_in_fp64_and_rounded():
    from pssgp import config
    t, y, _ = case(200)
    want = _all(_model(matern("m32"), t, y))
    old = config.default_float()
    config.set_default_float(np.float32)
    try:
        m = _model(matern("m32"), t, y)
        mean, var, logd = m.leave_one_out()
        assert mean.dtype == var.dtype == logd.dtype == np.float32
        assert np.asarray(m.loo_log_predictive_density()).dtype == np.float32
    finally:
        config.set_default_float(old)
    # inputs rounded to float32, arithmetic in fp64: far inside float32's resolution of the fp64 result's neighbourhood
    assert rel(mean[:, 0], want["loo_mean"]) <= 1e-4 and rel(var[:, 0], want["loo_var"]) <= 1e-4


def test_errors():
    t, y, s = case(37)
    k = matern("m32")
    for noise in (0.0, -0.1):
        m = _model(k, t, y, noise=noise)
        for call in (m.one_step_ahead, m.leave_one_out, m.loo_log_predictive_density):
            with pytest.raises(ValueError, match="noise_variance"):
                call()
    zero = np.array(s)
    zero[int(np.flatnonzero(~np.isnan(y))[2])] = 0.0
    with pytest.raises(ValueError, match="noise_variance"):
        _model(k, t, y, noise=0.0, observation_variances=zero).leave_one_out()
    assert np.all(np.isfinite(_model(k, t, y, noise=0.0, observation_variances=s).leave_one_out()[0]))    # R = 0, every s_k > 0
    from pssgp.model import StateSpaceGP
    two = StateSpaceGP((t[:, None], np.stack([y, y], axis=1)), k, noise_variance=R)
    calls = [two.one_step_ahead, two.leave_one_out, two.loo_log_predictive_density, lambda: two.predict_y(t[:3, None]),
             lambda: two.predict_log_density((t[:3, None], np.zeros((3, 2))))]
    for call in calls:
        with pytest.raises(NotImplementedError, match="single-output"):
            call()


def test_predict_y_and_predict_log_density():
    t, y, s = case(200)
    m = _model(matern("m52"), t, y)
    xq = np.linspace(t[0] - 0.1, t[-1] + 0.1, 23)[:, None]
    yq = np.sin(np.pi * xq)
    yq[4, 0] = np.nan
    mf, vf = m.predict_f(xq)
    my, vy = m.predict_y(xq)
    assert np.array_equal(my, mf) and np.array_equal(vy, vf + R) and vy.shape == (23, 1)
    logd = m.predict_log_density((xq, yq))
    assert logd.shape == (23, 1) and np.isnan(logd[4, 0]) and np.all(np.isfinite(np.delete(logd[:, 0], 4)))
    assert rel(np.delete(logd, 4), np.delete(log_density(yq, mf, vf + R), 4)) <= 1e-12
    with pytest.raises(NotImplementedError, match="full_cov"):
        m.predict_y(xq, full_cov=True)
    het = _model(matern("m52"), t, y, observation_variances=s)
    with pytest.raises(NotImplementedError, match="observation_variances"):
        het.predict_y(xq)
    with pytest.raises(NotImplementedError, match="observation_variances"):
        het.predict_log_density((xq, yq))
