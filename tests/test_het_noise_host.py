"""Host tests of per-observation noise variances (StateSpaceGP(observation_variances=s): y_k = f(t_k) + e_k,
e_k ~ N(0, noise_variance + s_k)) on the sequential twin (pgps_seq_kf_het_*, parallel=False: no device needed).  References
(het_refs.py): dense conditioning with K + diag(R + s) for the Matern family, at kernel_zoo's tolerance against the dense GP
(1e-6); a numpy Kalman filter + RTS smoother with a per-step R for RBF order 4 and Periodic * Matern32, at the project's 1e-9
(max norm relative to the largest entry)."""
import numpy as np
import pytest

from het_refs import MATERNS, R, dense_het, matern, queries, rel, series, ss_het

N, K = 200, 50
TOL = 1e-9


@pytest.fixture(autouse=True)
def host_discretisation(monkeypatch):
    """StateSpaceGP's sequential path builds its LGSSM through _backend.discretise, which runs on the device even with
    parallel=False; these tests have no GPU, so that one call takes the model's own host discretisation (expm per step), as
    in test_multi_output_host.py."""
    from pssgp import _backend, model
    monkeypatch.setattr(_backend, "discretise", lambda F, Pinf, ts, t0=0.0, device=0: model._host_discretise(F, Pinf, ts, t0))


def _model(kernel, t, y, s, **kw):
    from pssgp.model import StateSpaceGP
    return StateSpaceGP((t[:, None], y[:, None]), kernel, noise_variance=R, observation_variances=s, **kw)


@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
def test_matern_against_the_dense_gp(kname):
    _, spec, tol = MATERNS[kname]
    t, y, s = series(N)
    tq = queries(t, K)
    assert tq[0] < t[0] and tq[-1] > t[-1] and np.intersect1d(tq, t).size >= 5
    assert 0.15 < np.mean(np.isnan(y)) < 0.25 and s.max() / s.min() > 30.0
    m = _model(matern(kname), t, y, s)
    ll = float(m.maximum_log_likelihood_objective())
    mean, var = m.predict_f(tq[:, None])
    assert mean.shape == (K, 1) and var.shape == (K, 1)
    ll_d, mean_d, var_d = dense_het(spec, t, y, R, s, tq)
    print(f"{kname}: ll {abs(ll - ll_d):.2e} mean {np.max(np.abs(mean[:, 0] - mean_d)):.2e} var {np.max(np.abs(var[:, 0] - var_d)):.2e}")
    np.testing.assert_allclose(ll, ll_d, atol=tol, rtol=tol)
    np.testing.assert_allclose(mean[:, 0], mean_d, atol=tol, rtol=tol)
    np.testing.assert_allclose(var[:, 0], var_d, atol=tol, rtol=tol)


def _other_kernel(name):
    from pssgp.kernels import Matern32, Periodic, RBF, SquaredExponential
    if name == "rbf4":
        return RBF(variance=1., lengthscales=0.5, order=4, balancing_iter=5)
    return Periodic(SquaredExponential(1., 0.5), period=0.5, order=2) * Matern32(variance=1., lengthscales=0.5)


@pytest.mark.parametrize("name", ["rbf4", "periodic*m32"])
def test_other_kernels_against_the_state_space_reference(name):
    k = _other_kernel(name)
    t, y, s = series(N)
    tq = queries(t, K)
    m = _model(k, t, y, s)
    ll = float(m.maximum_log_likelihood_objective())
    mean, var = m.predict_f(tq[:, None])
    ll_r, mean_r, var_r = ss_het(k.get_sde(), t, y, R, s, tq)
    e = (abs(ll - ll_r) / abs(ll_r), rel(mean[:, 0], mean_r), rel(var[:, 0], var_r))
    print(f"{name}: ll {e[0]:.2e} mean {e[1]:.2e} var {e[2]:.2e}")
    assert max(e) <= TOL, e


def test_the_two_references_agree():
    """The state-space reference against the dense one where both apply (Matern-3/2), at the dense tolerance."""
    from het_refs import sde_of
    t, y, s = series(N)
    tq = queries(t, K)
    a, b = ss_het(sde_of("m32"), t, y, R, s, tq), dense_het(MATERNS["m32"][1], t, y, R, s, tq)
    for u, v in zip(a, b):
        np.testing.assert_allclose(u, v, atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("kname", ["m32", "rbf4"])
def test_constant_s_is_a_larger_noise_variance(kname):
    from pssgp.model import StateSpaceGP
    k = matern(kname) if kname in MATERNS else _other_kernel(kname)
    t, y, _ = series(N)
    tq = queries(t, K)
    c = 0.037
    m = _model(k, t, y, np.full(N, c))
    plain = StateSpaceGP((t[:, None], y[:, None]), k, noise_variance=R + c)
    ll, ll_p = float(m.maximum_log_likelihood_objective()), float(plain.maximum_log_likelihood_objective())
    (mean, var), (mean_p, var_p) = m.predict_f(tq[:, None]), plain.predict_f(tq[:, None])
    assert abs(ll - ll_p) <= 1e-12 * abs(ll_p)
    assert rel(mean, mean_p) <= 1e-12 and rel(var, var_p) <= 1e-12


def test_s_at_missing_rows_is_ignored_bit_for_bit():
    t, y, s = series(N)
    tq = queries(t, K)
    s_nan = np.where(np.isnan(y), np.nan, s)
    s_big = np.where(np.isnan(y), 1e30, s)
    out = []
    for sv in (s, s_nan, s_big, s_nan[:, None]):
        m = _model(matern("m32"), t, y, sv)
        out.append((m.maximum_log_likelihood_objective(),) + tuple(m.predict_f(tq[:, None])))
    for o in out[1:]:
        for a, b in zip(out[0], o):
            assert np.array_equal(np.asarray(a), np.asarray(b))


def test_none_restores_the_scalar_model_bit_for_bit():
    from pssgp.model import StateSpaceGP
    t, y, s = series(N)
    tq = queries(t, K)
    k = matern("m52")
    plain = StateSpaceGP((t[:, None], y[:, None]), k, noise_variance=R)
    want = (plain.maximum_log_likelihood_objective(),) + tuple(plain.predict_f(tq[:, None]))
    m = _model(k, t, y, s)
    with_s = float(m.maximum_log_likelihood_objective())
    assert m.observation_variances is not None and abs(with_s - float(want[0])) > 1e-3
    m.observation_variances = None
    assert m.observation_variances is None
    got = (m.maximum_log_likelihood_objective(),) + tuple(m.predict_f(tq[:, None]))
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    m.observation_variances = s                     # ... and the vector assigned again gives the per-observation result again
    assert float(m.maximum_log_likelihood_objective()) == with_s


def test_the_host_twin_takes_a_per_step_variance():
    """sequential.kf / kfs with observation_variances against the numpy filter, and equal to the scalar call for a constant."""
    from pssgp.kalman import sequential
    from het_refs import sde_of
    from oracle import np_oracle as O
    t, y, s = series(60)
    ssm = O.get_ssm(sde_of("m32"), t, R)
    fms, fPs, ll = sequential.kf(ssm, y, return_loglikelihood=True, observation_variances=R + s)
    ll_r = ss_het(sde_of("m32"), t, y, R, s)
    assert abs(float(ll) - ll_r) <= TOL * abs(ll_r)
    const = sequential.kf(ssm, y, return_loglikelihood=True, observation_variances=np.full(60, R))
    plain = sequential.kf(ssm, y, return_loglikelihood=True)
    for a, b in zip(const, plain):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    sms, sPs = sequential.kfs(ssm, y, observation_variances=np.full(60, R))
    sms_p, sPs_p = sequential.kfs(ssm, y)
    assert np.array_equal(sms, sms_p) and np.array_equal(sPs, sPs_p)
    with pytest.raises(ValueError):
        sequential.kf(ssm, y, observation_variances=np.full(59, R))


def test_error_cases():
    from pssgp.model import StateSpaceGP
    t, y, s = series(N)
    tq = queries(t, K)
    k = matern("m32")
    with pytest.raises(ValueError, match="observation_variances"):
        _model(k, t, y, s[:-1])
    bad = s.copy()
    bad[int(np.flatnonzero(~np.isnan(y))[3])] = -1e-3
    with pytest.raises(ValueError, match="observation_variances"):
        _model(k, t, y, bad)
    bad[bad < 0] = np.inf
    with pytest.raises(ValueError, match="observation_variances"):
        _model(k, t, y, bad)
    ok = s.copy()
    ok[np.isnan(y)] = -1.0                          # (not looked at where y is missing)
    m = _model(k, t, y, ok)
    with pytest.raises(ValueError, match="observation_variances"):
        m.observation_variances = s[:-1]
    with pytest.raises(ValueError, match="observation_variances"):
        m.data = (t[:-1, None], y[:-1, None])       # the length is checked on the data setter as well
    assert m.data[0].shape[0] == N
    with pytest.raises(NotImplementedError, match="observation_variances"):
        StateSpaceGP((t[:, None], np.stack([y, y], axis=1)), k, noise_variance=R, observation_variances=s)
    two = StateSpaceGP((t[:, None], np.stack([y, y], axis=1)), k, noise_variance=R)
    with pytest.raises(NotImplementedError, match="observation_variances"):
        two.observation_variances = s
    theta = np.array([[1.0, 0.5, R]])
    raising = [lambda: m.predict_f(tq[:, None], full_cov=True), lambda: m.predict_f_samples(tq[:, None], 2, seed=1),
               lambda: m.predict_f_batch(tq[:, None], theta), lambda: m.log_likelihood_batch(theta),
               lambda: m.log_likelihood_and_grad_batch(theta)]
    for call in raising:
        with pytest.raises(NotImplementedError, match="observation_variances"):
            call()
    # gradients: the parallel=False model raises as it always did; parallel=True off the device route says why
    with pytest.raises(NotImplementedError):
        m.log_likelihood_and_grad()
    for kernel, method in ((k, "dual"), (k, "differences"), (_other_kernel("rbf4"), None), (_other_kernel("rbf4"), "adjoint")):
        mp = _model(kernel, t, y, s, parallel=True)
        with pytest.raises(NotImplementedError, match="observation_variances"):
            mp.log_likelihood_and_grad(method=method)
