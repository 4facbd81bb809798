"""Host tests of mean functions (pssgp/mean_functions.py, StateSpaceGP(..., mean_function=...)) on the host
twin (parallel=False: no device needed).  References: dense algebra with K_y = K + R I on the observed rows (Rasmussen & Williams
eq. 2.41, 2.42, 2.45) and the zero-mean model itself on y - Phi beta.

The dense cases: N = 300 irregular times, Matern-3/2 with lengthscale 0.5, R = 0.1, 20 rows of y NaN, Polynomial(2) and a Basis
with p = 5."""
import numpy as np
import pytest

N, R, ELL = 300, 0.1, 0.5


@pytest.fixture(autouse=True)
def host_discretisation(monkeypatch):
    """The sequential paths of the zero-mean model build their LGSSM through _backend.discretise, which runs on the device even
    with parallel=False; these tests have no GPU, so that one call takes the model's own host discretisation, as in
    test_loo_host.py.  (The whitening host twin discretises on the host.)"""
    from pssgp import _backend, model
    monkeypatch.setattr(_backend, "discretise", lambda F, Pinf, ts, t0=0.0, device=0: model._host_discretise(F, Pinf, ts, t0))


def _series():
    rng = np.random.default_rng(11)
    t = np.cumsum(rng.uniform(0.01, 0.09, N))                     # irregular, t[-1] ~ 15
    y = 2.0 + 0.4 * t - 0.03 * t ** 2 + np.sin(2.0 * t) + 0.3 * rng.standard_normal(N)
    y[rng.choice(N, 20, replace=False)] = np.nan
    return t, y


T, Y = _series()
OBS = ~np.isnan(Y)
CENTER, SCALE = 0.5 * (T[0] + T[-1]), 0.5 * (T[-1] - T[0])


def _basis5(t):
    u = (t - CENTER) / SCALE
    return np.stack([np.ones_like(u), u, np.sin(2.0 * u), np.cos(2.0 * u), np.sin(5.0 * u)], axis=1)


def _mean_functions():
    from pssgp.mean_functions import Basis, Polynomial
    return {"poly2": Polynomial(2, center=CENTER, scale=SCALE), "basis5": Basis(_basis5, 5)}


def _kernel():
    from pssgp.kernels import Matern32
    return Matern32(variance=1.0, lengthscales=ELL)


def _model(mf=None, t=T, y=Y, **kw):
    from pssgp.model import StateSpaceGP
    return StateSpaceGP((t[:, None], y[:, None]), kw.pop("kernel", None) or _kernel(), noise_variance=R, mean_function=mf, **kw)


def _k32(a, b):
    r = np.sqrt(3.0) * np.abs(a[:, None] - b[None, :]) / ELL
    return (1.0 + r) * np.exp(-r)


def _dense(Phi_obs):
    """K_y^-1 on the observed rows, and the dense A, b, g_yy, logdet."""
    Ky = _k32(T[OBS], T[OBS]) + R * np.eye(int(OBS.sum()))
    Kinv = np.linalg.inv(Ky)
    y = Y[OBS]
    return Kinv, Phi_obs.T @ Kinv @ Phi_obs, Phi_obs.T @ Kinv @ y, float(y @ Kinv @ y), float(np.linalg.slogdet(Ky)[1])


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


def test_design_matrices():
    from pssgp.mean_functions import Basis, Constant, Linear, Polynomial
    t = np.array([0.0, 1.0, 3.0])
    assert np.array_equal(Constant().design(t), [[1.0], [1.0], [1.0]])
    assert np.array_equal(Linear().design(t), [[1.0, 0.0], [1.0, 1.0], [1.0, 3.0]])
    assert np.array_equal(Polynomial(3, center=1.0, scale=2.0).design(t),
                          [[1.0, -0.5, 0.25, -0.125], [1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]])
    b = Basis(lambda u: np.stack([u, u * u], axis=1), 2)
    assert np.array_equal(b.design(t[:, None]), [[0.0, 0.0], [1.0, 1.0], [3.0, 9.0]])
    for mf, p in ((Constant(), 1), (Linear(), 2), (Polynomial(3), 4), (b, 2)):
        assert mf.design(t).dtype == np.float64 and mf.beta.dtype == np.float64
        assert np.array_equal(mf.beta, np.zeros(p)) and np.array_equal(mf(t), np.zeros(3))
    lin = Linear()
    lin.beta = [2, -1]
    assert np.array_equal(lin(t), [2.0, 1.0, -1.0])
    with pytest.raises(ValueError):
        lin.beta = [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        Basis(lambda u: u[:, None], 2).design(t)


@pytest.mark.parametrize("name", ["poly2", "basis5"])
def test_whiten_against_dense(name):
    mf = _mean_functions()[name]
    m = _model()                                                    # whiten works without a mean function
    V = np.concatenate([Y[:, None], mf.design(T)], axis=1)
    W = m.whiten(V)
    assert W.shape == V.shape and W.dtype == np.float64
    assert np.all(W[~OBS] == 0.0) and np.all(np.isfinite(W))
    Vo = V[OBS]
    Kinv = _dense(Vo[:, 1:])[0]
    G_ref = Vo.T @ Kinv @ Vo
    G = W.T @ W
    scale = np.sqrt(np.outer(np.diag(G_ref), np.diag(G_ref)))
    e = float(np.max(np.abs(G - G_ref) / scale))
    print(f"{name}: W^T W against dense {e:.2e}")
    assert e <= 1e-9
    assert np.array_equal(m.whiten(Y), W[:, :1])                  # a vector is one column
    g = _model(mf).mean_gram()
    assert g.n_obs == int(OBS.sum())
    ll = -0.5 * (g.n_obs * np.log(2.0 * np.pi) + g.logdet + float(W[:, 0] @ W[:, 0]))
    ll_model = float(m.maximum_log_likelihood_objective())
    assert abs(ll - ll_model) <= 1e-10 * abs(ll_model)
    e = float(np.max(np.abs(g.G - G_ref) / scale))
    assert e <= 1e-9
    assert np.array_equal(g.G, g.G.T) and g.g_yy == g.G[0, 0] and np.array_equal(g.b, g.G[1:, 0]) and np.array_equal(g.A, g.G[1:, 1:])


@pytest.mark.parametrize("name", ["poly2", "basis5"])
def test_gls_against_dense(name):
    """mean_coefficients, log_marginal_likelihood_flat_mean and predict_f_gls against R&W eq. 2.41, 2.42, 2.45 in dense algebra,
    1e-8 relative; cond(A) < 1e6 by the centring and scaling of the basis."""
    mf = _mean_functions()[name]
    m = _model(mf)
    Phi = mf.design(T)[OBS]
    p = Phi.shape[1]
    Kinv, A, b, g_yy, logdet = _dense(Phi)
    assert np.linalg.cond(A) < 1e6
    beta_ref = np.linalg.solve(A, b)
    cov_ref = np.linalg.inv(A)
    n = int(OBS.sum())
    profile_ref = -0.5 * (n * np.log(2.0 * np.pi) + logdet + g_yy - b @ beta_ref)
    flat_ref = profile_ref - 0.5 * np.linalg.slogdet(A)[1] + 0.5 * p * np.log(2.0 * np.pi)
    beta, cov, profile = m.mean_coefficients()
    print(f"{name}: cond(A) {np.linalg.cond(A):.1e} beta {_rel(beta, beta_ref):.2e} cov {_rel(cov, cov_ref):.2e}")
    assert _rel(beta, beta_ref) <= 1e-8 and _rel(cov, cov_ref) <= 1e-8
    assert abs(profile - profile_ref) <= 1e-8 * abs(profile_ref)
    assert abs(m.log_marginal_likelihood_flat_mean() - flat_ref) <= 1e-8 * abs(flat_ref)
    # neither depends on beta; fit_mean_function assigns the estimate, and the objective there is the profile likelihood
    mf.beta = np.arange(1.0, p + 1.0)
    assert abs(m.log_marginal_likelihood_flat_mean() - flat_ref) <= 1e-8 * abs(flat_ref)
    tq = np.sort(np.concatenate([np.linspace(T[0] - 1.0, T[-1] + 1.0, 37), T[OBS][[3, 100]]]))
    Ks = _k32(tq, T[OBS])
    Rq = mf.design(tq) - Ks @ Kinv @ Phi
    mean_ref = Ks @ Kinv @ Y[OBS] + Rq @ beta_ref
    var_ref = 1.0 - np.einsum("ij,jk,ik->i", Ks, Kinv, Ks) + np.einsum("ij,jk,ik->i", Rq, cov_ref, Rq)
    mean, var = m.predict_f_gls(tq[:, None])
    assert mean.shape == var.shape == (tq.shape[0], 1)
    assert _rel(mean[:, 0], mean_ref) <= 1e-8 and _rel(var[:, 0], var_ref) <= 1e-8
    got = m.fit_mean_function()
    assert np.array_equal(got, mf.beta) and _rel(mf.beta, beta_ref) <= 1e-8
    ll = float(m.maximum_log_likelihood_objective())
    assert abs(ll - profile_ref) <= 1e-8 * abs(profile_ref)


def test_gpflow_semantics_bit_for_bit():
    """Every delegated evaluation at a non-zero beta is the zero-mean model on y - Phi beta with m added (to means and draws, and
    taken from the y side of densities): the same arithmetic, so equal bits."""
    mf = _mean_functions()["poly2"]
    mf.beta = np.array([1.5, -0.7, 0.3])
    m = _model(mf)
    z = _model(None, y=Y - mf(T))
    tq = np.sort(np.concatenate([np.linspace(T[0] - 0.5, T[-1] + 0.5, 23), T[[5, 50]]]))[:, None]
    mq, mt = mf(tq)[:, None], mf(T)[:, None]
    eq = lambda a, b: np.array_equal(a, b, equal_nan=True)
    assert m.maximum_log_likelihood_objective() == z.maximum_log_likelihood_objective()
    for full_cov in (False, True):
        (a, av), (b, bv) = m.predict_f(tq, full_cov=full_cov), z.predict_f(tq, full_cov=full_cov)
        assert eq(a, b + mq) and eq(av, bv) and np.any(a != b)
    assert eq(m.predict_f_samples(tq, 3, seed=5), z.predict_f_samples(tq, 3, seed=5) + mq)
    assert eq(m.predict_f_samples(tq, seed=5), z.predict_f_samples(tq, seed=5) + mq)
    for name in ("one_step_ahead", "leave_one_out"):
        (a, av, al), (b, bv, bl) = getattr(m, name)(), getattr(z, name)()
        assert eq(a, b + mt) and eq(av, bv) and eq(al, bl)
    assert m.loo_log_predictive_density() == z.loo_log_predictive_density()
    (a, av), (b, bv) = m.predict_y(tq), z.predict_y(tq)
    assert eq(a, b + mq) and eq(av, bv)
    ynew = np.cos(tq)
    assert eq(m.predict_log_density((tq, ynew)), z.predict_log_density((tq, ynew - mq)))
    # the residual model follows beta, noise_variance and the data
    mf.beta = np.zeros(3)
    assert m.maximum_log_likelihood_objective() == _model().maximum_log_likelihood_objective()
    m.noise_variance = 0.2
    z0 = _model()
    z0.noise_variance = 0.2
    assert m.maximum_log_likelihood_objective() == z0.maximum_log_likelihood_objective()
    m.data = (T[:100, None], Y[:100, None])
    z0.data = (T[:100, None], Y[:100, None])
    assert m.maximum_log_likelihood_objective() == z0.maximum_log_likelihood_objective()


def test_beta_gradient_against_central_differences_and_wrt():
    """d ll / d beta = b - A beta against central differences of the objective, exactly quadratic in beta: 1e-7 relative at step
    1e-3.  With only beta entries in `wrt` a parallel=False model answers (the kernel's gradient needs the device)."""
    mf = _mean_functions()["basis5"]
    beta0 = np.array([0.5, -1.0, 0.25, 2.0, -0.1])
    mf.beta = beta0
    m = _model(mf)
    params = m.trainable_parameters()
    n0 = len(_model().trainable_parameters())
    assert len(params) == n0 + 5 and params[n0 - 1] == (m, "noise_variance")
    assert [q[1:] for q in params[n0:]] == [("beta", j) for j in range(5)] and all(q[0] is mf for q in params[n0:])
    idx = list(range(n0, n0 + 5))
    ll, g = m.log_likelihood_and_grad(wrt=idx)
    assert g.shape == (n0 + 5,) and np.all(g[:n0] == 0.0)
    assert ll == m.maximum_log_likelihood_objective()
    fd = np.zeros(5)
    for j in range(5):
        for sgn in (1.0, -1.0):
            bj = beta0.copy()
            bj[j] += sgn * 1e-3
            mf.beta = bj
            fd[j] += sgn * float(m.maximum_log_likelihood_objective()) / 2e-3
    mf.beta = beta0
    print("d ll / d beta:", g[n0:], "central differences:", fd)
    assert _rel(g[n0:], fd) <= 1e-7
    _, g2 = m.log_likelihood_and_grad(wrt=[n0 + 1, n0 + 4])
    assert np.array_equal(g2[[n0 + 1, n0 + 4]], g[[n0 + 1, n0 + 4]]) and np.count_nonzero(g2) == 2
    with pytest.raises(IndexError):
        m.log_likelihood_and_grad(wrt=[n0 + 5])
    with pytest.raises(NotImplementedError):
        m.log_likelihood_and_grad()                                  # the kernel's entries: parallel=True only, as without a mean


def test_refusals():
    from pssgp.mean_functions import Basis, Constant, Linear
    from pssgp.model import StateSpaceGP
    k = _kernel()
    with pytest.raises(NotImplementedError):
        StateSpaceGP((T[:, None], np.stack([Y, Y], axis=1)), k, noise_variance=R, mean_function=Constant())
    with pytest.raises(NotImplementedError):
        StateSpaceGP((T[:, None], Y[:, None]), k, noise_variance=R, observation_variances=np.full(N, 0.1), mean_function=Constant())
    m = _model(Linear())
    with pytest.raises(NotImplementedError):
        m.observation_variances = np.full(N, 0.1)
    thetas = np.array([[1.0, 0.5, 0.1]])
    for call in (lambda: m.log_likelihood_batch(thetas), lambda: m.log_likelihood_and_grad_batch(thetas),
                 lambda: m.predict_f_batch(T[:5, None], thetas)):
        with pytest.raises(NotImplementedError):
            call()
    # rank-deficient designs: a repeated basis function, and one that vanishes on the observed rows
    twice = _model(Basis(lambda t: np.stack([np.ones_like(t), t, 2.0 * t - 3.0], axis=1), 3))
    with pytest.raises(ValueError, match="full column rank"):
        twice.mean_coefficients()
    with pytest.raises(ValueError, match="full column rank"):
        twice.predict_f_gls(T[:5, None])
    hidden = _model(Basis(lambda t: np.stack([np.ones_like(t), (t == T[~OBS][0]).astype(float)], axis=1), 2))
    with pytest.raises(ValueError, match="full column rank"):
        hidden.log_marginal_likelihood_flat_mean()
    with pytest.raises(ValueError):
        _model().mean_gram()                                         # no mean function
    with pytest.raises(ValueError):
        _model().whiten(np.zeros(N + 1))


def test_without_a_mean_function_nothing_changes():
    """mean_function=None is the model as it was: the objective and predict_f equal the residual-free route's values (the model
    built without the argument), and trainable_parameters() is unchanged."""
    from pssgp.model import StateSpaceGP
    k = _kernel()
    a = StateSpaceGP((T[:, None], Y[:, None]), k, noise_variance=R)
    b = StateSpaceGP((T[:, None], Y[:, None]), k, noise_variance=R, mean_function=None)
    assert a.mean_function is None and b.mean_function is None
    tq = np.linspace(T[0], T[-1], 17)[:, None]
    assert a.maximum_log_likelihood_objective() == b.maximum_log_likelihood_objective()
    for x, y in zip(a.predict_f(tq), b.predict_f(tq)):
        assert np.array_equal(x, y)
    pa, pb = a.trainable_parameters(), b.trainable_parameters()
    assert [(q[0] is k or q[0] is a, q[1]) for q in pa] == [(q[0] is k or q[0] is b, q[1]) for q in pb]
    assert all(len(q) == 2 for q in pb) and pb[-1] == (b, "noise_variance")
    # the zero-mean objective is also what the whitened y gives: the dense value
    Kinv, _, _, g_yy, logdet = _dense(np.ones((int(OBS.sum()), 1)))
    ref = -0.5 * (int(OBS.sum()) * np.log(2.0 * np.pi) + logdet + g_yy)
    assert abs(float(a.maximum_log_likelihood_objective()) - ref) <= 1e-9 * abs(ref)


def test_host_twin_takes_unsorted_times():
    """Times out of order are sorted for the host twin and the rows put back."""
    mf = _mean_functions()["poly2"]
    g = _model(mf).mean_gram()
    perm = np.random.default_rng(3).permutation(N)
    mfp = _mean_functions()["poly2"]
    gp = _model(mfp, t=T[perm], y=Y[perm]).mean_gram()
    assert _rel(gp.G, g.G) <= 1e-12 and abs(gp.logdet - g.logdet) <= 1e-12 * abs(g.logdet)
    W = _model(t=T[perm], y=Y[perm]).whiten(Y[perm])
    assert np.all(W[~OBS[perm]] == 0.0) and _rel(W[:, 0], _model().whiten(Y)[perm, 0]) <= 1e-12
