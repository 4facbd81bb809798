"""predict_f_batch on the host (parallel=False): the posterior at B hyper-parameter settings as a loop over the sequential
path -- the twin the device path (tests/test_gpu_predict_batch.py) is judged against -- and the mixture of the B
posteriors.  No GPU.

predict_f itself discretises on the device even with parallel=False, so the host twin is a function of its own
(StateSpaceGP._predict_f_host).  The exact comparison against the loop over that function pins the assignment and
restoration of the parameters only; the arithmetic is pinned by the numpy oracle's sequential predict_f (1e-9) and by the
dense GP (1e-8) below."""
import numpy as np
import pytest

from oracle import np_oracle as O


def _data(n, k, seed):
    """tests/test_gpu_predict.py's recipe: sorted uniform times, a sine plus noise, some queries beyond the last observation."""
    rng = np.random.RandomState(seed)
    t = np.sort(rng.rand(n)) * (n / 80.0)
    y = np.sin(3.0 * t) + 0.3 * rng.randn(n)
    tq = np.sort(rng.rand(k)) * (n / 80.0) * 1.1
    return t, y, tq


def _thetas(B, P, seed=2):
    """tests/test_gpu_batch.py's recipe: every parameter exp(U(-1, 1))."""
    return np.exp(np.random.RandomState(seed).uniform(-1.0, 1.0, (B, P)))


def _kernel(name, kernel_zoo):
    return {k[0]: k[1] for k in kernel_zoo}[name]()


def _loop(m, tq, thetas):
    """The loop over the settings: assign row b, the model's host predict (merge, host discretisation, sequential filter +
    smoother, projection -- predict_f itself discretises on the device even with parallel=False); parameters put back."""
    params = m.trainable_parameters()
    saved = [getattr(o, n) for o, n in params]
    means, variances, lls = [], [], []
    for row in thetas:
        for (o, n), v in zip(params, row):
            setattr(o, n, float(v))
        mean, var, ll = m._predict_f_host(tq)
        means.append(mean[:, None])
        variances.append(var[:, None])
        lls.append(ll)
    for (o, n), v in zip(params, saved):
        setattr(o, n, v)
    return np.stack(means), np.stack(variances), np.array(lls)


@pytest.mark.parametrize("kname", ["matern32", "rbf6", "m32*m52"])
def test_host_batch_is_the_loop_exactly(kname, kernel_zoo):
    from pssgp.model import StateSpaceGP
    t, y, tq = _data(120, 40, 5)
    m = StateSpaceGP((t[:, None], y[:, None]), _kernel(kname, kernel_zoo), noise_variance=0.2, parallel=False)
    params = m.trainable_parameters()
    before = [getattr(o, n) for o, n in params]
    base = np.array(before, np.float64)
    thetas = base[None, :] * np.exp(np.random.RandomState(3).uniform(-0.3, 0.3, (4, len(params))))
    means, variances, lls = m.predict_f_batch(tq[:, None], thetas, return_log_likelihood=True)
    assert means.shape == (4, 40, 1) and variances.shape == (4, 40, 1) and lls.shape == (4,)
    want_m, want_v, want_ll = _loop(m, tq, thetas)
    assert np.array_equal(means, want_m) and np.array_equal(variances, want_v) and np.array_equal(lls, want_ll)
    assert [getattr(o, n) for o, n in params] == before
    # ... and that loop is the oracle's sequential predict_f, setting by setting
    for b, row in enumerate(thetas):
        for (o, n), v in zip(params, row):
            setattr(o, n, float(v))
        sde = m.kernel.get_sde()
        mean_o, var_o = O.ssgp_predict_f(sde, t, y, float(row[-1]), tq, parallel=False)
        ll_o = O.ssgp_log_likelihood(sde, t, y, float(row[-1]), parallel=False)
        assert np.max(np.abs(means[b, :, 0] - mean_o)) < 1e-9 and np.max(np.abs(variances[b, :, 0] - var_o)) < 1e-9
        assert abs(lls[b] - ll_o) < 1e-9 * abs(ll_o)
    for (o, n), v in zip(params, before):
        setattr(o, n, v)
    two = m.predict_f_batch(tq[:, None], thetas)
    assert len(two) == 2 and np.array_equal(two[0], means) and np.array_equal(two[1], variances)


def test_parameters_restored_when_a_row_raises():
    from pssgp.kernels import Matern32
    from pssgp.model import StateSpaceGP

    class Failing(Matern32):
        calls = 0

        def get_sde(self):
            if float(self.lengthscales) == 0.77:
                raise RuntimeError("second row")
            return super().get_sde()

    t, y, tq = _data(60, 10, 1)
    m = StateSpaceGP((t[:, None], y[:, None]), Failing(1.3, 0.6), noise_variance=0.15, parallel=False)
    thetas = np.array([[1.0, 0.5, 0.1], [1.1, 0.77, 0.2], [1.2, 0.9, 0.3]])
    with pytest.raises(RuntimeError, match="second row"):
        m.predict_f_batch(tq[:, None], thetas)
    assert m.kernel.variance == 1.3 and m.kernel.lengthscales == 0.6 and m.noise_variance == 0.15


def test_shapes_and_query_order():
    from pssgp.kernels import Matern32
    from pssgp.model import StateSpaceGP
    t, y, tq = _data(80, 12, 2)
    m = StateSpaceGP((t[:, None], y[:, None]), Matern32(1.0, 0.5), noise_variance=0.1, parallel=False)
    thetas = _thetas(3, 3)
    mean, var = m.predict_f_batch(tq[:, None], thetas[:1])                      # B = 1
    assert mean.shape == (1, 12, 1) and var.shape == (1, 12, 1)
    mean, var = m.predict_f_batch(tq[:, None], thetas[0])                       # one setting as a vector
    assert mean.shape == (1, 12, 1)
    mean, var, lls = m.predict_f_batch(tq[:1, None], thetas, return_log_likelihood=True)     # K = 1
    assert mean.shape == (3, 1, 1) and var.shape == (3, 1, 1) and lls.shape == (3,)
    mean0, var0, lls0 = m.predict_f_batch(np.zeros((0, 1)), thetas, return_log_likelihood=True)     # K = 0
    assert mean0.shape == (3, 0, 1) and var0.shape == (3, 0, 1) and np.array_equal(lls0, lls)
    mix0 = m.predict_f_batch(np.zeros((0, 1)), thetas, reduce="mixture")
    assert mix0[0].shape == (0, 1) and mix0[1].shape == (0, 1)
    # any order, repeats: the rows of the sorted unique call
    pick = np.random.RandomState(0).randint(0, 12, 30)
    uniq, inverse = np.unique(tq[pick], return_inverse=True)
    sorted_mean, sorted_var = m.predict_f_batch(uniq[:, None], thetas)
    mean, var = m.predict_f_batch(tq[pick][:, None], thetas)
    assert mean.shape == (3, 30, 1)
    assert np.array_equal(mean, sorted_mean[:, inverse]) and np.array_equal(var, sorted_var[:, inverse])
    mm, mv = m.predict_f_batch(tq[pick][:, None], thetas, reduce="mixture")
    sm, sv = m.predict_f_batch(uniq[:, None], thetas, reduce="mixture")
    assert np.array_equal(mm, sm[inverse]) and np.array_equal(mv, sv[inverse])


def test_bad_arguments_raise():
    from pssgp.kernels import Matern32
    from pssgp.model import StateSpaceGP
    t, y, tq = _data(40, 6, 3)
    m = StateSpaceGP((t[:, None], y[:, None]), Matern32(1.0, 0.5), noise_variance=0.1, parallel=False)
    thetas = _thetas(3, 3)
    with pytest.raises(ValueError):
        m.predict_f_batch(tq[:, None], thetas[:, :2])                           # wrong column count
    with pytest.raises(ValueError):
        m.predict_f_batch(tq[:, None], np.ones((3, 4)))
    for bad in ([1.0, -1.0, 1.0], [0.0, 0.0, 0.0], [1.0, 1.0], [1.0, np.nan, 1.0]):
        with pytest.raises(ValueError):
            m.predict_f_batch(tq[:, None], thetas, reduce="mixture", weights=bad)
    with pytest.raises(ValueError):
        m.predict_f_batch(tq[:, None], thetas, reduce="mean")
    assert m.kernel.variance == 1.0 and m.kernel.lengthscales == 0.5 and m.noise_variance == 0.1


@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
def test_host_batch_equals_dense_gp(kname):
    """Nine settings against the dense GP at the project's bound for this comparison (the sequential oracle itself stays
    within 4.5e-15 of O.dense_gp on these inputs)."""
    from pssgp.kernels import Matern12, Matern32, Matern52
    from pssgp.model import StateSpaceGP
    cls, spec = {"m12": (Matern12, "matern12"), "m32": (Matern32, "matern32"), "m52": (Matern52, "matern52")}[kname]
    t, y, tq = _data(200, 50, 7 * 200 + 50)
    thetas = _thetas(9, 3)
    m = StateSpaceGP((t[:, None], y[:, None]), cls(1.0, 1.0), noise_variance=0.1, parallel=False)
    means, variances, lls = m.predict_f_batch(tq[:, None], thetas, return_log_likelihood=True)
    for b, th in enumerate(thetas):
        ll_gp, mean_gp, var_gp = O.dense_gp((spec, th[0], th[1]), t, y, th[2], tq)
        np.testing.assert_allclose(means[b, :, 0], mean_gp, atol=1e-8, rtol=1e-8)
        np.testing.assert_allclose(variances[b, :, 0], var_gp, atol=1e-8, rtol=1e-8)
        np.testing.assert_allclose(lls[b], ll_gp, atol=1e-8, rtol=1e-8)
    assert m.kernel.variance == 1.0 and m.kernel.lengthscales == 1.0 and m.noise_variance == 0.1


def test_mixture_moments():
    from pssgp.kernels import Matern32
    from pssgp.model import StateSpaceGP
    t, y, tq = _data(200, 50, 7 * 200 + 50)
    thetas = _thetas(9, 3)
    m = StateSpaceGP((t[:, None], y[:, None]), Matern32(1.0, 1.0), noise_variance=0.1, parallel=False)
    means, variances = m.predict_f_batch(tq[:, None], thetas)
    mu, s2 = np.ascontiguousarray(means[:, :, 0]), np.ascontiguousarray(variances[:, :, 0])       # (B, K)
    w = np.random.RandomState(4).uniform(0.1, 2.0, 9)
    for weights in (None, w):
        wn = np.full(9, 1.0 / 9) if weights is None else weights / weights.sum()
        mean, var = m.predict_f_batch(tq[:, None], thetas, reduce="mixture", weights=weights)
        assert mean.shape == (50, 1) and var.shape == (50, 1)
        want_mean = np.sum(wn[:, None] * mu, axis=0)
        want_var = np.sum(wn[:, None] * (s2 + (mu - want_mean[None, :]) ** 2), axis=0)
        assert np.array_equal(mean[:, 0], want_mean) and np.array_equal(var[:, 0], want_var)
        # the other algebraic form of the same variance, E[x^2] - mean^2: pins the formula, not the rounding
        other = np.sum(wn[:, None] * (s2 + mu ** 2), axis=0) - want_mean ** 2
        assert np.max(np.abs(var[:, 0] - other)) < 1e-12
        assert np.all(var[:, 0] >= np.sum(wn[:, None] * s2, axis=0) - 1e-15)
    eq = m.predict_f_batch(tq[:, None], thetas, reduce="mixture")
    ones = m.predict_f_batch(tq[:, None], thetas, reduce="mixture", weights=np.ones(9))
    assert np.array_equal(eq[0], ones[0]) and np.array_equal(eq[1], ones[1])
    one = m.predict_f_batch(tq[:, None], thetas[:1], reduce="mixture")          # B = 1: that model's moments
    assert np.array_equal(one[0], means[0]) and np.array_equal(one[1], variances[0])
    with_ll = m.predict_f_batch(tq[:, None], thetas, reduce="mixture", return_log_likelihood=True)
    assert len(with_ll) == 3 and with_ll[2].shape == (9,)
