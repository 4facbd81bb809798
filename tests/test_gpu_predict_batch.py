"""GPU tests of the batched predict_f (pgps_gp_predict_batch_*, StateSpaceGP.predict_f_batch): the posterior at B
hyper-parameter settings over one series and one query grid in one set of launches, and the mixture of the B posteriors
reduced on the device (pgps_mix_moments_dev_f64) -- the last step of the reference's MCMC drivers
(pssgp/experiments/sunspot/mcmc.py:78-97)."""
import ctypes
import os

import numpy as np
import pytest

from tests.conftest import relerr

pytestmark = pytest.mark.gpu

TOL64, TOL32 = 1e-9, 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n, k, seed, nan_frac=0.1):
    """tests/test_gpu_predict.py's recipe with missing observations: some queries lie beyond the last observation."""
    rng = np.random.RandomState(seed)
    t = np.sort(rng.rand(n)) * (n / 80.0)
    y = np.sin(3.0 * t) + 0.3 * rng.randn(n)
    if n > 1:
        y[rng.rand(n) < nan_frac] = np.nan
    tq = np.sort(rng.rand(k)) * (n / 80.0) * 1.1
    return t, y, tq


def _models(kname, B, seed):
    """B fused models, every parameter exp(U(-1, 1)) (tests/test_gpu_batch.py's recipe)."""
    from pssgp import _backend as Bk
    from pssgp.kernels import Matern12, Matern32, Matern52
    cls = {"m12": Matern12, "m32": Matern32, "m52": Matern52}[kname]
    thetas = np.exp(np.random.RandomState(seed).uniform(-1.0, 1.0, (B, 3)))
    models = []
    for v, l, r in thetas:
        sde = cls(v, l).get_sde()
        models.append((Bk.nilpotent_form(sde.F), np.asarray(sde.P0), np.asarray(sde.H).reshape(-1), r))
    return models


def _single(models, t, y, tq):
    from pssgp import _backend as Bk
    out = [Bk.gp_predict(f, P, H, r, t, y, tq) for f, P, H, r in models]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out])


def _check(got, want, dtype, what):
    tol = TOL64 if dtype == np.float64 else TOL32
    em, ev = relerr(got[0], want[0]), relerr(got[1], want[1])
    el = float(np.max(np.abs(got[2] - want[2]) / np.abs(want[2])))
    print(f"{what}: mean {em:.2e} var {ev:.2e} ll {el:.2e}")
    assert em < tol and ev < tol, (what, em, ev)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-11 if dtype == np.float64 else 1e-4)


class _Form:
    """pgps_set_batch_form for the block, restored on every exit."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        from pssgp import _backend as Bk
        Bk.get_context().set_batch_form(self.form)

    def __exit__(self, *exc):
        from pssgp import _backend as Bk
        Bk.get_context().set_batch_form(0)
        return False


CASES = [(1, 5, 3), (255, 64, 5), (3000, 2000, 10), (4096, 1024, 64), (30011, 4099, 33), (100000, 20000, 7)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
@pytest.mark.parametrize("n,k,B", CASES)
def test_batch_equals_single_predicts(n, k, B, kname, dtype):
    """Every row of the batch against the single-model call (another launch geometry: equal to rounding)."""
    from pssgp import _backend as Bk
    t, y, tq = _data(n, k, n + k)
    t, y, tq = t.astype(dtype), y.astype(dtype), tq.astype(dtype)
    models = _models(kname, B, B)
    mean, var, ll, _ = Bk.gp_predict_batch(models, t, y, tq)
    assert mean.shape == (B, k) and var.shape == (B, k) and ll.shape == (B,) and mean.dtype == dtype
    _check((mean, var, ll), _single(models, t, y, tq), dtype, f"auto {kname} {n} {k} {B} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
@pytest.mark.parametrize("n,k,B", CASES[:4])
def test_both_forms_equal_single_predicts_and_each_other(n, k, B, kname, dtype):
    """One workgroup per model (form 1) and three launches of (workgroups, models) grids (form 2)."""
    from pssgp import _backend as Bk
    t, y, tq = _data(n, k, n + k)
    t, y, tq = t.astype(dtype), y.astype(dtype), tq.astype(dtype)
    models = _models(kname, B, B)
    want = _single(models, t, y, tq)
    got = {}
    for form in (1, 2):
        with _Form(form):
            got[form] = Bk.gp_predict_batch(models, t, y, tq)[:3]
        _check(got[form], want, dtype, f"form {form} {kname} {n} {k} {B} {np.dtype(dtype).name}")
    tol = TOL64 if dtype == np.float64 else TOL32
    assert relerr(got[1][0], got[2][0]) < tol and relerr(got[1][1], got[2][1]) < tol


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("n,k", [(300, 120), (120, 300), (200, 200)])
def test_tied_times_in_both_forms(n, k, form):
    """tests/test_gpu_predict.py::test_predict_with_tied_times_matches_oracle_merge's data: queries AT training times and
    repeated times, merged once for all models by the same kernel as the single call."""
    from pssgp import _backend as Bk
    rng = np.random.RandomState(n + k)
    t = np.sort(np.round(rng.rand(n) * 20.0, 1))
    y = np.cos(t) + 0.2 * rng.randn(n)
    tq = np.sort(np.round(rng.rand(k) * 22.0, 1))
    models = _models("m32", 4, 11)
    with _Form(form):
        got = Bk.gp_predict_batch(models, t, y, tq)[:3]
    _check(got, _single(models, t, y, tq), np.float64, f"ties form {form} {n} {k}")


@pytest.mark.parametrize("form", [0, 1, 2])
def test_invariance_bit_for_bit(form):
    from pssgp import _backend as Bk
    t, y, tq = _data(3000, 500, 5)
    models = _models("m52", 16, 3)
    ctx = Bk.get_context()
    with _Form(form):
        a = Bk.gp_predict_batch(models, t, y, tq)[:3]
        b = Bk.gp_predict_batch(models, t, y, tq)[:3]
        assert all(np.array_equal(x, z) for x, z in zip(a, b))                     # two identical calls
        perm = np.random.RandomState(0).permutation(16)
        p = Bk.gp_predict_batch([models[i] for i in perm], t, y, tq)[:3]
        assert all(np.array_equal(x[perm], z) for x, z in zip(a, p))               # the rows follow their settings
        # a budget of 2.5 MB: three to five models of this shape per group, so at least four groups (per model
        # (N + K)(d + d^2) scalars of moments = 336 kB, plus the lane records of the form: 90 to 370 kB)
        try:
            ctx.set_batch_scratch(5 * (3500 * 12 * 8 + 160 * 1024))
            g = Bk.gp_predict_batch(models, t, y, tq)[:3]
            ctx.set_batch_scratch(1)                                               # one model per group
            g1 = Bk.gp_predict_batch(models, t, y, tq)[:3]
        finally:
            ctx.set_batch_scratch(0)
        assert all(np.array_equal(x, z) for x, z in zip(a, g))
        assert all(np.array_equal(x, z) for x, z in zip(a, g1))
        c = Bk.gp_predict_batch([models[3]] * 16, t, y, tq)[:3]                    # B copies of one setting
        for x in c:
            assert all(np.array_equal(x[0], row) for row in x)
        assert all(np.array_equal(x[3], z[0]) for x, z in zip(a, c))               # ... each that setting's row of the batch


def _kernel(name):
    from pssgp.kernels import Matern12, Matern32, Matern52, RBF, Periodic, SquaredExponential
    return {"matern12": lambda: Matern12(1.0, 0.5), "matern32": lambda: Matern32(1.0, 0.5),
            "matern52": lambda: Matern52(1.0, 0.5),
            "rbf6": lambda: RBF(variance=1., lengthscales=0.5, order=6, balancing_iter=10),
            "periodic2": lambda: Periodic(SquaredExponential(1., 0.5), period=0.5, order=2),
            "m32*m52": lambda: Matern32(variance=1., lengthscales=0.5) * Matern52(variance=1., lengthscales=0.5),
            # tests/test_gpu_rowcoop.py's kernels, restated
            "rbf7": lambda: RBF(variance=1., lengthscales=0.7, order=7, balancing_iter=10),                       # d = 7
            "c5_qp_m52": lambda: Periodic(SquaredExponential(1., 1.), period=1., order=1) * Matern32(1., 1.) +
            Matern52(1., 1.),                                                                                     # d = 11
            "rbf13": lambda: RBF(variance=1., lengthscales=0.6, order=13, balancing_iter=10),                     # d = 13
            "periodic7": lambda: Periodic(SquaredExponential(1., 0.5), period=0.5, order=7)}[name]()              # d = 16


def _perturbed(m, B, seed, spread=0.5):
    base = np.array([getattr(o, n) for o, n in m.trainable_parameters()], np.float64)
    return base[None, :] * np.exp(np.random.RandomState(seed).uniform(-spread, spread, (B, base.size)))


def _lti_models(kname, B, seed):
    """B general-LTI models (F, Pinf, H, R): variances, lengthscales, periods' base parameters and the noise of `kname`
    varied per row by factors exp(U(-0.5, 0.5))."""
    from pssgp.model import StateSpaceGP
    m = StateSpaceGP((np.arange(3.0)[:, None], np.zeros((3, 1))), _kernel(kname), noise_variance=0.1, parallel=True)
    params = m.trainable_parameters()
    names = [n for _, n in params]
    base = np.array([getattr(o, n) for o, n in params], np.float64)
    fac = np.exp(np.random.RandomState(seed).uniform(-0.5, 0.5, (B, base.size)))
    fac[:, [i for i, n in enumerate(names) if n == "period"]] = 1.0
    out = []
    for row in base[None, :] * fac:
        for (o, n), v in zip(params, row):
            setattr(o, n, float(v))
        sde = m.kernel.get_sde()
        out.append((np.array(sde.F, np.float64), np.array(sde.P0, np.float64), np.array(sde.H, np.float64).reshape(-1), float(row[-1])))
    return out


def _lti_single(models, t, y, tq):
    from pssgp import _backend as Bk
    out = [Bk.lti_predict(F, P, H, r, t, y, tq) for F, P, H, r in models]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out])


@pytest.mark.parametrize("kname", ["rbf6", "periodic2", "m32*m52", "rbf7", "c5_qp_m52", "rbf13", "periodic7"])
def test_lti_batch_equals_single_predicts(kname):
    """pgps_lti_predict_batch_f64 against B single lti_predict calls, host arrays and resident series, with the mixture."""
    from pssgp import _backend as Bk
    from pssgp.model import StateSpaceGP
    t, y, tq = _data(1500, 400, 21)
    models = _lti_models(kname, 5, 8)
    want = _lti_single(models, t, y, tq)
    got = Bk.lti_predict_batch(models, t, y, tq)
    _check(got[:3], want, np.float64, f"lti {kname} d={models[0][0].shape[0]}")
    ser = Bk.Series(t, y)
    try:
        ser.set_queries(tq)
        sgot = ser.lti_predict_batch(models)
        _check(sgot[:3], want, np.float64, f"lti series {kname}")
        w = np.full(5, 0.2)
        _, _, sll, (mm, mv) = ser.lti_predict_batch(models, mix=w)
        wm, wv = StateSpaceGP._mix_moments_host(sgot[0], sgot[1], w)
        assert relerr(mm, wm) < 1e-12 and relerr(mv, wv) < 1e-12 and np.array_equal(sll, sgot[2])
    finally:
        ser.close()
    again = Bk.lti_predict_batch(models, t, y, tq)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3]))
    # the chain geometry is fixed per call: groups of two models and of one give the bits of the whole batch, and a
    # permutation of the models permutes the rows
    ctx = Bk.get_context()
    d = models[0][0].shape[0]
    try:
        ctx.set_batch_scratch(2 * (3 * 1900 * d * d + 1900 * d) * 8 + 4096)
        two = Bk.lti_predict_batch(models, t, y, tq)
        ctx.set_batch_scratch(1)
        one = Bk.lti_predict_batch(models, t, y, tq)
    finally:
        ctx.set_batch_scratch(0)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], two[:3]))
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], one[:3]))
    perm = [3, 0, 4, 1, 2]
    p = Bk.lti_predict_batch([models[i] for i in perm], t, y, tq)
    assert all(np.array_equal(a[perm], b) for a, b in zip(got[:3], p[:3]))


def test_lti_batch_long_series():
    from pssgp import _backend as Bk
    t, y, tq = _data(2 ** 17, 2 ** 13, 3)
    models = _lti_models("rbf6", 4, 2)
    got = Bk.lti_predict_batch(models, t, y, tq)
    _check(got[:3], _lti_single(models, t, y, tq), np.float64, "lti long rbf6")


def test_lti_batch_errors_and_no_memory():
    """d = 17 to the general call, R <= 0, and scratch that cannot be had: PGPS_E_NOMEM with no sticky HIP error -- a
    good call follows each."""
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    lib = ctx.lib
    t, y, tq = _data(200, 30, 1)
    models = _lti_models("rbf6", 3, 1)
    table, d = Bk._lti_table(models)
    mean, var, ll = np.empty((3, 30)), np.empty((3, 30)), np.empty(3)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(B, dd, tab):
        with ctx.lock:
            return lib.pgps_lti_predict_batch_f64(ctx.handle, B, 200, 30, dd, P(tab), P(t), P(y), 0.0, P(tq), P(mean), P(var), P(ll))

    def good():
        _check(Bk.lti_predict_batch(models, t, y, tq)[:3], _lti_single(models, t, y, tq), np.float64, "lti after an error")
        fm = _models("m32", 3, 1)
        _check(Bk.gp_predict_batch(fm, t, y, tq)[:3], _single(fm, t, y, tq), np.float64, "fused after an error")

    assert call(3, 17, np.zeros((3, 2 * 17 * 17 + 17 + 1))) == -2
    good()
    assert call(0, d, table) == -1
    bad = table.copy()
    bad[1, -1] = 0.0
    assert call(3, d, bad) == -1
    good()
    # ONE (B, K) staging array larger than the whole device memory, whatever the device: the allocation cannot succeed, so
    # the small output arrays are never written
    import torch
    K = 2 ** 20
    nb = int(torch.cuda.get_device_properties(0).total_memory // (8 * K)) + 1024
    assert nb <= 65535 * 64
    tq_big = np.sort(np.random.RandomState(0).rand(K)) * t[-1]
    fm = np.tile(Bk._gp_rows(_models("m32", 1, 1))[0], (nb, 1))
    with ctx.lock:
        rc = lib.pgps_gp_predict_batch_f64(ctx.handle, nb, 200, K, 2, P(fm), P(t), P(y), 0.0, P(tq_big), P(mean), P(var), None)
    assert rc == -4                                          # PGPS_E_NOMEM
    good()
    big = np.tile(table[:1], (nb, 1))
    with ctx.lock:
        rc = lib.pgps_lti_predict_batch_f64(ctx.handle, nb, 200, K, d, P(big), P(t), P(y), 0.0, P(tq_big), P(mean), P(var), None)
    assert rc == -4
    good()


# (rbf13, d = 13, is compared against single device calls above only: the host twin discretises with scipy's expm, whose
# error at that conditioning -- cond Pinf ~ 1e5 -- has no bound to hold the comparison to)
@pytest.mark.parametrize("kname", ["matern12", "matern32", "matern52", "rbf6", "periodic2", "m32*m52", "rbf7", "c5_qp_m52",
                                   "periodic7", "co2"])
def test_model_device_against_host(kname):
    """parallel=True against the host twin (parallel=False), on the first evaluation (host arrays) and on a later one
    (resident series); parameters restored."""
    from pssgp.experiments.real_data import co2_covariance
    from pssgp.model import StateSpaceGP
    make = co2_covariance if kname == "co2" else (lambda: _kernel(kname))
    n, k, B = (400, 90, 3) if kname == "co2" else (600, 150, 5) if kname in ("rbf7", "c5_qp_m52", "periodic7") else (1500, 400, 5)
    t, y, tq = _data(n, k, 9, nan_frac=0.0)
    dev = StateSpaceGP((t[:, None], y[:, None]), make(), noise_variance=0.1, parallel=True)
    host = StateSpaceGP((t[:, None], y[:, None]), make(), noise_variance=0.1, parallel=False)
    params = dev.trainable_parameters()
    before = [getattr(o, n) for o, n in params]
    thetas = _perturbed(dev, B, 4, 0.2 if kname == "co2" else 0.5)
    want = host.predict_f_batch(tq[:, None], thetas, return_log_likelihood=True)
    first = dev.predict_f_batch(tq[:, None], thetas, return_log_likelihood=True)
    later = dev.predict_f_batch(tq[:, None], thetas, return_log_likelihood=True)
    assert [getattr(o, n) for o, n in params] == before
    for name, got in (("first", first), ("resident", later)):
        assert got[0].shape == (B, k, 1) and got[1].shape == (B, k, 1) and got[2].shape == (B,)
        em, ev = relerr(got[0], want[0]), relerr(got[1], want[1])
        print(f"model {kname} {name}: mean {em:.2e} var {ev:.2e}")
        assert em < TOL64 and ev < TOL64
        np.testing.assert_allclose(got[2], want[2], rtol=1e-9)
    assert relerr(first[0], later[0]) < TOL64 and relerr(first[1], later[1]) < TOL64
    # shuffled queries with repeats, mixture: the reduction of the unreduced call
    pick = np.random.RandomState(1).randint(0, k, 2 * k)
    m2, v2 = dev.predict_f_batch(tq[pick][:, None], thetas)
    uniq, inverse = np.unique(tq[pick], return_inverse=True)
    mu, vu = dev.predict_f_batch(uniq[:, None], thetas)
    assert np.array_equal(m2, mu[:, inverse]) and np.array_equal(v2, vu[:, inverse])     # the rows of the sorted unique call
    assert relerr(m2, later[0][:, pick]) < TOL64 and relerr(v2, later[1][:, pick]) < TOL64
    w = np.random.RandomState(2).uniform(0.5, 1.5, B)
    mm, mv = dev.predict_f_batch(tq[:, None], thetas, reduce="mixture", weights=w)
    wm, wv = StateSpaceGP._mix_moments_host(later[0][:, :, 0], later[1][:, :, 0], w / w.sum())
    assert relerr(mm[:, 0], wm) < 1e-12 and relerr(mv[:, 0], wv) < 1e-12
    # a single setting takes the single call: the same numbers as predict_f at that setting
    one = dev.predict_f_batch(tq[:, None], thetas[:1])
    assert relerr(one[0][0], later[0][0]) < TOL64 and relerr(one[1][0], later[1][0]) < TOL64


def test_float32_model_against_fp64():
    from pssgp import config
    from pssgp.kernels import Matern32
    from pssgp.model import StateSpaceGP
    t, y, tq = _data(1500, 400, 9, nan_frac=0.0)
    m64 = StateSpaceGP((t[:, None], y[:, None]), Matern32(1.0, 0.5), noise_variance=0.1, parallel=True)
    thetas = _perturbed(m64, 5, 4)
    want = m64.predict_f_batch(tq[:, None], thetas)
    config.set_default_float(np.float32)
    try:
        m32 = StateSpaceGP((t[:, None], y[:, None]), Matern32(1.0, 0.5), noise_variance=0.1, parallel=True)
        got = m32.predict_f_batch(tq[:, None], thetas)
        mix = m32.predict_f_batch(tq[:, None], thetas, reduce="mixture")
    finally:
        config.set_default_float(np.float64)
    assert got[0].dtype == np.float32 and got[0].shape == (5, 400, 1)
    assert relerr(got[0], want[0]) < TOL32 and relerr(got[1], want[1]) < TOL32
    wm, wv = StateSpaceGP._mix_moments_host(want[0][:, :, 0], want[1][:, :, 0], np.full(5, 0.2))
    assert relerr(mix[0][:, 0], wm) < TOL32 and relerr(mix[1][:, 0], wv) < TOL32


@pytest.mark.parametrize("B,K", [(1, 7), (9, 50), (64, 1024), (1000, 2000), (1024, 129)])
def test_mixture_on_the_device_against_numpy(B, K):
    """A sum of B non-negative fp64 terms per pass: B eps = 2.3e-13 at B = 1024."""
    from pssgp import _backend as Bk
    from pssgp.model import StateSpaceGP
    rng = np.random.RandomState(B + K)
    mean = rng.randn(B, K) * 3.0 + 10.0
    var = rng.uniform(0.01, 2.0, (B, K))
    w = rng.uniform(0.0, 1.0, B)
    w /= w.sum()
    for weights, wn in ((None, np.full(B, 1.0 / B)), (w, w)):
        mm, mv = Bk.mix_moments(mean, var, weights)
        wm, wv = StateSpaceGP._mix_moments_host(mean, var, wn)
        em, ev = relerr(mm, wm), relerr(mv, wv)
        print(f"mix B={B} K={K} {'equal' if weights is None else 'random'}: mean {em:.2e} var {ev:.2e}")
        assert em < 1e-12 and ev < 1e-12
        again = Bk.mix_moments(mean, var, weights)
        assert np.array_equal(mm, again[0]) and np.array_equal(mv, again[1])


def test_mixture_of_the_batch_stays_on_the_device():
    """reduce on the device from the (B, K) results of the same call, host arrays and resident series."""
    from pssgp import _backend as Bk
    from pssgp.model import StateSpaceGP
    t, y, tq = _data(3000, 2000, 8)
    models = _models("m32", 100, 6)
    w = np.random.RandomState(3).uniform(0.1, 1.0, 100)
    w /= w.sum()
    mean, var, ll, _ = Bk.gp_predict_batch(models, t, y, tq)
    wm, wv = StateSpaceGP._mix_moments_host(mean, var, w)
    none_m, none_v, ll2, (mm, mv) = Bk.gp_predict_batch(models, t, y, tq, mix=w)
    assert none_m is None and none_v is None and np.array_equal(ll, ll2)
    assert relerr(mm, wm) < 1e-12 and relerr(mv, wv) < 1e-12
    ser = Bk.Series(t, y)
    try:
        ser.set_queries(tq)
        smean, svar, sll, _ = ser.gp_predict_batch(models)
        assert np.array_equal(smean, mean) and np.array_equal(svar, var) and np.array_equal(sll, ll)
        _, _, sll2, (sm, sv) = ser.gp_predict_batch(models, mix=w)
        assert np.array_equal(sm, mm) and np.array_equal(sv, mv) and np.array_equal(sll2, ll)
    finally:
        ser.close()


def test_errors_leave_the_context_usable():
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    lib = ctx.lib
    t, y, tq = _data(200, 30, 1)
    models = _models("m32", 3, 1)
    packed, d = Bk._gp_rows(models)
    mean, var, ll = np.empty((3, 30)), np.empty((3, 30)), np.empty(3)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(B, dd, table, tq_ptr):
        with ctx.lock:
            return lib.pgps_gp_predict_batch_f64(ctx.handle, B, 200, 30, dd, P(table), P(t), P(y), 0.0, tq_ptr, P(mean), P(var), P(ll))

    def good():
        got = Bk.gp_predict_batch(models, t, y, tq)[:3]
        _check(got, _single(models, t, y, tq), np.float64, "after an error")

    good()
    bad = packed.copy()
    bad[1, -1] = -0.1                                        # R <= 0 in one row
    assert call(3, d, bad, P(tq)) == -1
    good()
    bad = packed.copy()
    bad[2, 0] = 0.0                                          # lam <= 0
    assert call(3, d, bad, P(tq)) == -1
    assert call(0, d, packed, P(tq)) == -1                   # B = 0
    good()
    assert call(3, 4, np.zeros((3, 1 + 3 * 16 + 4 + 1)), P(tq)) == -2       # d = 4: PGPS_E_UNSUPPORTED_DIM
    good()
    assert call(3, d, packed, None) == -1                    # tq = NULL
    good()
    with ctx.lock:
        assert lib.pgps_set_batch_form(ctx.handle, 3) == -1
        assert lib.pgps_mix_moments_dev_f64(ctx.handle, 0, 5, None, None, None, None, None) == -1
    good()
    with pytest.raises(Bk.PgpsError):
        Bk.gp_predict_batch([(models[0][0], models[0][1], models[0][2], -1.0)], t, y, tq)
    good()


def test_sunspot_posterior_predictive():
    """sunspot/mcmc.py:78-97 at the reference's smallest training size with a 20-sample chain."""
    from pssgp.experiments.real_data import load_sunspots, sunspot_covariance, sunspot_posterior_predictive
    from pssgp.model import StateSpaceGP
    data_dir = os.path.join(ROOT, "tests", "golden", "real")
    out = sunspot_posterior_predictive(data_dir, n_training=50, n_samples=20, n_burnin=5, n_interp=300)
    assert out["curves"].shape == (20, 300) and out["thetas"].shape == (20, 3)
    assert out["mean"].shape == (300,) and out["variance"].shape == (300,)
    assert np.all(np.isfinite(out["curves"])) and np.all(np.isfinite(out["mean"])) and np.all(out["variance"] > 0.0)
    assert np.all(out["band"][0] < out["mean"]) and np.all(out["mean"] < out["band"][1])
    assert np.all(np.diff(out["times"]) >= 0) and set(out["seconds"]) == {"chain", "curves", "mixture"}
    few = sunspot_posterior_predictive(data_dir, n_training=50, n_draws=10, n_samples=20, n_burnin=5, n_interp=300)
    assert few["curves"].shape == (10, 300)
    # the curves are the loop a user writes over predict_f
    t, y = load_sunspots(data_dir, 50)
    gp = StateSpaceGP((t, y), sunspot_covariance(), 10., parallel=True)
    for row, curve, cvar in zip(out["thetas"], out["curves"], out["curve_variances"]):
        gp.kernel.variance, gp.kernel.lengthscales, gp.noise_variance = float(row[0]), float(row[1]), float(row[2])
        mean, var = gp.predict_f(out["times"][:, None])
        assert relerr(curve, mean[:, 0]) < TOL64 and relerr(cvar, var[:, 0]) < TOL64
