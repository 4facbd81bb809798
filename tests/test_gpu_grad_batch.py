"""GPU tests of the batched adjoint pass (pgps_gp_ll_grad_adj_batch_*, pgps_lti_ll_grad_batch_*, include/pgps.h) and of
StateSpaceGP.log_likelihood_and_grad_batch: every row of a batch against the numpy reverse sweep of oracle/np_grad.py at
the tolerances tests/test_gpu_adjoint.py holds the single calls to, bitwise independence of a row from its place, its
neighbours and the groups, the model-level method against log_likelihood_and_grad row by row, the C ABI's error codes, and
the lock-step HMC driver against the single-chain one."""
import ctypes

import numpy as np
import pytest

from oracle import np_grad as G
from tests.test_gpu_adjoint import _check_stats, _kernels, _series

pytestmark = pytest.mark.gpu

# (variance, lengthscale, R): the settings tests/test_gpu_adjoint.py holds the single call to
SETTINGS = [(1.3, 0.7, 0.2), (0.9, 0.45, 0.12), (2.2, 1.1, 0.12), (1.1, 0.8, 0.25), (1.2, 0.6, 0.15)]


def _matern(kname, s2, ell):
    from pssgp.kernels import Matern12, Matern32, Matern52
    return {"m12": Matern12, "m32": Matern32, "m52": Matern52}[kname](s2, ell)


def _fused_models(kname, settings=SETTINGS):
    """[(form, Pinf, H, R)] as gp_ll_batch takes them, and the SDEs."""
    from pssgp import _backend as B
    models, sdes = [], []
    for s2, ell, R in settings:
        sde = _matern(kname, s2, ell).get_sde()
        form = B.nilpotent_form(sde.F)
        assert form is not None
        models.append((form, sde.P0, np.asarray(sde.H).reshape(-1), R))
        sdes.append(sde)
    return models, sdes


def _check_rows(rows, refs, d, tol):
    from pssgp import _backend as B
    assert rows.shape == (len(refs), 2 + d * d + 2 * d)
    for row, ref in zip(rows, refs):
        _check_stats(B.split_grad_stats(row, d), ref, tol)


@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
@pytest.mark.parametrize("n,chunk", [(1, 0), (2, 0), (37, 0), (700, 0), (2048, 0), (2049, 0), (5000, 3), (3000, 1)])
def test_fused_rows_match_the_reverse_sweep(kname, n, chunk):
    """One step, less than a workgroup, the one-launch form and its boundary, three or more workgroups with ragged tails,
    one step per lane; 15 % of the observations missing: every row of B = 5 on the resident series and on the host-array
    entry point (and once on the device-pointer one) against the oracle."""
    from pssgp import _backend as B
    from tests.test_segments import _Dev
    t, y = _series(n, seed=11 + n, nan_frac=0.15 if n > 2 else 0.0)
    models, sdes = _fused_models(kname)
    d = sdes[0].F.shape[0]
    refs = [G.ll_grad_stats(s.F, s.P0, s.H, R, t, y) for s, (_, _, R) in zip(sdes, SETTINGS)]
    ctx = B.get_context()
    ctx.set_chunk(chunk)
    ser = B.Series(t, y)
    try:
        _check_rows(ser.gp_ll_grad_adj_batch(models), refs, d, 1e-9)
        _check_rows(B.gp_ll_grad_adj_batch(models, t, y), refs, d, 1e-9)
        if (kname, n) == ("m52", 5000):
            table, _ = B._gp_rows(models)
            ts, ys, out = _Dev(ctx, t), _Dev(ctx, y), _Dev(ctx, shape=(5, 2 + d * d + 2 * d))
            try:
                ctx.call("pgps_gp_ll_grad_adj_batch_dev_f64", ctypes.c_int(5), ctypes.c_long(n), ctypes.c_int(d),
                         table.ctypes.data_as(ctypes.c_void_p), ts.p, ctypes.c_double(0.0), ys.p, out.p)
                ctx.synchronize()
                _check_rows(out.get(), refs, d, 1e-9)
            finally:
                for b in (ts, ys, out):
                    b.free()
    finally:
        ctx.set_chunk(0)
        ser.close()


def test_fused_rows_are_independent_bit_for_bit():
    """m32, n = 5000, 3 steps per lane: row b does not depend on its place in the table, on the groups the batch budget
    cuts the table into, or on the other rows; B = 1 works."""
    from pssgp import _backend as B
    t, y = _series(5000, seed=31, nan_frac=0.15)
    models, sdes = _fused_models("m32")
    ctx = B.get_context()
    ctx.set_chunk(3)
    ser = B.Series(t, y)
    try:
        base = ser.gp_ll_grad_adj_batch(models)
        assert np.array_equal(ser.gp_ll_grad_adj_batch(models[::-1])[::-1], base)
        # one model's scratch (launch_gp_adj_batch, d = 2, 7 workgroups, 1792 lanes, every part rounded up to 256 bytes):
        # filter records 1024 + 200704 (14 doubles per workgroup / lane), adjoint records 512 + 129024 (9 doubles), 256 for
        # the log-likelihood partials, kept states 3 steps x 5 doubles x 1792 lanes = 215040, partials 512: 547072 bytes.
        # 1.2 MB holds two models and not three: B = 5 runs as groups of 2, 2, 1; 600 KiB holds one: five groups of one
        per_model = 1024 + 200704 + 512 + 129024 + 256 + 215040 + 512
        assert 2 * per_model <= 1200 * 1024 < 3 * per_model and per_model <= 600 * 1024 < 2 * per_model
        for budget in (1200 * 1024, 600 * 1024):
            ctx.set_batch_scratch(budget)
            try:
                assert np.array_equal(ser.gp_ll_grad_adj_batch(models), base)
                assert np.array_equal(B.gp_ll_grad_adj_batch(models, t, y), base)
            finally:
                ctx.set_batch_scratch(0)
        for b in range(5):
            assert np.array_equal(ser.gp_ll_grad_adj_batch([models[b]] * 5), np.broadcast_to(base[b], base.shape))
        one = ser.gp_ll_grad_adj_batch(models[2:3])
        ref = G.ll_grad_stats(sdes[2].F, sdes[2].P0, sdes[2].H, SETTINGS[2][2], t, y)
        _check_rows(one, [ref], 2, 1e-9)
    finally:
        ctx.set_chunk(0)
        ser.close()


def _lti_models(name):
    """B = 3 rows of the kernel's SDE: R = 0.1, R = 0.25, and (F / 1.25, 2 Pinf) at R = 0.1 (a longer lengthscale, twice the
    variance: still a stationary model)."""
    sde = _kernels()[name]().get_sde()
    F, P, H = np.asarray(sde.F, np.float64), np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1)
    return [(F, P, H, 0.1), (F, P, H, 0.25), (F / 1.25, 2.0 * P, H, 0.1)]


def _rc_scratch_per_model(n, d, B, chunk):
    """Bytes of scratch launch_ll_grad_lti_batch (csrc/pgps_wc.hip) charges to the batch budget per model: transition
    matrices and kept covariances (n d^2 doubles each), kept means (n d), and per chain -- Lw steps each: pgps_set_chunk's
    value, else ceil(n B / 8192) clamped to [8, 128] -- two buffers of filter records (3 d^2 + 2 d doubles), two of adjoint
    records (2 d^2 + d), the log-likelihood partial and the d^2 + 2 d + 1 partials, every part rounded up to 256 bytes."""
    up = lambda x: (x + 255) // 256 * 256
    lw = chunk if chunk > 0 else min(128, max(8, -(-n * B // 8192)))
    nc = -(-n // lw)
    dd = d * d
    return (2 * n * dd + n * d) * 8 + 2 * up(nc * (3 * dd + 2 * d) * 8) + 2 * up(nc * (2 * dd + d) * 8) + up(nc * 8) \
        + up(nc * (dd + 2 * d + 1) * 8)


@pytest.mark.parametrize("name", ["rbf6", "c5", "rbf15"])
@pytest.mark.parametrize("n", [37, 1300])
@pytest.mark.parametrize("chunk", [0, 5])
def test_row_cooperative_rows_match_the_reverse_sweep(name, n, chunk):
    """Every row of a batch on the row-cooperative kernels (d = 6, 11, 15) against the oracle, on the resident series and the
    host-array entry point; a row does not depend on its place or on the groups, bit for bit."""
    from pssgp import _backend as B
    models = _lti_models(name)
    d = models[0][0].shape[0]
    t, y = _series(n, seed=3 + n)
    refs = [G.ll_grad_stats(F, P, H, R, t, y) for F, P, H, R in models]
    tol = 5e-8 if name == "rbf15" else 1e-9
    ctx = B.get_context()
    ctx.set_chunk(chunk)
    ser = B.Series(t, y)
    try:
        base = ser.lti_ll_grad_batch(models)
        _check_rows(base, refs, d, tol)
        host = B.lti_ll_grad_batch(models, t, y)
        _check_rows(host, refs, d, tol)
        assert np.array_equal(host, base)
        assert np.array_equal(ser.lti_ll_grad_batch(models[::-1])[::-1], base)
        # groups of 2, 1 (a budget of two and a half models) and three groups of one (one and a half)
        per_model = _rc_scratch_per_model(n, d, 3, chunk)
        for budget in (5 * per_model // 2, 3 * per_model // 2):
            ctx.set_batch_scratch(budget)
            try:
                assert np.array_equal(ser.lti_ll_grad_batch(models), base)
            finally:
                ctx.set_batch_scratch(0)
    finally:
        ctx.set_chunk(0)
        ser.close()


def test_row_cooperative_device_pointer_entry_point_and_one_row():
    from pssgp import _backend as B
    from tests.test_segments import _Dev
    models = _lti_models("rbf6")
    d, n = 6, 1300
    t, y = _series(n, seed=3 + n)
    refs = [G.ll_grad_stats(F, P, H, R, t, y) for F, P, H, R in models]
    ctx = B.get_context()
    table, _ = B._lti_table(models)
    ts, ys, out = _Dev(ctx, t), _Dev(ctx, y), _Dev(ctx, shape=(3, 2 + d * d + 2 * d))
    try:
        ctx.call("pgps_lti_ll_grad_batch_dev_f64", ctypes.c_int(3), ctypes.c_long(n), ctypes.c_int(d),
                 table.ctypes.data_as(ctypes.c_void_p), ts.p, ys.p, ctypes.c_double(0.0), out.p)
        ctx.synchronize()
        _check_rows(out.get(), refs, d, 1e-9)
    finally:
        for b in (ts, ys, out):
            b.free()
    _check_rows(B.lti_ll_grad_batch(models[1:2], t, y), refs[1:2], d, 1e-9)      # B = 1


def test_state_dimensions_above_16_go_through_the_stream():
    from pssgp import _backend as B
    models = _lti_models("co2")
    d = models[0][0].shape[0]
    assert d == 18
    t, y = _series(300, seed=303)
    refs = [G.ll_grad_stats(F, P, H, R, t, y) for F, P, H, R in models]
    _check_rows(B.lti_ll_grad_batch(models, t, y), refs, d, 1e-9)


def _thetas_for(gp, B, seed):
    """B settings around the model's own: every parameter scaled by a factor in [0.8, 1.25]."""
    rng = np.random.default_rng(seed)
    x0 = np.array([getattr(o, n) for o, n in gp.trainable_parameters()], np.float64)
    return x0[None, :] * rng.uniform(0.8, 1.25, size=(B, x0.size))


def _rowwise_adjoint(gp, thetas):
    params = gp.trainable_parameters()
    saved = [getattr(o, n) for o, n in params]
    lls, gs = [], []
    try:
        for row in thetas:
            for (o, n), v in zip(params, row):
                setattr(o, n, float(v))
            ll, g = gp.log_likelihood_and_grad(method="adjoint")
            lls.append(float(ll))
            gs.append(np.asarray(g, np.float64))
    finally:
        for (o, n), v in zip(params, saved):
            setattr(o, n, v)
    return np.array(lls), np.stack(gs)


def _model_kernel(name):
    from pssgp.kernels import Matern32, Matern52
    if name == "m32":
        return Matern32(1.3, 0.7)
    if name == "m52":
        return Matern52(1.1, 0.8)
    return _kernels()[name]()


@pytest.mark.parametrize("name", ["m32", "m52", "m32+m52", "c5"])
@pytest.mark.parametrize("n", [300, 3000])
def test_model_level_rows_equal_the_single_adjoint_gradient(name, n):
    from pssgp.model import StateSpaceGP
    t, y = _series(n, seed=5 + n, nan_frac=0.1)
    gp = StateSpaceGP((t[:, None], y[:, None]), _model_kernel(name), noise_variance=0.15, parallel=True)
    params = gp.trainable_parameters()
    before = [getattr(o, a) for o, a in params]
    thetas = _thetas_for(gp, 4, seed=n)
    want_ll, want_g = _rowwise_adjoint(gp, thetas)
    fresh = StateSpaceGP((t[:, None], y[:, None]), _model_kernel(name), noise_variance=0.15, parallel=True)
    for m in (fresh, gp):                       # a model's first evaluation (host arrays), then the resident series
        lls, grads = m.log_likelihood_and_grad_batch(thetas)
        assert lls.shape == (4,) and grads.shape == (4, len(params))
        assert np.all(np.abs(lls - want_ll) <= 1e-10 * np.abs(want_ll))
        for b in range(4):
            assert np.max(np.abs(grads[b] - want_g[b])) <= 1e-9 * max(1.0, float(np.max(np.abs(want_g[b])))), (b, grads[b], want_g[b])
    _, g0 = gp.log_likelihood_and_grad_batch(thetas, wrt=[0])
    assert np.array_equal(g0[:, 0], grads[:, 0]) and not g0[:, 1:].any()
    assert [getattr(o, a) for o, a in params] == before
    bad = thetas.copy()
    bad[2, 1] = -0.5                            # a negative lengthscale in row 2
    from pssgp._backend import PgpsError
    with pytest.raises((PgpsError, ValueError)):
        gp.log_likelihood_and_grad_batch(bad)
    assert [getattr(o, a) for o, a in params] == before


def _outcome(fn):
    """("ok", lls, grads) or ("raised", exception type, error code) of a gradient evaluation."""
    try:
        ll, g = fn()
    except Exception as e:          # noqa: BLE001 -- whatever the single call raises is the outcome to reproduce
        return ("raised", type(e), getattr(e, "code", None))
    return ("ok", np.asarray(ll, np.float64), np.asarray(g, np.float64))


@pytest.mark.parametrize("what", ["float32", "unsorted"])
def test_series_the_batch_does_not_take_give_the_loop_results(what):
    """A float32 series and an unsorted one do not go to the batched launches: the method gives what the loop over
    log_likelihood_and_grad gives -- the same numbers bit for bit, or, where the single call refuses the series (times that
    are not sorted have no state-space likelihood: PGPS_E_NUMERIC), the same error -- and puts the parameters back."""
    from pssgp import config
    from pssgp.kernels import Matern52
    from pssgp.model import StateSpaceGP
    t, y = _series(400, seed=9, nan_frac=0.1)
    if what == "unsorted":
        perm = np.random.default_rng(0).permutation(t.size)
        t, y = t[perm], y[perm]
    if what == "float32":
        config.set_default_float(np.float32)
    try:
        gp = StateSpaceGP((t[:, None], y[:, None]), Matern52(1.1, 0.8), noise_variance=0.15, parallel=True)
        assert gp.data[0].dtype == (np.float32 if what == "float32" else np.float64)
        thetas = _thetas_for(gp, 3, seed=1)
        params = gp.trainable_parameters()

        def loop():
            lls, gs = [], []
            try:
                for row in thetas:
                    for (o, a), v in zip(params, row):
                        setattr(o, a, float(v))
                    ll, g = gp.log_likelihood_and_grad()
                    lls.append(float(ll))
                    gs.append(np.asarray(g, np.float64))
            finally:
                for (o, a), v in zip(params, (1.1, 0.8, 0.15)):
                    setattr(o, a, v)
            return np.array(lls), np.stack(gs)

        want = _outcome(loop)
        for _ in range(2):                      # a model's first evaluations and its later ones
            got = _outcome(lambda: gp.log_likelihood_and_grad_batch(thetas))
            assert got[0] == want[0]
            if want[0] == "ok":
                assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            else:
                assert got[1:] == want[1:]
            assert [getattr(o, a) for o, a in params] == [1.1, 0.8, 0.15]
    finally:
        config.set_default_float(np.float64)
    if what == "float32":
        assert want[0] == "ok"                  # (the float32 series has a gradient: numbers were compared)


def test_error_codes_through_ctypes():
    from pssgp import _backend as B
    ctx = B.get_context()
    lib = ctx.lib
    n = 50
    t, y = _series(n, seed=4, nan_frac=0.0)
    models, _ = _fused_models("m32")
    table, d = B._gp_rows(models)
    out = np.zeros((5, 2 + d * d + 2 * d))
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(Bn=5, dd=d, tab=table, outp=None):
        return lib.pgps_gp_ll_grad_adj_batch_f64(ctx.handle, Bn, n, dd, P(tab), P(t), ctypes.c_double(0.0), P(y),
                                                 P(out) if outp is None else outp)

    assert call() == 0
    assert call(Bn=0) == -1
    assert call(outp=ctypes.c_void_p(None)) == -1
    bad = table.copy()
    bad[1, -1] = 0.0                            # R = 0 in row 1
    assert call(tab=bad) == -1
    assert call(dd=4) == -2
    # the general-LTI batch: d = 17 has no batched kernel
    d17 = 17
    tab17 = np.ones((2, 2 * d17 * d17 + d17 + 1))
    out17 = np.zeros((2, 2 + d17 * d17 + 2 * d17))
    assert lib.pgps_lti_ll_grad_batch_f64(ctx.handle, 2, n, d17, P(tab17), P(t), P(y), ctypes.c_double(0.0), P(out17)) == -2
    lmodels = _lti_models("rbf6")
    ltab, ld = B._lti_table(lmodels)
    lout = np.zeros((3, 2 + ld * ld + 2 * ld))
    assert lib.pgps_lti_ll_grad_batch_f64(ctx.handle, 3, n, ld, P(ltab), P(t), P(y), ctypes.c_double(0.0), P(lout)) == 0
    assert lib.pgps_lti_ll_grad_batch_f64(ctx.handle, 0, n, ld, P(ltab), P(t), P(y), ctypes.c_double(0.0), P(lout)) == -1
    lbad = ltab.copy()
    lbad[1, -1] = 0.0
    assert lib.pgps_lti_ll_grad_batch_f64(ctx.handle, 3, n, ld, P(lbad), P(t), P(y), ctypes.c_double(0.0), P(lout)) == -1


def test_lock_step_hmc_walks_the_single_chains_paths():
    """m32, n = 200, C = 3, 15 iterations of 5 leapfrogs, no adaptation: chain c of hmc_chains == hmc with chain c's seed from
    the same start (1e-6: the batched adjoint pass against the single call's gradient, a handful of accept / reject
    decisions); the model is left at chain 0's last point."""
    from pssgp.experiments.toy import hmc, hmc_chains
    from pssgp.kernels import Matern32
    from pssgp.model import StateSpaceGP
    t, y = _series(200, seed=77, nan_frac=0.0)
    seeds = [101, 202, 303]

    def model():
        return StateSpaceGP((t[:, None], y[:, None]), Matern32(1.1, 0.9), noise_variance=0.2, parallel=True)

    gp = model()
    samples, rates = hmc_chains(gp, 3, n_samples=10, n_burnin=5, step_size=0.02, n_leapfrogs=5, seeds=seeds, adapt=False)
    assert samples.shape == (3, 10, 3) and rates.shape == (3,)
    last = [getattr(o, a) for o, a in gp.trainable_parameters()]
    assert np.allclose(last, samples[0, -1], rtol=0, atol=1e-12)
    assert np.ptp(samples, axis=1).max() > 0                    # (the chains move)
    for c, seed in enumerate(seeds):
        one, rate = hmc(model(), n_samples=10, n_burnin=5, step_size=0.02, n_leapfrogs=5, seed=seed, adapt=False)
        assert np.max(np.abs(one - samples[c])) <= 1e-6, (c, np.max(np.abs(one - samples[c])))
        assert abs(rate - rates[c]) < 1e-12
