"""GPU parity of the functionals of the state (pgps_lti_predict_lin_*: C sm and C sP C^T at the query rows of the general-LTI
chain -- the functionals flavour of the row-cooperative projecting smoother up to d = 16, k_project_rows_lin behind the
wave-cooperative smoother from 17 to 32) against the sequential oracle on the merged series, and of StateSpaceGP's
predict_components / predict_f_derivative / predict_functionals on the device route.

Tolerances are those of tests/test_gpu_lti.py for the same chain: 1e-7 max(1, max |ref|) on mean and cov (2e-6 for RBF of
order >= 15, for the reason written there), 1e-8 relative on the log-likelihood."""
import ctypes
import functools

import numpy as np
import pytest

from tests import functional_refs as R

pytestmark = pytest.mark.gpu

NOISE = 0.1


def _rows(name, sde, kernel):
    """The functionals each kernel is tested with."""
    comps = kernel.component_functionals()[1]
    P = R.powers_of_F(sde, 2)
    return {"m32": P[:2], "m52": P[:3], "m32+m52": np.vstack([comps, P[1]]), "c5_qp_m52": comps, "rbf15": P[:3], "rbf16": P[:3],
            "co2_d18": np.vstack([comps, P[1]]), "periodic10": P[:2]}[name]


def _tol(name):
    return 2e-6 if name in ("rbf15", "rbf16") else 1e-7


@functools.lru_cache(maxsize=None)
def _road_case(name):
    """(sde, C, t, y, tq, oracle mean, cov, ll) of the kernels x roads case: N = 1700 with every 7th y missing, K = 400 queries
    reaching 0.5 beyond both ends -- 2100 merged steps, at chain length 8 that is 65 full workgroups and a ragged last one."""
    kernel = R.kernels()[name]()
    sde = kernel.get_sde()
    C = np.ascontiguousarray(_rows(name, sde, kernel))
    t, y = R.series(1700, 3)
    y[::7] = np.nan
    tq = np.sort(np.random.default_rng(5).uniform(t[0] - 0.5, t[-1] + 0.5, 400))
    return (sde, C, t, y, tq) + R.oracle_lin(sde, C, NOISE, t, y, tq)


def _check(got, want, tol, what):
    mean, cov, ll = got
    mean_o, cov_o, ll_o = want
    assert mean.shape == mean_o.shape and cov.shape == cov_o.shape
    R.assert_close(mean, mean_o, tol, f"{what}: mean")
    R.assert_close(cov, cov_o, tol, f"{what}: cov")
    assert abs(ll - ll_o) < 1e-8 * abs(ll_o), (what, ll, ll_o)
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2)), f"{what}: a (J, J) block is not symmetric bit for bit"


@pytest.mark.parametrize("name", ["m32", "m52", "m32+m52", "c5_qp_m52", "rbf15", "rbf16", "co2_d18", "periodic10"])
def test_functionals_vs_oracle_on_every_road(name):
    from pssgp import _backend as B
    sde, C, t, y, tq, mean_o, cov_o, ll_o = _road_case(name)
    got = B.lti_predict_lin(sde.F, sde.P0, sde.H, C, NOISE, t, y, tq)
    _check(got, (mean_o, cov_o, ll_o), _tol(name), name)
    again = B.lti_predict_lin(sde.F, sde.P0, sde.H, C, NOISE, t, y, tq)
    assert all(np.array_equal(a, b) for a, b in zip(got[:2], again[:2])) and got[2] == again[2], "a repeated call differs"


@pytest.mark.parametrize("name", ["m32+m52", "c5_qp_m52"])
@pytest.mark.parametrize("n,k,chunk", [(20, 6, 0), (1700, 348, 0), (4000, 1003, 64)])
def test_functionals_geometries(name, n, k, chunk):
    """N + K = 26: one workgroup, chains partly empty; 2048: a full last workgroup; 5003 after pgps_set_chunk(64): long chains,
    several scan levels, a ragged tail."""
    from pssgp import _backend as B
    kernel = R.kernels()[name]()
    sde = kernel.get_sde()
    C = np.vstack([kernel.component_functionals()[1], R.powers_of_F(sde, 1)[1]])
    t, y = R.series(n, 11)
    y[::5] = np.nan
    tq = np.sort(np.random.default_rng(13).uniform(t[0] - 0.2, t[-1] + 0.2, k))
    want = R.oracle_lin(sde, C, NOISE, t, y, tq)
    ctx = B.get_context()
    try:
        if chunk:
            ctx.set_chunk(chunk)
        got = B.lti_predict_lin(sde.F, sde.P0, sde.H, C, NOISE, t, y, tq)
    finally:
        ctx.set_chunk(0)
    _check(got, want, 1e-7, f"{name} N + K = {n + k}, chunk {chunk}")


def test_functionals_large_series_vs_c_oracle():
    """m32+m52 at 2^15 + 2^13 merged steps against the sequential C oracle run on the merged series."""
    from pssgp import _backend as B
    kernel = R.kernels()["m32+m52"]()
    sde = kernel.get_sde()
    C = np.vstack([kernel.component_functionals()[1], R.powers_of_F(sde, 1)[1]])
    t, y = R.series(1 << 15, 21)
    tq = np.sort(np.random.default_rng(2).uniform(t[0], t[-1], 1 << 13))
    got = B.lti_predict_lin(sde.F, sde.P0, sde.H, C, NOISE, t, y, tq)
    _check(got, R.oracle_lin(sde, C, NOISE, t, y, tq), 1e-7, "2^15 + 2^13 steps")


@pytest.mark.parametrize("name", ["m32", "m32+m52", "rbf16", "co2_d18"])
def test_one_functional_H_equals_lti_predict(name):
    """J = 1, C = H: the same chain with the same chain length as pgps_lti_predict_*, another order of the last sums."""
    from pssgp import _backend as B
    sde, _, t, y, tq = _road_case(name)[:5]
    H = np.asarray(sde.H, np.float64).reshape(1, -1)
    mean, cov, ll = B.lti_predict_lin(sde.F, sde.P0, sde.H, H, NOISE, t, y, tq)
    mean_p, var_p, ll_p = B.lti_predict(sde.F, sde.P0, sde.H, NOISE, t, y, tq)
    assert mean.shape == (400, 1) and cov.shape == (400, 1, 1)
    err_m, err_v = float(np.max(np.abs(mean[:, 0] - mean_p))), float(np.max(np.abs(cov[:, 0, 0] - var_p)))
    print(f"{name}: mean {err_m:.2e} of {np.max(np.abs(mean_p)):.2e}, var {err_v:.2e} of {np.max(np.abs(var_p)):.2e}")
    assert err_m <= 1e-12 * float(np.max(np.abs(mean_p)))
    assert err_v <= 1e-12 * float(np.max(np.abs(var_p)))
    assert abs(ll - ll_p) <= 1e-12 * abs(ll_p)              # (the filter passes are the same launches)


@pytest.mark.parametrize("name", ["m32", "rbf16"])
def test_eight_random_functionals(name):
    """J = PGPS_MAX_FUNCTIONALS with a fixed-seed random C at d = 2 (the (8, 8) blocks have rank 2) and d = 16."""
    from pssgp import _backend as B
    sde, _, t, y, tq = _road_case(name)[:5]
    d = np.asarray(sde.F).shape[0]
    C = np.random.default_rng(17).standard_normal((8, d))
    got = B.lti_predict_lin(sde.F, sde.P0, sde.H, C, NOISE, t, y, tq)
    _check(got, R.oracle_lin(sde, C, NOISE, t, y, tq), _tol(name), f"{name}, J = 8")
    again = B.lti_predict_lin(sde.F, sde.P0, sde.H, C, NOISE, t, y, tq)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])


def test_invalid_numbers_of_functionals():
    from pssgp import _backend as B
    from pssgp._backend import _ptr
    sde, _, t, y, tq = _road_case("m32+m52")[:5]
    F, P, H = (np.ascontiguousarray(a, np.float64) for a in (sde.F, sde.P0, np.asarray(sde.H).reshape(-1)))
    t, y, tq = (np.ascontiguousarray(a[:50]) for a in (t, y, tq))
    C = np.zeros((9, 5))
    mean, cov = np.zeros(50 * 9), np.zeros(50 * 81)
    ctx = B.get_context()

    def code(J, c):
        with ctx.lock:
            return ctx.lib.pgps_lti_predict_lin_f64(ctx.handle, 50, 50, 5, J, _ptr(F), _ptr(P), _ptr(H), c, NOISE, _ptr(t), _ptr(y),
                                                    0.0, _ptr(tq), _ptr(mean), _ptr(cov), None)

    invalid = -1                                            # PGPS_E_INVALID
    assert ctx.lib.pgps_strerror(invalid).decode().lower().find("invalid") >= 0
    assert code(0, _ptr(C)) == invalid and code(9, _ptr(C)) == invalid and code(2, None) == invalid
    assert code(8, _ptr(C)) == B.PGPS_OK


def test_device_pointer_entry_point_equals_the_host_one():
    from pssgp import _backend as B
    from pssgp._backend import _ptr
    c_long, c_int, c_double, c_void_p = ctypes.c_long, ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    for name in ("m32+m52", "co2_d18"):
        sde, C, t, y, tq = _road_case(name)[:5]
        F, P, H = (np.ascontiguousarray(a, np.float64) for a in (sde.F, sde.P0, np.asarray(sde.H).reshape(-1)))
        d, J, N, K = F.shape[0], C.shape[0], t.shape[0], tq.shape[0]
        want = B.lti_predict_lin(F, P, H, C, NOISE, t, y, tq)
        mean, cov, ll = np.empty((K, J)), np.empty((K, J, J)), np.empty(1)
        ctx = B.Context(0)
        bufs = []
        try:
            for a in (t, y, tq, mean, cov, ll):
                bufs.append(ctx.malloc(a.nbytes))
            for p, a in zip(bufs[:3], (t, y, tq)):
                ctx.h2d(p, np.ascontiguousarray(a))
            ctx.call("pgps_lti_predict_lin_dev_f64", c_long(N), c_long(K), c_int(d), c_int(J), _ptr(F), _ptr(P), _ptr(H), _ptr(C),
                     c_double(NOISE), c_void_p(bufs[0]), c_void_p(bufs[1]), c_double(0.0), c_void_p(bufs[2]), c_void_p(bufs[3]),
                     c_void_p(bufs[4]), c_void_p(bufs[5]))
            for a, p in zip((mean, cov, ll), bufs[3:]):
                ctx.d2h(a, p)
        finally:
            try:
                for p in bufs:
                    ctx.free(p)
            finally:
                ctx.close()
        assert np.array_equal(mean, want[0]) and np.array_equal(cov, want[1]) and ll[0] == want[2]


def test_functionals_ties_follow_merge_sorted():
    """The query set of test_lti_predict_ties_follow_merge_sorted: queries equal to training times, repeated queries, more
    queries than training points, queries before the first and after the last observation; 1e-8 as there.
    The two component rows only: the query one time unit before the first observation sits behind a long first step, where
    the oracle's matrix-fraction Q is 2.3e-8 off Pinf - F Pinf F^T -- the oracle run with either Q differs from itself by 4e-9
    in the components' block but by 2.5e-7 in the variance of H F x (18.7 there), which no 1e-8 can be asked of."""
    from pssgp import _backend as B
    kernel = R.kernels()["m32+m52"]()
    sde = kernel.get_sde()
    C = kernel.component_functionals()[1]
    t, y = R.series(60, 8)
    tq = np.sort(np.concatenate([t[::3], t[::3], [t[0] - 1.0, t[-1] + 2.0], np.linspace(t[0], t[-1], 150)]))
    mean, cov, _ = B.lti_predict_lin(sde.F, sde.P0, sde.H, C, 0.2, t, y, tq)
    mean_o, cov_o, _ = R.oracle_lin(sde, C, 0.2, t, y, tq)
    assert np.max(np.abs(mean - mean_o)) < 1e-8 and np.max(np.abs(cov - cov_o)) < 1e-8
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))


# -- model level -------------------------------------------------------------------------------------------------------------
def _model(name, parallel=True, n=900, seed=31):
    from pssgp.model import StateSpaceGP
    t, y = R.series(n, seed)
    return StateSpaceGP((t[:, None], y[:, None]), R.kernels()[name](), noise_variance=NOISE, parallel=parallel), t


@pytest.mark.parametrize("name", ["m32+m52", "co2_d18"])
def test_components_add_up_to_predict_f(name):
    m, t = _model(name)
    tq = np.sort(np.random.default_rng(1).uniform(t[0], t[-1], 120))[:, None]
    mean, cov = m.predict_components(tq, cross_cov=True)
    mean2, var = m.predict_components(tq)
    pm, pv = m.predict_f(tq)
    J = len(m.component_names())
    assert J == 2 and mean.shape == (120, J) and cov.shape == (120, J, J) and var.shape == (120, J)
    assert np.max(np.abs(mean.sum(axis=1) - pm[:, 0])) < 1e-9 * max(1.0, float(np.max(np.abs(pm))))
    assert np.max(np.abs(cov.sum(axis=(1, 2)) - pv[:, 0])) < 1e-9 * max(1.0, float(np.max(np.abs(pv))))
    assert np.array_equal(mean2, mean) and np.array_equal(var, np.diagonal(cov, axis1=1, axis2=2))


def test_the_device_call_is_taken_in_parallel_mode_only(monkeypatch):
    from pssgp import _backend as B
    calls = []
    real = B.lti_predict_lin
    monkeypatch.setattr(B, "lti_predict_lin", lambda *a, **k: calls.append("lin") or real(*a, **k))
    tq = np.linspace(0.5, 5.0, 40)[:, None]
    m, _ = _model("m32+m52", n=300)
    got = m.predict_components(tq, cross_cov=True)
    assert calls == ["lin"]
    d1 = m.predict_f_derivative(tq)
    assert calls == ["lin", "lin"]
    h, _ = _model("m32+m52", parallel=False, n=300)
    want = h.predict_components(tq, cross_cov=True)
    d1_h = h.predict_f_derivative(tq)
    assert calls == ["lin", "lin"]
    for a, b in zip(got + d1, want + d1_h):                 # the device route against the host twin
        R.assert_close(a, b, 1e-8, "device route vs host twin")


def test_shuffled_repeated_queries_give_the_rows_of_the_sorted_call():
    m, t = _model("m32+m52", n=300)
    k = m.kernel
    C = np.vstack([k.component_functionals()[1], k.derivative_functional(1)])
    tq = np.sort(np.random.default_rng(3).uniform(t[0], t[-1], 50))
    mean, cov = m.predict_functionals(tq[:, None], C)
    perm = np.random.default_rng(4).permutation(np.concatenate([np.arange(50), [7, 7, 31]]))
    mean_p, cov_p = m.predict_functionals(tq[perm][:, None], C)
    assert np.array_equal(mean_p, mean[perm]) and np.array_equal(cov_p, cov[perm])


def test_float32_default_float_gives_float32_outputs():
    from pssgp import config
    from pssgp.model import StateSpaceGP
    t, y = R.series(900, 31)
    tq = np.sort(np.random.default_rng(1).uniform(t[0], t[-1], 120))
    kernel = R.kernels()["m32+m52"]()
    m64 = StateSpaceGP((t[:, None], y[:, None]), kernel, noise_variance=NOISE, parallel=True)
    mean64, cov64 = m64.predict_components(tq[:, None], cross_cov=True)
    d64 = m64.predict_f_derivative(tq[:, None])
    old = config.default_float()
    config.set_default_float(np.float32)
    try:
        m = StateSpaceGP((t[:, None].astype(np.float32), y[:, None].astype(np.float32)), R.kernels()["m32+m52"](),
                         noise_variance=NOISE, parallel=True)
        mean, cov = m.predict_components(tq[:, None].astype(np.float32), cross_cov=True)
        d32 = m.predict_f_derivative(tq[:, None].astype(np.float32))
    finally:
        config.set_default_float(old)
    assert all(a.dtype == np.float32 for a in (mean, cov) + d32)
    for a, b in zip((mean, cov) + d32, (mean64, cov64) + d64):
        R.assert_close(a, b, 1e-3, "float32 model vs float64 model")
