"""GPU tests of per-observation noise variances on the fused path (pgps_gp_ll_het_*, pgps_gp_predict_het_*,
pgps_gp_ll_grad_adj_het_*): y_k = f(t_k) + e_k, e_k ~ N(0, R + s_k).  ctypes -> C ABI.  References
(het_refs.py; neither is the code under test): a numpy Kalman filter + RTS smoother with a per-step R at the project's 1e-9
(max norm relative to the largest entry), and dense conditioning with K + diag(R + s) at kernel_zoo's tolerance against the
dense GP (1e-6).  Shapes: N in {1, 2, 37, 300} on the default geometry, 700 with one step per lane (three workgroups, a ragged
tail, every wave of the block scan, the spine fold) and with three (a chunk that is no whole sub-tile); 20 % of y missing, s
log-uniform over two decades.  The LDS-staged road, eight steps per lane and the forgetting shortcut:
test_gpu_fused_geometries.py."""
import ctypes
import functools

import numpy as np
import pytest

from het_refs import MATERNS, R, dense_het, matern, queries, rel, sde_of, series, ss_het
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-9
KNAMES = ("m12", "m32", "m52")
# (N, steps per lane or 0 = the default geometry, a run of missing rows (first, length) or None): 252..260 straddles the first
# workgroup boundary of the one-step-per-lane geometry (256 lanes per workgroup)
GEOMS = [(1, 0, None), (2, 0, None), (37, 0, None), (300, 0, None), (700, 1, (252, 9)), (700, 3, None)]
GEOM_IDS = ["N1", "N2", "N37", "N300", "N700-chunk1-straddle", "N700-chunk3"]


class _Chunk:
    """pgps_set_chunk for the block, restored on every exit."""

    def __init__(self, steps):
        from pssgp import _backend as Bk
        self.ctx, self.steps = Bk.get_context(), steps

    def __enter__(self):
        self.ctx.set_chunk(self.steps)

    def __exit__(self, *exc):
        self.ctx.set_chunk(0)


def _form(kname):
    from pssgp import _backend as Bk
    sde = sde_of(kname)
    return Bk.nilpotent_form(sde.F), np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1)


@functools.lru_cache(maxsize=None)
def _case(n, run, k):
    t, y, s = series(n, run=run)
    tq = queries(t, k)
    for a in (t, y, s, tq):
        a.setflags(write=False)
    return t, y, s, tq


@functools.lru_cache(maxsize=None)
def _refs(kname, n, run, k):
    """(state-space reference, dense reference) of a case: (ll, mean, var) each.  Computed once, shared by the tests."""
    t, y, s, tq = _case(n, run, k)
    return ss_het(sde_of(kname), t, y, R, s, tq), dense_het(MATERNS[kname][1], t, y, R, s, tq)


def _check(got, kname, n, run, k, what):
    ref_ss, ref_d = _refs(kname, n, run, k)
    tol = MATERNS[kname][2]
    e = [abs(got[0] - ref_ss[0]) / abs(ref_ss[0])] + [rel(a, b) for a, b in zip(got[1:], ref_ss[1:])]
    print(f"{what}: against the state-space reference " + " ".join(f"{x:.2e}" for x in e))
    assert max(e) <= TOL, (what, e)
    for a, b in zip(got, ref_d):
        np.testing.assert_allclose(a, b, atol=tol, rtol=tol)


@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_ll_and_predict_against_both_references(kname, geom):
    from pssgp import _backend as Bk
    n, chunk, run = geom
    form, P, H = _form(kname)
    for k in (1, 50):
        t, y, s, tq = _case(n, run, k)
        if run is not None:
            assert np.all(np.isnan(y[run[0]:run[0] + run[1]]))
        if k == 50 and n >= 37:
            assert tq[0] < t[0] and tq[-1] > t[-1] and np.intersect1d(tq, t).size >= 5
        with _Chunk(chunk):
            ll = Bk.gp_ll_het(form, P, H, R, t, y, s)
            mean, var, ll_p = Bk.gp_predict_het(form, P, H, R, t, y, s, tq)
        assert mean.shape == (k,) and var.shape == (k,)
        _check((ll_p, mean, var), kname, n, run, k, f"{kname} N {n} chunk {chunk} K {k} predict")
        ref_ll = _refs(kname, n, run, k)[0][0]
        assert abs(ll - ref_ll) <= TOL * abs(ref_ll), (ll, ref_ll)


@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("n,chunk", [(300, 0), (700, 1)])
def test_a_ramp_of_s_sees_a_shifted_index(kname, n, chunk):
    """s strictly increasing over two decades: reading rs[k - 1] or rs[k + 1] for rs[k] moves every result.  The dense
    reference at s shifted by one row differs from the reference at s by far more than the tolerance (asserted), so the
    comparison can tell."""
    from pssgp import _backend as Bk
    form, P, H = _form(kname)
    _, spec, tol = MATERNS[kname]
    t, y, _, tq = _case(n, None, 50)
    s = R * np.logspace(-2.0, 0.0, n)
    ref = dense_het(spec, t, y, R, s, tq)
    shifted = dense_het(spec, t, y, R, np.roll(s, 1), tq)
    assert abs(shifted[0] - ref[0]) > 50.0 * tol * (1.0 + abs(ref[0]))        # (50 times what assert_allclose lets through)
    with _Chunk(chunk):
        ll = Bk.gp_ll_het(form, P, H, R, t, y, s)
        mean, var, ll_p = Bk.gp_predict_het(form, P, H, R, t, y, s, tq)
        grad_ll = Bk.gp_ll_grad_adj_het(form, P, H, R, t, y, s)[0]
    for got in (ll, ll_p, grad_ll):
        np.testing.assert_allclose(got, ref[0], atol=tol, rtol=tol)
    np.testing.assert_allclose(mean, ref[1], atol=tol, rtol=tol)
    np.testing.assert_allclose(var, ref[2], atol=tol, rtol=tol)
    ss = ss_het(sde_of(kname), t, y, R, s, tq)
    assert abs(ll - ss[0]) <= TOL * abs(ss[0]) and rel(mean, ss[1]) <= TOL and rel(var, ss[2]) <= TOL


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


_L, _I, _F = ctypes.c_long, ctypes.c_int, ctypes.c_double


def _scalar_namesakes(kname, t, y, tq, Rc):
    """ll (pgps_gp_dev_f64 with only ll asked for), mean / var / ll (pgps_gp_predict_f64) and the adjoint statistics
    (pgps_gp_ll_grad_adj_dev_f64) of the scalar-noise entry points at noise variance Rc: existing code, not the code under test."""
    from pssgp import _backend as Bk
    form, P, H = _form(kname)
    ll = float(Bk.gp(form, P, H, Rc, t, y)["ll"])
    mean, var, ll_p = Bk.gp_predict(form, P, H, Rc, t, y, tq)
    ctx = Bk.get_context()
    lam, N1, N2 = form
    d = P.shape[0]
    N1, N2 = (np.ascontiguousarray(a, np.float64) for a in (N1, N2))
    out = np.full(1 + d * d + 2 * d + 1, np.nan)
    dev = {"t": ctx.malloc(t.nbytes), "y": ctx.malloc(y.nbytes), "out": ctx.malloc(out.nbytes)}
    try:
        ctx.h2d(dev["t"], np.ascontiguousarray(t)), ctx.h2d(dev["y"], np.ascontiguousarray(y))
        rc = ctx.lib.pgps_gp_ll_grad_adj_dev_f64(ctx.handle, _L(t.size), _I(d), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _F(Rc),
                                                 ctypes.c_void_p(dev["t"]), _F(0.0), ctypes.c_void_p(dev["y"]),
                                                 ctypes.c_void_p(dev["out"]))
        assert rc == 0
        ctx.synchronize()
        ctx.d2h(out, dev["out"])
    finally:
        for ptr in dev.values():
            ctx.free(ptr)
    return ll, (mean, var, ll_p), Bk.split_grad_stats(out, d)


@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("n,chunk", [(37, 0), (300, 0), (700, 1)])
def test_constant_s_equals_the_scalar_entry_points(kname, n, chunk):
    from pssgp import _backend as Bk
    form, P, H = _form(kname)
    t, y, _, tq = _case(n, None, 50)
    c = 0.037
    s = np.full(n, c)
    with _Chunk(chunk):
        ll = Bk.gp_ll_het(form, P, H, R, t, y, s)
        mean, var, ll_p = Bk.gp_predict_het(form, P, H, R, t, y, s, tq)
        stats = Bk.gp_ll_grad_adj_het(form, P, H, R, t, y, s)
        w_ll, (w_mean, w_var, w_llp), w_stats = _scalar_namesakes(kname, t, y, tq, R + c)
    e = [abs(ll - w_ll) / abs(w_ll), abs(ll_p - w_llp) / abs(w_llp), rel(mean, w_mean), rel(var, w_var),
         abs(stats[0] - w_stats[0]) / abs(w_stats[0])] + [rel(a, b) for a, b in zip(stats[1:], w_stats[1:])]
    print(f"{kname} N {n} chunk {chunk}: constant s against R + c, [ll ll_p mean var | ll Abar Ubar Hbar Rbar] "
          + " ".join(f"{x:.2e}" for x in e))
    assert max(e) <= TOL, e


# ---- the gradient with non-constant s, through the model ---------------------------------------------------------------
def _dense_grad(kname, t, y, Rv, s):
    """d ll / d (variance, lengthscale, noise_variance) of the dense GP with C = K + diag(Rv + s): 1/2 (a^T dC a - tr(C^-1 dC)),
    a = C^-1 y, dC / d theta by Richardson-extrapolated central differences of O.dense_K (relative steps 1e-3 and 5e-4: K is
    analytic in both parameters at every r, the truncation error is O(h^4)), dC / d noise_variance = I."""
    name, var, ell = MATERNS[kname][1]
    o = ~np.isnan(y)
    to, yo = t[o], y[o]
    C = O.dense_K((name, var, ell), to, to) + np.diag(Rv + s[o])
    Ci = np.linalg.inv(C)
    a = Ci @ yo

    def dK(i):
        def central(h):
            up, dn = [var, ell], [var, ell]
            up[i] += h
            dn[i] -= h
            return (O.dense_K((name, up[0], up[1]), to, to) - O.dense_K((name, dn[0], dn[1]), to, to)) / (2.0 * h)
        h = 1e-3 * (var, ell)[i]
        return (4.0 * central(0.5 * h) - central(h)) / 3.0

    return np.array([0.5 * (a @ dC @ a - np.sum(Ci * dC)) for dC in (dK(0), dK(1), np.eye(to.size))])


def _grad_err(g, ref):
    """Every component against the reference's, relative to its own size -- but to no less than 1e-3 of the gradient's largest
    component: the reference's own error (differences of K, a dense inverse) scales with the largest one."""
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(g - ref) / np.maximum(np.abs(ref), 1e-3 * np.max(np.abs(ref)))))


# The floor of the dense reference gradient, measured on an MI355X on the scalar-noise model (s = None) against the existing
# device gradient (correct to 1e-9 by tests/test_gpu_adjoint.py), N = 300, _grad_err; the per-observation case is held to
# 10 x that floor (the margin covers the worse conditioning of C when s spans two decades).
GRAD_FLOOR = {"m12": 1.331e-11, "m32": 3.402e-12, "m52": 3.393e-12}


@pytest.mark.parametrize("kname", KNAMES)
def test_model_gradient_against_the_dense_analytic_gradient(kname):
    """N = 300.  Measured on an MI355X (_grad_err): the floor -- s = None, the existing device gradient against the dense
    reference -- is 1.331e-11 (Matern-1/2), 3.402e-12 (-3/2), 3.393e-12 (-5/2), so the bounds (10 x floor) are 1.331e-10, 3.402e-11,
    3.393e-11; the per-observation gradient measured 1.170e-11, 9.503e-12, 1.049e-11.  The floor is measured again and printed
    by every run; it is the reference's error, not the code's, and is held to the same bound."""
    from pssgp.model import StateSpaceGP
    n = 300
    t, y, s, _ = _case(n, None, 50)
    plain = StateSpaceGP((t[:, None], y[:, None]), matern(kname), noise_variance=R, parallel=True)
    plain.maximum_log_likelihood_objective()        # (the fused adjoint pass runs on the resident series: from the second evaluation)
    ll0, g0 = plain.log_likelihood_and_grad(method="adjoint")
    floor = _grad_err(g0, _dense_grad(kname, t, y, R, np.zeros(n)))
    m = StateSpaceGP((t[:, None], y[:, None]), matern(kname), noise_variance=R, parallel=True, observation_variances=s)
    ll, g = m.log_likelihood_and_grad()
    ref = _dense_grad(kname, t, y, R, s)
    err = _grad_err(g, ref)
    print(f"{kname}: floor (s = None) {floor:.3e}, per-observation error {err:.3e}, gradient {g}, reference {ref}")
    assert floor <= 10.0 * GRAD_FLOOR[kname], (floor, GRAD_FLOOR[kname])
    assert err <= 10.0 * GRAD_FLOOR[kname], (err, GRAD_FLOOR[kname])
    ll_d = dense_het(MATERNS[kname][1], t, y, R, s)
    assert abs(float(ll) - ll_d) <= MATERNS[kname][2] * abs(ll_d)
    g_adj = m.log_likelihood_and_grad(method="adjoint")[1]
    assert np.array_equal(g, g_adj)
    g_wrt = m.log_likelihood_and_grad(wrt=[2])[1]
    assert g_wrt[0] == 0.0 and g_wrt[1] == 0.0 and g_wrt[2] == g[2]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _all_three(kname, t, y, s, tq):
    from pssgp import _backend as Bk
    form, P, H = _form(kname)
    ll = Bk.gp_ll_het(form, P, H, R, t, y, s)
    mean, var, ll_p = Bk.gp_predict_het(form, P, H, R, t, y, s, tq)
    stats = Bk.gp_ll_grad_adj_het(form, P, H, R, t, y, s)
    return [np.asarray(ll), mean, var, np.asarray(ll_p)] + [np.asarray(a) for a in stats]


@pytest.mark.parametrize("kname", KNAMES)
def test_nan_at_missing_steps_and_repeatability(kname):
    t, y, s, tq = _case(700, (252, 9), 50)
    with _Chunk(1):
        first = _all_three(kname, t, y, s, tq)
        again = _all_three(kname, t, y, s, tq)
        s_nan = np.where(np.isnan(y), np.nan, s)
        assert np.isnan(s_nan).sum() > 100
        with_nan = _all_three(kname, t, y, s_nan, tq)
    for a, b, c in zip(first, again, with_nan):
        assert np.all(np.isfinite(a))
        assert np.array_equal(_bits(a), _bits(b)), "two calls differ"
        assert np.array_equal(_bits(a), _bits(c)), "s at a missing step reached the arithmetic"


def test_abi_errors_and_the_dev_entries():
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    lib = ctx.lib
    kname, n, k, d = "m32", 300, 50, 2
    form, P, H = _form(kname)
    lam, N1, N2 = form
    N1, N2 = (np.ascontiguousarray(a, np.float64) for a in (N1, N2))
    t, y, s, tq = (np.array(a) for a in _case(n, None, k))
    nout = 1 + d * d + 2 * d + 1
    ll, ll2 = ctypes.c_double(0.0), ctypes.c_double(0.0)
    llp, llp2 = ctypes.cast(ctypes.byref(ll), ctypes.c_void_p), ctypes.cast(ctypes.byref(ll2), ctypes.c_void_p)
    mean, var, out = np.full(k, np.nan), np.full(k, np.nan), np.full(nout, np.nan)

    def calls(dim=d, r=R, rs=s):
        rp = None if rs is None else _p(rs)
        return (lib.pgps_gp_ll_het_f64(ctx.handle, _L(n), _I(dim), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _F(r), _p(t), _p(y), rp, _F(0.0), llp),
                lib.pgps_gp_predict_het_f64(ctx.handle, _L(n), _L(k), _I(dim), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _F(r), _p(t), _p(y), rp, _F(0.0),
                                            _p(tq), _p(mean), _p(var), llp2),
                lib.pgps_gp_ll_grad_adj_het_f64(ctx.handle, _L(n), _I(dim), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _F(r), _p(t), _F(0.0), _p(y), rp,
                                                _p(out)))

    seen = np.flatnonzero(~np.isnan(y))
    neg, zero, inf = s.copy(), s.copy(), s.copy()
    neg[seen[3]] = -1e-3
    zero[seen[7]] = 0.0
    inf[seen[5]] = np.inf
    assert calls(rs=None) == (-1, -1, -1)           # PGPS_E_INVALID: null rs
    assert calls(rs=neg) == (-1, -1, -1)            # a negative s_k at an observed row
    assert calls(rs=inf) == (-1, -1, -1)            # a non-finite one
    assert calls(r=0.0, rs=zero) == (-1, -1, -1)    # R = 0 with some s_k = 0
    assert calls(r=-0.01) == (-1, -1, -1)
    assert calls(dim=4) == (-2, -2, -2)             # PGPS_E_UNSUPPORTED_DIM
    # R = 0 with every s_k > 0 is a model: accepted, and right
    assert calls(r=0.0) == (0, 0, 0)
    _, spec, tol = MATERNS[kname]
    ref = dense_het(spec, t, y, 0.0, s, tq)
    for got_ll in (ll.value, ll2.value, out[0]):
        np.testing.assert_allclose(got_ll, ref[0], atol=tol, rtol=tol)
    np.testing.assert_allclose(mean, ref[1], atol=tol, rtol=tol)
    np.testing.assert_allclose(var, ref[2], atol=tol, rtol=tol)
    ss = ss_het(sde_of(kname), t, y, 0.0, s, tq)
    assert abs(ll.value - ss[0]) <= TOL * abs(ss[0]) and rel(mean, ss[1]) <= TOL and rel(var, ss[2]) <= TOL
    # a valid call on the same context after the refused ones; the _dev forms on device pointers give the same bits
    assert calls() == (0, 0, 0)
    host = [np.array([ll.value, 0.0]), mean.copy(), var.copy(), out.copy(), np.array([ll2.value, 0.0])]
    names = {"t": t, "y": y, "s": s, "tq": tq, "mean": mean, "var": var, "out": out, "ll": np.zeros(2), "ll_p": np.zeros(2)}
    dev = {key: ctx.malloc(a.nbytes) for key, a in names.items()}
    D = {key: ctypes.c_void_p(ptr) for key, ptr in dev.items()}
    try:
        for key in ("t", "y", "s", "tq"):
            ctx.h2d(dev[key], names[key])
        rc = (lib.pgps_gp_ll_het_dev_f64(ctx.handle, _L(n), _I(d), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _F(R), D["t"], D["y"], D["s"], _F(0.0), D["ll"]),
              lib.pgps_gp_predict_het_dev_f64(ctx.handle, _L(n), _L(k), _I(d), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _F(R), D["t"], D["y"], D["s"], _F(0.0),
                                              D["tq"], D["mean"], D["var"], D["ll_p"]),
              lib.pgps_gp_ll_grad_adj_het_dev_f64(ctx.handle, _L(n), _I(d), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _F(R), D["t"], _F(0.0), D["y"], D["s"],
                                                  D["out"]))
        assert rc == (0, 0, 0)
        ctx.synchronize()
        got = {key: np.full(names[key].shape, np.nan) for key in ("ll", "mean", "var", "out", "ll_p")}
        for key, a in got.items():
            ctx.d2h(a, dev[key])
        assert lib.pgps_gp_ll_het_dev_f64(ctx.handle, _L(n), _I(d), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _F(R), D["t"], D["y"], None, _F(0.0),
                                          D["ll"]) == -1
    finally:
        for ptr in dev.values():
            ctx.free(ptr)
    for a, b in zip((got["ll"][:1], got["mean"], got["var"], got["out"], got["ll_p"][:1]), (host[0][:1],) + tuple(host[1:4]) + (host[4][:1],)):
        assert np.array_equal(_bits(a), _bits(b)), "a device-pointer entry differs from its host-array entry"


# ---- model routing ------------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    from pssgp import _backend as Bk
    calls = {"gp_ll_het": 0, "gp_predict_het": 0, "gp_ll_grad_adj_het": 0, "Series": 0}

    def wrap(name):
        real = getattr(Bk, name)

        def spy(*args, **kwargs):
            calls[name] += 1
            return real(*args, **kwargs)
        monkeypatch.setattr(Bk, name, spy)

    for name in calls:
        wrap(name)
    return calls


def test_a_matern_model_takes_the_device_route_and_no_resident_series(monkeypatch):
    from pssgp.model import StateSpaceGP
    calls = _spy(monkeypatch)
    kname, n, k = "m32", 300, 50
    t, y, s, tq = _case(n, None, k)
    m = StateSpaceGP((t[:, None], y[:, None]), matern(kname), noise_variance=R, parallel=True, observation_variances=s)
    want = dict(calls)
    for _ in range(3):                              # (a scalar model makes its series resident at its second evaluation)
        ll = float(m.maximum_log_likelihood_objective())
        want["gp_ll_het"] += 1
        assert calls == want
        mean, var = m.predict_f(tq[:, None])
        want["gp_predict_het"] += 1
        assert calls == want
        ll_g, g = m.log_likelihood_and_grad()
        want["gp_ll_grad_adj_het"] += 1
        assert calls == want
    assert calls["Series"] == 0 and not getattr(m, "_series", None)
    _check((ll, mean[:, 0], var[:, 0]), kname, n, None, k, "model, device route")
    assert abs(float(ll_g) - ll) <= 1e-12 * abs(ll) and g.shape == (3,)
    # None assigned later: today's behaviour, evaluation by evaluation, the resident series included
    back = StateSpaceGP((t[:, None], y[:, None]), matern(kname), noise_variance=R, parallel=True, observation_variances=s)
    back.observation_variances = None
    plain = StateSpaceGP((t[:, None], y[:, None]), matern(kname), noise_variance=R, parallel=True)
    for _ in range(2):
        a, b = back.maximum_log_likelihood_objective(), plain.maximum_log_likelihood_objective()
        assert np.array_equal(_bits(a), _bits(b))
        for u, v in zip(back.predict_f(tq[:, None]), plain.predict_f(tq[:, None])):
            assert np.array_equal(_bits(u), _bits(v))
    assert calls == {**want, "Series": 2}


def test_an_rbf_model_takes_the_host_twin(monkeypatch):
    from pssgp.kernels import RBF
    from pssgp.model import StateSpaceGP
    calls = _spy(monkeypatch)
    n, k = 200, 50
    t, y, s, tq = _case(n, None, k)
    kern = RBF(variance=1., lengthscales=0.5, order=4, balancing_iter=5)
    m = StateSpaceGP((t[:, None], y[:, None]), kern, noise_variance=R, parallel=True, observation_variances=s)
    for _ in range(2):
        ll = float(m.maximum_log_likelihood_objective())
        mean, var = m.predict_f(tq[:, None])
    assert all(v == 0 for v in calls.values()), calls
    ll_r, mean_r, var_r = ss_het(kern.get_sde(), t, y, R, s, tq)
    e = (abs(ll - ll_r) / abs(ll_r), rel(mean[:, 0], mean_r), rel(var[:, 0], var_r))
    print(f"rbf4 on the host twin: ll {e[0]:.2e} mean {e[1]:.2e} var {e[2]:.2e}")
    assert max(e) <= TOL, e
    with pytest.raises(NotImplementedError, match="observation_variances"):
        m.log_likelihood_and_grad()
