"""GPU tests of Laplace inference on the fused path (pgps_gp_newton_*, pgps_lik_sites_*, LaplaceStateSpaceGP(parallel=True);
DESIGN.md section 4y).  ctypes -> C ABI.  References (laplace_refs.py; none is the code under test): a numpy Kalman filter + RTS
smoother over the sites followed by the site update, at the project's 1e-9 (max norm relative to the largest entry), and the
dense Laplace approximation of Rasmussen & Williams at kernel_zoo's tolerance against the dense GP (1e-6).  Shapes of one pass:
those of test_gpu_loo.py -- N in {1, 2, 37, 300} on the default geometry, 700 with one step per lane (three workgroups, a ragged
tail, the spine fold, rows 252..260 missing across a workgroup boundary) and with three (the unstaged path), 300 rows with five
repeated times -- and 6144 rows with eight steps per lane (LDS-staged; 256 x 8 >= 2048 steps per workgroup: the forgetting
shortcut is on)."""
import ctypes
import warnings

import numpy as np
import pytest

import laplace_refs as LR
from laplace_refs import ARRAYS, LIKS, MATERNS, PARS, TOL, err, matern, pass_case, sde_of

pytestmark = pytest.mark.gpu

KNAMES = ("m12", "m32", "m52")
LIKELIHOODS = ("bernoulli", "poisson")
# (N, steps per lane or 0 = the default geometry, a run of missing rows (first, length) or None, repeated times, spaced times)
GEOMS = [(1, 0, None, False, False), (2, 0, None, False, False), (37, 0, None, False, False), (300, 0, None, False, False),
         (700, 1, (252, 9), False, False), (700, 3, None, False, False), (300, 0, None, True, False), (6144, 8, None, False, True)]
GEOM_IDS = ["N1", "N2", "N37", "N300", "N700-chunk1-straddle", "N700-chunk3", "N300-repeated-times", "N6144-chunk8-staged-shortcut"]


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


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _sum_errors(got, want):
    """every sum against the reference's, relative to max(1, |reference|): the terms of the sums are of order one"""
    return [abs(g - w) / max(1.0, abs(w)) for g, w in zip(got, want)]


def _likelihood(lik):
    from pssgp.likelihoods import Bernoulli, Gaussian, Poisson
    return {"gaussian": lambda: Gaussian(PARS["gaussian"]), "bernoulli": Bernoulli, "poisson": lambda: Poisson(PARS["poisson"])}[lik]()


@pytest.mark.parametrize("lik", LIKELIHOODS)
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_one_newton_pass_against_the_state_space_reference(geom, kname, lik):
    from pssgp import _backend as Bk
    n, chunk, run, repeated, spaced = geom
    form, P, H = _form(kname)
    t, y, z, s, f_prev, ref = pass_case(kname, lik, n, run, repeated, spaced)
    nan = np.isnan(y)
    if run is not None:
        assert np.all(nan[run[0]:run[0] + run[1]])
    # the floor of W is inactive at every row of the reference: the sites are the likelihood's own curvature
    assert np.all(1.0 / np.asarray(s)[~nan] > LR.W_MIN) and np.all(1.0 / ref["ss"][~nan] > LR.W_MIN)
    with _Chunk(chunk):
        if chunk == 8:
            assert Bk.get_context().get_chunk(n)[0] == 8
        got = Bk.gp_newton(form, P, H, LIKS[lik], PARS[lik], t, y, z, s, f_prev)
        again = Bk.gp_newton(form, P, H, LIKS[lik], PARS[lik], t, y, z, s, f_prev)
    e = [err(got[a], ref[a]) for a in ARRAYS] + _sum_errors(got["sums"], ref["sums"])
    print(f"{kname} {lik} N {n} chunk {chunk}: " + " ".join(f"{x:.1e}" for x in e))
    assert max(e) <= TOL, e
    # missing rows: no site there, a finite law of f, and the count of the observed rows
    assert np.array_equal(np.isnan(got["zs"]), nan) and np.all(got["ss"][nan] == 1.0) and np.all(got["alpha"][nan] == 0.0)
    assert np.all(np.isfinite(got["f"])) and np.all(np.isfinite(got["v"])) and np.all(got["v"] > 0.0)
    assert got["sums"][5] == float((~nan).sum())
    # two equal calls agree bit for bit in every array and sum
    for a in ARRAYS + ("sums",):
        assert np.array_equal(_bits(got[a]), _bits(again[a])), f"two calls differ in {a}"


@pytest.mark.parametrize("lik", LIKELIHOODS + ("gaussian",))
def test_lik_sites_against_numpy(lik):
    from pssgp import _backend as Bk
    n = 1500                                                    # (six workgroups of the elementwise grid, the last one ragged)
    t, y = LR.case(lik, n)
    nan = np.isnan(y)
    rng = np.random.RandomState(11)
    f_a, f_b = 0.3 * np.sin(t), 0.3 * np.sin(t) + 0.5 * rng.randn(n)
    al_a, al_b = rng.randn(n), rng.randn(n)
    for step, with_b in ((0.0, True), (0.25, True), (1.0, True), (0.0, False)):
        got = Bk.lik_sites(LIKS[lik], PARS[lik], y, f_a, al_a, f_b if with_b else None, al_b if with_b else None, step)
        f = f_a + step * (f_b - f_a) if with_b else f_a
        al = al_a + step * (al_b - al_a) if with_b else al_a
        z, s, _, _ = LR.sites_at(lik, PARS[lik], y, f)
        want = {"f": f, "alpha": al, "zs": z, "ss": s}
        e = [err(got[a], want[a]) for a in want]
        # the sums, relative to the sum of the magnitudes of their terms (they are added in another order than numpy's)
        lp, g, W, _ = LR.lik_derivs(lik, PARS[lik], np.where(nan, 0.0, y), f)
        logn = -0.5 * (LR.LOG2PI - np.log(W) + g * g / W)               # log N(z | f, s)
        terms = (lp[~nan], f * al, (lp - logn)[~nan])
        # (a correction term is a difference of two log densities -- zero for the Gaussian likelihood: its scale is theirs)
        scales = (np.abs(lp[~nan]), np.abs(f * al), (np.abs(lp) + np.abs(logn))[~nan])
        es = [abs(got_sum - float(np.sum(term))) / float(np.sum(scale)) for got_sum, term, scale in zip(got["sums"], terms, scales)]
        print(f"{lik} step {step} f_b {with_b}: " + " ".join(f"{x:.1e}" for x in e + es))
        assert max(e) <= 1e-14 and max(es) <= 1e-14
        assert np.array_equal(np.isnan(got["zs"]), nan) and np.all(got["ss"][nan] == 1.0)
        again = Bk.lik_sites(LIKS[lik], PARS[lik], y, f_a, al_a, f_b if with_b else None, al_b if with_b else None, step)
        for a in got:
            assert np.array_equal(_bits(got[a]), _bits(again[a]))


@pytest.mark.parametrize("kname", KNAMES)
def test_gaussian_likelihood_is_the_gaussian_pass(kname):
    from pssgp import _backend as Bk
    n, var = 300, PARS["gaussian"]
    form, P, H = _form(kname)
    t, y = LR.case("gaussian", n)
    start = Bk.lik_sites(LIKS["gaussian"], var, y, np.zeros(n), np.zeros(n))
    got = Bk.gp_newton(form, P, H, LIKS["gaussian"], var, t, y, start["zs"], start["ss"], np.zeros(n))
    ll_het = Bk.gp_ll_het(form, P, H, 0.0, t, y, np.full(n, var))
    ll = float(Bk.gp(form, P, H, var, t, y)["ll"])
    evidence = got["sums"][0] + got["sums"][3]
    print(f"{kname}: sums[0] against gp_ll_het {abs(got['sums'][0] - ll_het) / abs(ll_het):.1e}, evidence against gp {abs(evidence - ll) / abs(ll):.1e}")
    assert abs(got["sums"][0] - ll_het) <= 1e-12 * abs(ll_het)
    assert abs(evidence - ll) <= 1e-12 * abs(ll)


_L, _I, _F = ctypes.c_long, ctypes.c_int, ctypes.c_double


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_abi_errors_and_the_dev_entries():
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    lib = ctx.lib
    kname, lik, n, d = "m32", "poisson", 300, 2
    form, P, H = _form(kname)
    lam, N1, N2 = form
    N1, N2 = (np.ascontiguousarray(a, np.float64) for a in (N1, N2))
    t, y, z, s, f_prev, ref = (np.array(a) if isinstance(a, np.ndarray) else a for a in pass_case(kname, lik, n))
    out = {a: np.full(n, np.nan) for a in ARRAYS}
    sums = np.full(6, np.nan)

    def call(count=n, dim=d, lm=lam, lk=LIKS[lik], par=PARS[lik], ts=t, ys=y, zs=z, ss=s, fp=f_prev, o=out, sm=sums):
        return lib.pgps_gp_newton_f64(ctx.handle, _L(count), _I(dim), _F(lm), _p(N1), _p(N2), _p(P), _p(H), _I(lk), _F(par), _p(ts),
                                      _p(ys), _p(zs), _p(ss), _p(fp), _F(0.0), *(_p(o.get(a)) for a in ARRAYS), _p(sm))

    assert call(ts=None) == -1 and call(ys=None) == -1 and call(zs=None) == -1 and call(ss=None) == -1 and call(sm=None) == -1
    assert call(o={}) == -1 and call(count=0) == -1 and call(lm=0.0) == -1 and call(lm=-1.0) == -1
    assert call(lk=3) == -1 and call(lk=-1) == -1 and call(par=0.0) == -1 and call(par=np.nan) == -1
    assert call(dim=4) == -2 and call(dim=0) == -2                  # PGPS_E_UNSUPPORTED_DIM
    bad = s.copy()
    bad[np.flatnonzero(~np.isnan(y))[3]] = -1.0
    assert call(ss=bad) == -1                                       # (the host form's scan of the site variances)
    assert np.all(np.isnan(sums)) and all(np.all(np.isnan(a)) for a in out.values())       # (a refused call writes nothing)
    assert call() == 0
    assert max([err(out[a], ref[a]) for a in ARRAYS] + _sum_errors(sums, ref["sums"])) <= TOL
    # without f_prev: the same arrays, no move
    out0, sums0 = {a: np.full(n, np.nan) for a in ARRAYS}, np.full(6, np.nan)
    assert call(fp=None, o=out0, sm=sums0) == 0
    assert all(np.array_equal(_bits(out0[a]), _bits(out[a])) for a in ARRAYS) and sums0[4] == 0.0
    assert np.array_equal(_bits(np.delete(sums0, 4)), _bits(np.delete(sums, 4)))

    sites = {a: np.full(n, np.nan) for a in ("f", "alpha", "zs", "ss")}
    sums3 = np.full(3, np.nan)

    def call_sites(count=n, lk=LIKS[lik], par=PARS[lik], ys=y, fa=f_prev, aa=out["alpha"], fb=out["f"], ab=out["alpha"], step=0.5, o=sites,
                   sm=sums3):
        return lib.pgps_lik_sites_f64(ctx.handle, _L(count), _I(lk), _F(par), _p(ys), _p(fa), _p(aa), _p(fb), _p(ab), _F(step),
                                      *(_p(o.get(a)) for a in ("f", "alpha", "zs", "ss")), _p(sm))

    assert call_sites(ys=None) == -1 and call_sites(fa=None) == -1 and call_sites(aa=None) == -1 and call_sites(sm=None) == -1
    assert call_sites(o={}) == -1 and call_sites(count=0) == -1 and call_sites(lk=7) == -1 and call_sites(par=-2.0) == -1
    assert call_sites(ab=None) == -1 and call_sites(step=np.nan) == -1
    assert np.all(np.isnan(sums3)) and all(np.all(np.isnan(a)) for a in sites.values())
    assert call_sites() == 0

    # the _dev forms on device pointers give the same bits
    names = {"t": t, "y": y, "z": z, "s": s, "fp": f_prev, **out, "sums": sums, **{"s_" + k: v for k, v in sites.items()}, "sums3": sums3}
    dev = {key: ctx.malloc(a.nbytes) for key, a in names.items()}
    D = {key: ctypes.c_void_p(ptr) for key, ptr in dev.items()}
    try:
        for key in ("t", "y", "z", "s", "fp"):
            ctx.h2d(dev[key], names[key])
        args = (_L(n), _I(d), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _I(LIKS[lik]), _F(PARS[lik]), D["t"], D["y"], D["z"], D["s"], D["fp"],
                _F(0.0), *(D[a] for a in ARRAYS))
        assert lib.pgps_gp_newton_dev_f64(ctx.handle, *args, D["sums"]) == 0
        assert lib.pgps_lik_sites_dev_f64(ctx.handle, _L(n), _I(LIKS[lik]), _F(PARS[lik]), D["y"], D["fp"], D["alpha"], D["f"], D["alpha"],
                                          _F(0.5), *(D["s_" + a] for a in ("f", "alpha", "zs", "ss")), D["sums3"]) == 0
        ctx.synchronize()
        got = {key: np.full(names[key].shape, np.nan) for key in names if key not in ("t", "y", "z", "s", "fp")}
        for key, a in got.items():
            ctx.d2h(a, dev[key])
        assert lib.pgps_gp_newton_dev_f64(ctx.handle, *args, None) == -1
        assert lib.pgps_gp_newton_dev_f64(ctx.handle, *args[:7], _I(9), *args[8:], D["sums"]) == -1
        assert lib.pgps_lik_sites_dev_f64(ctx.handle, _L(n), _I(LIKS[lik]), _F(PARS[lik]), None, D["fp"], D["alpha"], None, None,
                                          _F(0.0), *(D["s_" + a] for a in ("f", "alpha", "zs", "ss")), D["sums3"]) == -1
    finally:
        for ptr in dev.values():
            ctx.free(ptr)
    for key in got:
        assert np.array_equal(_bits(got[key]), _bits(names[key])), f"the device-pointer entry differs from the host entry in {key}"


# ---- the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lik", LIKELIHOODS)
@pytest.mark.parametrize("kname", ("m32", "m52"))
def test_model_against_the_dense_reference_and_the_host_twin(kname, lik):
    from pssgp.laplace import LaplaceStateSpaceGP
    n = 300
    t, y = LR.case(lik, n)
    tq = np.sort(np.random.RandomState(2).uniform(t[0] - 0.1, t[-1] + 0.1, 40))
    ref = LR.dense_fit(kname, 1.0, 0.5, t, y, lik, PARS[lik], tol=1e-11, tq=tq, grad=True)
    assert not ref["diverged"]
    tol = MATERNS[kname][2]
    m = LaplaceStateSpaceGP((t[:, None], y[:, None]), matern(kname), _likelihood(lik), parallel=True)
    f, v = (a[:, 0] for a in m.posterior_mode())
    ev, grad = m.log_likelihood_and_grad()
    mean, var = (a[:, 0] for a in m.predict_f(tq[:, None]))
    assert m.fit_info["converged"] and float(m.maximum_log_likelihood_objective()) == float(ev)
    e = {"mode": LR.rel(f, ref["f_all"]), "variance": LR.rel(v, ref["v_all"]), "evidence": abs(ev - ref["evidence"]) / abs(ref["evidence"]),
         "predict mean": LR.rel(mean, ref["mean_q"]), "predict var": LR.rel(var, ref["var_q"]), "gradient": LR.rel(grad, ref["gradient"])}
    print(f"{kname} {lik} against the dense reference: " + " ".join(f"{k} {x:.1e}" for k, x in e.items()) + f"; {m.fit_info}")
    assert max(e.values()) <= tol, e
    host = LaplaceStateSpaceGP((t[:, None], y[:, None]), matern(kname), _likelihood(lik), parallel=False)
    hf, hv = (a[:, 0] for a in host.posterior_mode())
    hm, hvar = (a[:, 0] for a in host.predict_f(tq[:, None]))
    eh = [LR.rel(f, hf), LR.rel(v, hv), LR.rel(mean, hm), LR.rel(var, hvar),
          abs(ev - float(host.maximum_log_likelihood_objective())) / abs(ev)]
    print("   against the host twin: " + " ".join(f"{x:.1e}" for x in eh) + f"; {host.fit_info}")
    assert max(eh) <= 1e-8


def test_damping_on_the_device():
    from pssgp.kernels import Matern32
    from pssgp.laplace import LaplaceStateSpaceGP
    from pssgp.likelihoods import Poisson
    rng = np.random.default_rng(1)                  # (the case of test_laplace_host.py: undamped Newton overflows)
    t = np.sort(rng.uniform(0.0, 10.0, 200))
    K = LR.matern_K("m32", 9.0, 1.0, t, t)
    y = rng.poisson(np.exp(np.linalg.cholesky(K + 1e-10 * np.eye(200)) @ rng.standard_normal(200))).astype(float)
    assert LR.dense_laplace(K, y, "poisson", 1.0, damp=False)["diverged"]
    ref = LR.dense_laplace(K, y, "poisson", 1.0)
    m = LaplaceStateSpaceGP((t[:, None], y[:, None]), Matern32(variance=9., lengthscales=1.), Poisson(), parallel=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        f, _ = m.posterior_mode()
    print(m.fit_info, ref["iterations"], ref["halvings"])
    assert m.fit_info["converged"] and m.fit_info["halvings"] > 0
    assert LR.rel(f[:, 0], ref["f"]) <= MATERNS["m32"][2]
    assert abs(float(m.maximum_log_likelihood_objective()) - ref["evidence"]) <= MATERNS["m32"][2] * abs(ref["evidence"])
