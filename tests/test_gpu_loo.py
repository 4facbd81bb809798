"""GPU tests of the predictive checks on the fused path (pgps_gp_loo_f64, pgps_gp_loo_dev_f64): the
one-step-ahead law y_k | y_1..k-1 and the leave-one-out law y_k | y_-k of every training row, and their summed log densities,
from one filter and one smoother pass.  ctypes -> C ABI.  References (loo_refs.py; none is the code under test): a numpy Kalman
filter + RTS smoother followed by the cavity formula at the project's 1e-9 (max norm relative to the largest entry), and the
dense K_y^-1 formula over the observed rows at kernel_zoo's tolerance against the dense GP (1e-6).  Shapes: those of
test_gpu_het_noise.py -- N in {1, 2, 37, 300} on the default geometry, 700 with one step per lane (three workgroups, a ragged
tail, the spine fold, rows 252..260 missing across a workgroup boundary) and with three (a chunk that is no whole sub-tile: the
unstaged path) -- and 300 rows with five repeated times (dt = 0; the references agree on it to 1e-9: test_loo_host.py).
The LDS-staged road, eight steps per lane and the forgetting shortcut: test_gpu_fused_geometries.py."""
import ctypes

import numpy as np
import pytest

from loo_refs import FIELDS, MATERNS, R, TOL, case, err, gaps, log_density, matern, refs, sde_of, ss_checks

pytestmark = pytest.mark.gpu

KNAMES = ("m12", "m32", "m52")
# (N, steps per lane or 0 = the default geometry, a run of missing rows (first, length) or None, repeated times)
GEOMS = [(1, 0, None, False), (2, 0, None, False), (37, 0, None, False), (300, 0, None, False), (700, 1, (252, 9), False),
         (700, 3, None, False), (300, 0, None, True)]
GEOM_IDS = ["N1", "N2", "N37", "N300", "N700-chunk1-straddle", "N700-chunk3", "N300-repeated-times"]


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


@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_arrays_and_sums_against_both_references(kname, geom):
    from pssgp import _backend as Bk
    n, chunk, run, repeated = geom
    form, P, H = _form(kname)
    t, y, _ = case(n, run, repeated)
    if run is not None:
        assert np.all(np.isnan(y[run[0]:run[0] + run[1]]))
    with _Chunk(chunk):
        got = Bk.gp_loo(form, P, H, R, t, y)
        again = Bk.gp_loo(form, P, H, R, t, y)
        scores = Bk.gp_loo(form, P, H, R, t, y, osa=False, loo=False)
        ll = float(Bk.gp(form, P, H, R, t, y)["ll"])              # (existing code: the log-likelihood of the same series)
    e_ss, e_dn = gaps(got, kname, n, run, repeated)
    e_ll = abs(got["ll"] - ll) / abs(ll)
    print(f"{kname} N {n} chunk {chunk}{' repeated times' if repeated else ''}: state-space {e_ss:.2e} dense {e_dn:.2e} "
          f"ll against gp {e_ll:.2e}")
    assert e_ss <= TOL and e_dn <= MATERNS[kname][2]
    assert e_ll <= 1e-12
    # the log densities (formed on the host from (y, mean, var)): NaN exactly at the missing rows, the references' elsewhere
    ss = refs(kname, n, run, repeated)[0]
    nan = np.isnan(y)
    for name in ("osa", "loo"):
        logd = got[f"{name}_log_density"]
        assert logd.shape == (n,) and np.array_equal(np.isnan(logd), nan)
        assert np.all(np.isfinite(got[f"{name}_mean"])) and np.all(np.isfinite(got[f"{name}_var"]))
        assert err(logd[~nan], ss[f"{name}_log_density"][~nan]) <= TOL
    # two identical calls, and the call without the four arrays, agree bit for bit
    for f in FIELDS + ("ll", "loo_lpd"):
        assert np.array_equal(_bits(got[f]), _bits(again[f])), f"two calls differ in {f}"
    assert set(scores) == {"ll", "loo_lpd"}
    for f in ("ll", "loo_lpd"):
        assert np.array_equal(_bits(got[f]), _bits(scores[f])), f"the scores-only call differs in {f}"


_L, _I, _F = ctypes.c_long, ctypes.c_int, ctypes.c_double


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_abi_errors_and_the_dev_entry():
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    lib = ctx.lib
    kname, n, d = "m32", 300, 2
    form, P, H = _form(kname)
    lam, N1, N2 = form
    N1, N2 = (np.ascontiguousarray(a, np.float64) for a in (N1, N2))
    t, y = (np.array(a) for a in case(n)[:2])
    arrays = {f: np.full(n, np.nan) for f in FIELDS}
    sums = np.full(2, np.nan)

    def call(count=n, dim=d, r=R, ts=t, ys=y, out=arrays, sm=sums):
        return lib.pgps_gp_loo_f64(ctx.handle, _L(count), _I(dim), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _F(r), _p(ts), _p(ys),
                                   _F(0.0), *(_p(out.get(f)) for f in FIELDS), _p(sm))

    assert call(r=0.0) == -1                        # PGPS_E_INVALID: leaving out a noise-free observation is undefined
    assert call(r=-0.01) == -1 and call(r=np.nan) == -1 and call(r=np.inf) == -1
    assert call(ts=None) == -1 and call(ys=None) == -1 and call(sm=None) == -1
    assert call(count=0) == -1
    assert call(dim=4) == -2 and call(dim=0) == -2  # PGPS_E_UNSUPPORTED_DIM
    assert np.all(np.isnan(sums)) and all(np.all(np.isnan(a)) for a in arrays.values())     # (a refused call writes nothing)
    # a valid call on the same context after the refused ones
    assert call() == 0
    e_ss, e_dn = gaps({**arrays, "ll": sums[0], "loo_lpd": sums[1]}, kname, n)
    assert e_ss <= TOL and e_dn <= MATERNS[kname][2]
    # any subset of the arrays: the others are not touched, the ones asked for and the sums have the same bits
    only, sums1 = {"loo_var": np.full(n, np.nan)}, np.full(2, np.nan)
    assert call(out=only, sm=sums1) == 0
    assert np.array_equal(_bits(only["loo_var"]), _bits(arrays["loo_var"])) and np.array_equal(_bits(sums1), _bits(sums))
    # the _dev form on device pointers gives the same bits
    names = {"t": t, "y": y, **arrays, "sums": sums}
    dev = {key: ctx.malloc(a.nbytes) for key, a in names.items()}
    D = {key: ctypes.c_void_p(ptr) for key, ptr in dev.items()}
    try:
        ctx.h2d(dev["t"], t), ctx.h2d(dev["y"], y)
        rc = lib.pgps_gp_loo_dev_f64(ctx.handle, _L(n), _I(d), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _F(R), D["t"], D["y"], _F(0.0),
                                     *(D[f] for f in FIELDS), D["sums"])
        assert rc == 0
        ctx.synchronize()
        got = {key: np.full(names[key].shape, np.nan) for key in FIELDS + ("sums",)}
        for key, a in got.items():
            ctx.d2h(a, dev[key])
        assert lib.pgps_gp_loo_dev_f64(ctx.handle, _L(n), _I(d), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _F(0.0), D["t"], D["y"], _F(0.0),
                                       *(D[f] for f in FIELDS), D["sums"]) == -1
        assert lib.pgps_gp_loo_dev_f64(ctx.handle, _L(n), _I(d), _F(lam), _p(N1), _p(N2), _p(P), _p(H), _F(R), D["t"], D["y"], _F(0.0),
                                       *(D[f] for f in FIELDS), None) == -1
    finally:
        for ptr in dev.values():
            ctx.free(ptr)
    for key in FIELDS + ("sums",):
        assert np.array_equal(_bits(got[key]), _bits(names[key])), f"the device-pointer entry differs from the host entry in {key}"


# ---- model routing ------------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    from pssgp import _backend as Bk
    calls = {"gp_loo": 0, "Series": 0}

    def wrap(name):
        real = getattr(Bk, name)

        def spy(*args, **kwargs):
            calls[name] += 1
            return real(*args, **kwargs)
        monkeypatch.setattr(Bk, name, spy)

    for name in calls:
        wrap(name)
    return calls


def _model_dict(m):
    (om, ov, ol), (lm, lv, ld) = m.one_step_ahead(), m.leave_one_out()
    return {"osa_mean": om[:, 0], "osa_var": ov[:, 0], "loo_mean": lm[:, 0], "loo_var": lv[:, 0], "ll": float(np.nansum(ol)),
            "loo_lpd": float(m.loo_log_predictive_density()), "loo_log_density": ld[:, 0]}


def test_a_matern_model_takes_the_device_route_and_no_resident_series(monkeypatch):
    from pssgp.model import StateSpaceGP
    calls = _spy(monkeypatch)
    kname, n = "m32", 300
    t, y, _ = case(n)
    m = StateSpaceGP((t[:, None], y[:, None]), matern(kname), noise_variance=R, parallel=True)
    want = 0
    for _ in range(3):                              # (predict_f makes the series resident at the second evaluation: not these)
        for call in (m.one_step_ahead, m.leave_one_out, m.loo_log_predictive_density):
            out = call()
            want += 1
            assert calls == {"gp_loo": want, "Series": 0}
        assert np.ndim(out) == 0
    assert not getattr(m, "_series", None)
    got = _model_dict(m)
    e_ss, e_dn = gaps(got, kname, n)
    print(f"model, device route: state-space {e_ss:.2e} dense {e_dn:.2e}")
    assert e_ss <= TOL and e_dn <= MATERNS[kname][2]
    nan = np.isnan(y)
    assert np.array_equal(np.isnan(got["loo_log_density"]), nan)
    assert np.array_equal(got["loo_log_density"][~nan], log_density(y[~nan], got["loo_mean"][~nan], got["loo_var"][~nan]))
    ll = float(m.maximum_log_likelihood_objective())
    assert abs(got["ll"] - ll) <= 1e-12 * abs(ll)
    with pytest.raises(ValueError, match="noise_variance"):
        StateSpaceGP((t[:, None], y[:, None]), matern(kname), noise_variance=0.0, parallel=True).leave_one_out()


def test_an_rbf_model_and_observation_variances_take_the_host_twin(monkeypatch):
    from pssgp.kernels import RBF
    from pssgp.model import StateSpaceGP
    calls = _spy(monkeypatch)
    n = 200
    t, y, s = case(n)
    rbf = RBF(variance=1., lengthscales=0.5, order=4, balancing_iter=5)
    models = {"rbf4": (StateSpaceGP((t[:, None], y[:, None]), rbf, noise_variance=R, parallel=True), rbf.get_sde(), R),
              "m32 with s": (StateSpaceGP((t[:, None], y[:, None]), matern("m32"), noise_variance=R, parallel=True,
                                          observation_variances=s), sde_of("m32"), R + s)}
    for name, (m, sde, Rk) in models.items():
        got = _model_dict(m)
        assert calls == {"gp_loo": 0, "Series": 0}, (name, calls)
        ref = ss_checks(sde, t, y, Rk)
        e = [err(got[f], ref[f]) for f in FIELDS] + [abs(got[x] - ref[x]) / abs(ref[x]) for x in ("ll", "loo_lpd")]
        print(f"{name} on the host twin: " + " ".join(f"{x:.2e}" for x in e))
        assert max(e) <= TOL, (name, e)
