"""GPU tests of the panel's mean-function entry points (pgps_gp_panel_gram_*, pgps_gp_panel_residual_dev_f64; k_gpp_gram,
csrc/pgps_panel_gram.hip.h) and of StateSpaceGPPanel(..., mean_function=...) on the device route.
ctypes -> C ABI.  Data and references: panel_trend_refs.py (a different seed per series, so a read from a neighbour's rows
moves a result; the numpy multi-column filter with a per-step R + s_k; dense GLS) -- none is the code under test.  Every case
asserts the reference's two conditions (panel_trend_refs.well_posed) before any device call, on every series of at least 10
rows (a series of 1 or 2 rows has fewer observed rows than basis functions: its Gram record is still checked entry by entry).
Tolerances: 1e-9 on |G_ij - ref| / sqrt(G_ii G_jj) (test_gpu_whiten.py's metric), 1e-9 relative on logdet, n_obs exact.  Every
checked call follows the same call on other data (_fresh): W lives in scratch that is not zeroed."""
import ctypes
import functools

import numpy as np
import pytest

import panel_trend_refs as T
from het_refs import LOG2PI, R, matern, rel, sde_of
from test_gpu_panel import _BatchScratch, _CountLaunches, _form, _kernel, _model, _same_bits
from test_gpu_multi_geometries import _Chunk

pytestmark = pytest.mark.gpu

TOL = 1e-9
HET = pytest.mark.parametrize("het", [False, True], ids=["scalar", "rs"])
LENGTHS = (257, 1, 700, 37, 256, 2, 255)
LONG = (2048, 37)                                       # one panel holding a series at PGPS_PANEL_MAX_STEPS
CLASS_LENGTHS = (257, 12, 700, 37, 256, 16, 255)        # every series has more observed rows than basis functions
TILE = {"m12": 8, "m32": 4, "m52": 2}                   # MultiTile<D>::MC
CHUNKS = [1, 4, 16, 0]
E_INVALID = -1
# C: one column, two, the tile + 1 (a second round that holds one column; at d = 1 the tile is all 8 columns) and 8
GRAM_CASES = [(k, c) for k in T.KNAMES for c in sorted({1, 2, min(TILE[k] + 1, 8), 8})]


def _concat(lengths, C, het, order=None, flip=False):
    """(offs, ts, V, rs or None) of the panel's series in `order`; flip: other data of the same shape (the same rows missing)."""
    cases = T.panel(lengths)
    idx = list(range(len(cases)) if order is None else order)
    offs = np.concatenate([[0], np.cumsum([cases[i][0].size for i in idx])]).astype(np.int64)
    V = np.concatenate([T.wide_columns(cases[i][0], cases[i][1], C) for i in idx])
    return (offs, np.concatenate([cases[i][0] for i in idx]), np.ascontiguousarray(1.0 - V if flip else V),
            np.concatenate([cases[i][2] for i in idx]) if het else None)


def _gram(models, lengths, C, het, order=None, chunk=0, budget=0):
    """gp_panel_gram (the host form) after the same call on other data under the library's own geometry and budget."""
    from pssgp import _backend as Bk
    Bk.gp_panel_gram(models, *_concat(lengths, C, het, order, flip=True))
    offs, ts, V, rs = _concat(lengths, C, het, order)
    with _Chunk(chunk), _BatchScratch(budget):
        return Bk.gp_panel_gram(models, offs, ts, V, rs)


def _gram_err(G, G_ref):
    dg = np.sqrt(np.diag(G_ref))
    return float(np.max(np.abs(G - G_ref) / np.outer(dg, dg)))


# ---- 1. the records at every geometry --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname,C", GRAM_CASES)
@HET
@pytest.mark.parametrize("chunk", CHUNKS)
def test_gram_against_the_reference(kname, C, het, chunk):
    from pssgp import _backend as Bk
    for lengths in (LENGTHS, LONG):
        refs = [T.ref_gram(kname, lengths, i, het, None, C) for i in range(len(lengths))]
        for i, n in enumerate(lengths):
            if n >= 10:
                T.well_posed(*refs[i], (kname, het, C, i))
        G, logdet, n_obs = _gram([_model(kname)], lengths, C, het, chunk=chunk)
        assert G.shape == (len(lengths), C, C) and logdet.shape == n_obs.shape == (len(lengths),)
        for i, (G_ref, logdet_ref, n_ref) in enumerate(refs):
            e = [_gram_err(G[i], G_ref), abs(logdet[i] - logdet_ref) / abs(logdet_ref)]
            print(f"{kname} rs {het} C {C} chunk {chunk} series {i} (n {lengths[i]}): G {e[0]:.2e} logdet {e[1]:.2e}")
            assert max(e) <= TOL, (i, e)
            assert n_obs[i] == n_ref
            _same_bits(G[i], G[i].T.copy(), ("G is symmetric bit for bit", i))
        if C == 1:
            # -(n log 2 pi + logdet + G_00) / 2 is the panel's log-likelihood (test_gpu_whiten.py's check through gp_ll_multi)
            offs, ts, V, rs = _concat(lengths, 1, het)
            ll = Bk.gp_panel_ll([_model(kname)], offs, ts, V[:, 0], rs)
            np.testing.assert_allclose(-0.5 * (n_obs * LOG2PI + logdet + G[:, 0, 0]), ll, rtol=1e-11, atol=0.0)


# ---- 2. a record depends on nothing else -----------------------------------------------------------------------------------------
def _records_equal(got, want, order, what):
    for j, i in enumerate(order):
        for a, b, name in zip(got, want, ("G", "logdet", "n_obs")):
            _same_bits(np.asarray(a[j], np.float64), np.asarray(b[i], np.float64), (what, name, i))


@pytest.mark.parametrize("kname", T.KNAMES)
@HET
def test_a_record_depends_on_nothing_but_its_series(kname, het):
    C, S = 5, len(LENGTHS)
    models = [_model(kname)]
    want = _gram(models, LENGTHS, C, het)
    _records_equal(_gram(models, LENGTHS, C, het), want, range(S), "repeated")
    rev = list(range(S - 1, -1, -1))
    _records_equal(_gram(models, LENGTHS, C, het, order=rev), want, rev, "reversed")
    for i in range(S):
        _records_equal(_gram(models, LENGTHS, C, het, order=[i]), want, [i], "alone")
    # a budget of one byte: every series is a group of its own, S launches; 300 KiB: groups of uneven size
    from pssgp import _backend as Bk
    offs, ts, V, rs = _concat(LENGTHS, C, het)
    with _BatchScratch(1), _CountLaunches() as count:
        got = Bk.gp_panel_gram(models, offs, ts, V, rs)
        n = count.launches()
    assert n == S, n
    _records_equal(got, want, range(S), "one series per group")
    with _BatchScratch(300 * 1024), _CountLaunches() as count:
        got = Bk.gp_panel_gram(models, offs, ts, V, rs)
        n = count.launches()
    print(f"{kname} rs {het}: {n} launches under a 300 KiB budget")
    assert 1 <= n < S
    _records_equal(got, want, range(S), "a few series per group")
    _records_equal(_gram(models * S, LENGTHS, C, het), want, range(S), "S equal rows of the model table")
    # a pinned chunk that covers every series changes the steps per lane, not the reference it agrees with
    pinned = _gram(models, LENGTHS, C, het, chunk=4)
    _records_equal(_gram(models, LENGTHS, C, het, order=rev, chunk=4), pinned, rev, "reversed, chunk 4")


@pytest.mark.parametrize("kname", T.KNAMES)
def test_scalar_noise_against_the_single_series_gram(kname):
    from pssgp import _backend as Bk
    C = 5
    form, P, H = _form(kname)
    G, logdet, n_obs = _gram([_model(kname)], LENGTHS, C, False)
    for i, (t, y, _) in enumerate(T.panel(LENGTHS)):
        G1, logdet1, n1 = Bk.gp_gram_multi(form, P, H, R, t, T.wide_columns(t, y, C))
        e = [_gram_err(G[i], G1), abs(logdet[i] - logdet1) / abs(logdet1)]
        print(f"{kname} series {i} against gp_gram_multi alone: {e[0]:.2e} {e[1]:.2e}")
        assert max(e) <= TOL and n_obs[i] == n1


# ---- 3. the residual kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 5, 8])
def test_residual_kernel_bits(C):
    from pssgp import _backend as Bk
    offs, ts, V, _ = _concat(LENGTHS, C, False)
    S = len(LENGTHS)
    betas = np.random.RandomState(C).randn(S, C - 1)
    want = np.empty(V.shape[0])
    for s in range(S):
        for k in range(offs[s], offs[s + 1]):
            acc = np.float64(0.0)
            for j in range(C - 1):                      # (left to right, every product and sum rounded once)
                acc = acc + V[k, 1 + j] * betas[s, j]
            want[k] = V[k, 0] - acc
    data = Bk.PanelData(offs, ts, V[:, 0], None, V=V)
    try:
        view = Bk.panel.gp_panel_residual_dev(data, betas, data.residual_view())
        got = np.full(V.shape[0], 7.0)
        data.ctx.d2h(got, view.ys)
        missing = np.isnan(V[:, 0])
        assert missing.sum() > 100 and np.all(np.isnan(got[missing]))
        _same_bits(got[~missing], want[~missing], "residual rows")
        # ... into the panel's own ys
        Bk.panel.gp_panel_residual_dev(data, betas, data)
        data.ctx.d2h(got, data.ys)
        _same_bits(got[~missing], want[~missing], "residual rows in place")
    finally:
        data.close()


# ---- 4. the ABI -----------------------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_abi_errors_leave_the_output_untouched():
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    lib = ctx.lib
    C, S = 3, len(LENGTHS)
    offs, ts, V, rs = _concat(LENGTHS, C, True)
    table, d = Bk._gp_rows([_model("m32")])
    out = np.full((S, 8 * 8 + 2), -3.0)

    def call(offs_=offs, S_=S, C_=C, V_=V, rs_=rs, table_=table, fn="pgps_gp_panel_gram_f64"):
        return getattr(lib, fn)(ctx.handle, S_, _p(offs_), d, 1, _p(table_), C_, _p(ts), _p(V_), _p(rs_), _p(out))

    partial = V.copy()
    partial[np.flatnonzero(~np.isnan(V[:, 0]))[5], 2] = np.nan          # a row that is NaN in some columns only
    zero_R = table.copy()
    zero_R[0, -1] = 0.0
    big = np.zeros((2049, 9))
    invalid = {"C = 0": call(C_=0), "C = 9": call(C_=9, V_=big), "a 2049-row series": call(S_=1, offs_=np.array([0, 2049], np.int64), V_=big),
               "NaN in some columns only": call(V_=partial), "R = 0 without rs": call(table_=zero_R, rs_=None),
               "C = 0 (dev)": call(C_=0, fn="pgps_gp_panel_gram_dev_f64"), "C = 9 (dev)": call(C_=9, fn="pgps_gp_panel_gram_dev_f64"),
               "residual C = 9": lib.pgps_gp_panel_residual_dev_f64(ctx.handle, S, _p(offs), 9, _p(V), _p(V), _p(out)),
               "residual C = 0": lib.pgps_gp_panel_residual_dev_f64(ctx.handle, S, _p(offs), 0, _p(V), _p(V), _p(out))}
    assert {k: v for k, v in invalid.items() if v != E_INVALID} == {}
    assert np.all(out == -3.0), "a refused call must not touch the output"
    assert ctx.status() == 0
    assert call(table_=zero_R) == 0 and call() == 0             # (R = 0 is accepted with rs; the context still works)
    assert np.all(out.reshape(-1)[:S * (C * C + 2)] != -3.0)
    # the _dev form on device pointers gives the bits of the host form (with and without rs)
    for rs_ in (rs, None):
        host = Bk.gp_panel_gram(table, offs, ts, V, rs_)
        data = Bk.PanelData(offs, ts, V[:, 0], rs_, V=V)
        try:
            for a, b in zip(Bk.panel.gp_panel_gram_dev(data, table), host):
                _same_bits(np.asarray(a, np.float64), np.asarray(b, np.float64), "the _dev form")
        finally:
            data.close()


# ---- 5. the class on the device route ------------------------------------------------------------------------------------------
class _Spy:
    """Counts the calls of the _backend.panel wrappers the class takes (restored on exit)."""
    NAMES = ("gp_panel_gram_dev", "gp_panel_residual_dev", "gp_panel_ll_dev", "gp_panel_ll_grad_dev", "gp_panel_predict_dev",
             "gp_panel_loo_dev")

    def __enter__(self):
        from pssgp import _backend as Bk
        self.calls, self._saved = [], []
        for name in self.NAMES:
            fn = getattr(Bk.panel, name)
            self._saved.append((name, fn))
            setattr(Bk.panel, name, self._wrap(name, fn))
        return self

    def _wrap(self, name, fn):
        def inner(*a, **kw):
            self.calls.append(name)
            return fn(*a, **kw)
        return inner

    def take(self):
        out, self.calls = self.calls, []
        return out

    def __exit__(self, *exc):
        from pssgp import _backend as Bk
        for name, fn in self._saved:
            setattr(Bk.panel, name, fn)


@functools.lru_cache(maxsize=None)
def _class_refs(kname, het, basis):
    """Per series of CLASS_LENGTHS: (beta, cov, profile, flat, cond) from the state-space reference, after its conditions hold."""
    out = []
    for i in range(len(CLASS_LENGTHS)):
        G, logdet, n_obs = T.ref_gram(kname, CLASS_LENGTHS, i, het, basis)
        cond = T.well_posed(G, logdet, n_obs, (kname, het, basis, i))
        out.append(T.gls_from_gram(G, logdet, n_obs)[:4] + (cond,))
    return out


def _class_panel(kname, het, basis, parallel=True, lengths=CLASS_LENGTHS, mean_function=None):
    from pssgp.panel import StateSpaceGPPanel
    cases = T.panel(lengths)
    return StateSpaceGPPanel([(t, y) for t, y, _ in cases], _kernel(kname), noise_variance=R, parallel=parallel,
                             observation_variances=[s for _, _, s in cases] if het else None,
                             mean_function=T.bases()[basis] if mean_function is None else mean_function)


@pytest.mark.parametrize("kname", T.KNAMES)
@HET
@pytest.mark.parametrize("basis", ["linear", "cubic"])
def test_the_class_on_the_device_route(kname, het, basis):
    from oracle import np_grad as G
    from pssgp.kernels.sde_grads import sde_with_grads
    from pssgp.model import StateSpaceGP
    refs = _class_refs(kname, het, basis)
    cases = T.panel(CLASS_LENGTHS)
    S = len(cases)
    panel = _class_panel(kname, het, basis)
    assert panel._panel_data is not None and panel._panel_data.V is not None
    with _Spy() as spy:
        betas, covs, profiles = panel.mean_coefficients()
        assert spy.take() == ["gp_panel_gram_dev"]
        flats = panel.log_marginal_likelihoods_flat_mean()
        assert spy.take() == ["gp_panel_gram_dev"]
        for i, (b, c, pr, fl, cond) in enumerate(refs):
            bound = 4.0 * cond * TOL                    # (from the Gram tolerance: at most 4e-7)
            e = [float(np.max(np.abs(betas[i] - b)) / np.max(np.abs(b))), abs(profiles[i] - pr) / abs(pr), abs(flats[i] - fl) / abs(fl)]
            print(f"{kname} rs {het} {basis} series {i}: beta {e[0]:.2e} (bound {bound:.2e}) profile {e[1]:.2e} flat {e[2]:.2e}")
            assert e[0] <= bound and bound <= 4e-7 and max(e[1:]) <= TOL, (i, e)
        # the profile likelihood's gradient: that of the zero-mean model on the REFERENCE residuals y - Phi beta_ref
        before = np.arange(float(S * betas.shape[1])).reshape(betas.shape)
        panel.betas = before
        total, grad = panel.profile_log_likelihood_and_grad()
        assert spy.take() == ["gp_panel_gram_dev", "gp_panel_residual_dev", "gp_panel_ll_grad_dev"]
        assert np.array_equal(panel.betas, before)
        sde, kgrads = sde_with_grads(_kernel(kname))
        w_ll, w_g = 0.0, np.zeros(3)
        for i, (t, y, s) in enumerate(cases):
            res = y - T.design(basis, t) @ refs[i][0]
            if het:         # (np_grad has one R for all steps: the single-series adjoint entry point on the same residuals)
                m = StateSpaceGP((t[:, None], res[:, None]), _kernel(kname), noise_variance=R, parallel=True, observation_variances=s)
                l1, g1 = m.log_likelihood_and_grad(method="adjoint")
            else:
                stats = G.ll_grad_stats(sde.F, sde.P0, sde.H, R, t[~np.isnan(res)], res[~np.isnan(res)])
                l1, g1 = stats[0], G.contract(stats, sde.H, kgrads)
            w_ll, w_g = w_ll + float(l1), w_g + np.asarray(g1, np.float64)
        e = [abs(float(total) - w_ll) / abs(w_ll), rel(grad, w_g), abs(float(total) - np.sum([r[2] for r in refs])) / abs(w_ll)]
        print(f"{kname} rs {het} {basis}: profile ll and gradient {e[0]:.2e} {e[1]:.2e}, against the summed profiles {e[2]:.2e}")
        assert max(e) <= TOL, e
        # the evaluations at the fitted betas against the loop
        fitted = panel.fit_mean_functions()
        assert spy.take() == ["gp_panel_gram_dev"] and np.array_equal(fitted, betas)
        Xnews = [np.linspace(t[0] - 0.05, t[-1] + 0.05, 9) for t, _, _ in cases]
        pred = panel.predict_f(Xnews)
        assert spy.take() == ["gp_panel_predict_dev"]
        loo = panel.leave_one_out()
        lpd = panel.loo_log_predictive_densities()
        assert spy.take() == ["gp_panel_loo_dev", "gp_panel_loo_dev"]
        lls = panel.log_likelihoods()
        assert spy.take() == ["gp_panel_ll_dev"]
    for i, (t, y, s) in enumerate(cases):
        m = StateSpaceGP((t[:, None], (y - T.design(basis, t) @ betas[i])[:, None]), _kernel(kname), noise_variance=R, parallel=True,
                         observation_variances=s if het else None)
        w_mean, w_var = m.predict_f(Xnews[i][:, None])
        w_mean = w_mean[:, 0] + T.design(basis, Xnews[i]) @ betas[i]
        w_loo = m.leave_one_out()
        e = [rel(pred[i][0][:, 0], w_mean), rel(pred[i][1][:, 0], w_var[:, 0]),
             rel(loo[i][0][:, 0], w_loo[0][:, 0] + T.design(basis, t) @ betas[i]), rel(loo[i][1][:, 0], w_loo[1][:, 0]),
             abs(lpd[i] - float(m.loo_log_predictive_density())) / abs(lpd[i]), abs(lls[i] - profiles[i]) / abs(profiles[i])]
        print(f"{kname} rs {het} {basis} series {i}: at the fitted betas against the loop " + " ".join(f"{x:.2e}" for x in e))
        assert max(e) <= TOL, (i, e)


@HET
def test_the_class_against_its_host_twin(het):
    """mean_grams of the device route against the loop of section 4 (parallel=False: the single model, or the twin with rs)."""
    dev, host = _class_panel("m32", het, "quadratic"), _class_panel("m32", het, "quadratic", parallel=False)
    for i, (a, b) in enumerate(zip(dev.mean_grams(), host.mean_grams())):
        assert _gram_err(a.G, b.G) <= TOL and abs(a.logdet - b.logdet) <= TOL * abs(b.logdet) and a.n_obs == b.n_obs, i


@HET
def test_a_long_series_is_spliced_and_nine_columns_fall_back(het):
    from pssgp.mean_functions import Basis
    lengths = (37, 3000, 300)
    refs = [T.gls_from_gram(*T.ref_gram("m32", lengths, i, het, "linear")) for i in range(3)]
    panel = _class_panel("m32", het, "linear", lengths=lengths)
    with _Spy() as spy:
        betas, _, profiles = panel.mean_coefficients()
        assert spy.take() == ["gp_panel_gram_dev"] and panel._panel_data.S == 2
        total, _ = panel.profile_log_likelihood_and_grad()
        assert spy.take() == ["gp_panel_gram_dev", "gp_panel_residual_dev", "gp_panel_ll_grad_dev"]
    for i, r in enumerate(refs):
        assert np.max(np.abs(betas[i] - r[0])) <= 4.0 * r[4] * TOL * np.max(np.abs(r[0])) and abs(profiles[i] - r[2]) <= TOL * abs(r[2]), i
    assert abs(float(total) - np.sum(profiles)) <= TOL * abs(np.sum(profiles))
    # C = 9: off the panel entry points, the same numbers as the host loop
    cos8 = lambda: Basis(lambda t: np.stack([np.cos(j * np.pi * (t - 0.05)) for j in range(8)], axis=1), 8)
    wide, host = (_class_panel("m32", het, None, parallel=par, mean_function=cos8()) for par in (True, False))
    with _Spy() as spy:
        g_dev = wide.mean_grams()
        assert spy.take() == [] and wide._panel_data.V is None
    for i, (a, b) in enumerate(zip(g_dev, host.mean_grams())):
        assert a.G.shape == (9, 9)
        assert _gram_err(a.G, b.G) <= TOL and abs(a.logdet - b.logdet) <= TOL * abs(b.logdet) and a.n_obs == b.n_obs, i
