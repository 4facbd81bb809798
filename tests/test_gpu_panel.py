"""GPU tests of the panel entry points (pgps_gp_panel_ll_*, pgps_gp_panel_ll_grad_*, pgps_gp_panel_predict_*; DESIGN.md section
4aa) and of StateSpaceGPPanel on the device route: S series, each on its own clock, one workgroup per series.  ctypes -> C ABI.
Data: het_refs.series / queries with a different seed per series, so a read from a neighbour's rows moves a result.
References (none is the code under test): het_refs.ss_het (a numpy Kalman filter + RTS smoother) at the project's 1e-9,
het_refs.dense_het at kernel_zoo's 1e-6, and the existing single-series device entry points at 1e-9."""
import ctypes
import functools

import numpy as np
import pytest

from het_refs import MATERNS, R, dense_het, queries, rel, sde_of, series, ss_het

pytestmark = pytest.mark.gpu

TOL = 1e-9
KNAMES = ("m12", "m32", "m52")
HET = pytest.mark.parametrize("het", [False, True], ids=["scalar", "rs"])
# odd sizes, one and two rows, a multiple of the 256 lanes and its two neighbours; a series without queries, one with a single one
LENGTHS = (257, 1, 700, 37, 256, 2, 255)
QUERIES = (50, 1, 50, 0, 50, 4, 1)
E_INVALID, E_UNSUPPORTED_DIM = -1, -2


def _form(kname, variance=1.0, ell=0.5):
    import pssgp.kernels as Kn
    from pssgp import _backend as Bk
    sde = getattr(Kn, MATERNS[kname][0])(variance=variance, lengthscales=ell).get_sde()
    return Bk.nilpotent_form(sde.F), np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1)


def _model(kname, Rv=R, variance=1.0, ell=0.5):
    form, P, H = _form(kname, variance, ell)
    return (form, P, H, Rv)


@functools.lru_cache(maxsize=None)
def _panel(lengths, counts):
    """[(t, y, s, tq)] of the panel's series, read-only; series i has seed i."""
    out = []
    for i, (n, k) in enumerate(zip(lengths, counts)):
        t, y, s = series(n, seed=i)
        tq = queries(t, k, seed=i)
        for a in (t, y, s, tq):
            a.setflags(write=False)
        out.append((t, y, s, tq))
    return tuple(out)


def _concat(cases, het, order=None):
    """(offs, qoffs, ts, ys, rs or None, tq) of the cases in `order`."""
    cases = [cases[i] for i in (range(len(cases)) if order is None else order)]
    offs = np.concatenate([[0], np.cumsum([c[0].size for c in cases])])
    qoffs = np.concatenate([[0], np.cumsum([c[3].size for c in cases])])
    cat = lambda j: np.concatenate([c[j] for c in cases])
    return offs, qoffs, cat(0), cat(1), (cat(2) if het else None), cat(3)


def _calls(models, cases, het, order=None):
    """(ll (S,), (mean, var, ll) of predict, gradient rows, qoffs) of the host forms; a panel without any query has no predict
    call (qoffs[S] < 1 is refused): None in its place."""
    from pssgp import _backend as Bk
    offs, qoffs, ts, ys, rs, tq = _concat(cases, het, order)
    ll = Bk.gp_panel_ll(models, offs, ts, ys, rs)
    pred = Bk.gp_panel_predict(models, offs, qoffs, ts, ys, rs, tq) if tq.size else None
    rows = Bk.gp_panel_ll_grad(models, offs, ts, ys, rs)
    return ll, pred, rows, qoffs


def _single(model, case, het):
    """(ll, (mean, var, ll) or None, gradient row) of series `case` from the existing single-series device entry points."""
    from pssgp import _backend as Bk
    form, P, H, Rv = model
    t, y, s, tq = case
    d = P.shape[0]
    if het:
        ll = Bk.gp_ll_het(form, P, H, Rv, t, y, s)
        pred = Bk.gp_predict_het(form, P, H, Rv, t, y, s, tq) if tq.size else None
        stats = Bk.gp_ll_grad_adj_het(form, P, H, Rv, t, y, s)
    else:
        ll = float(Bk.gp(form, P, H, Rv, t, y)["ll"])
        pred = Bk.gp_predict(form, P, H, Rv, t, y, tq) if tq.size else None
        ser = Bk.Series(t, y)
        try:
            stats = ser.gp_ll_grad_adj(Bk.Series.pack(form, P, H), Rv)
        finally:
            ser.close()
    row = np.concatenate([[stats[0]], stats[1].reshape(-1), stats[2], stats[3], [stats[4]]])
    assert row.shape == (2 + d * d + 2 * d,)
    return ll, pred, row


@functools.lru_cache(maxsize=None)
def _refs(kname, lengths, counts, het, i):
    """(state-space reference, dense reference) of series i: (ll, mean, var), or (ll,) without queries.  Computed once."""
    t, y, s, tq = _panel(lengths, counts)[i]
    s = s if het else np.zeros(t.size)
    q = tq if tq.size else None
    a, b = ss_het(sde_of(kname), t, y, R, s, q), dense_het(MATERNS[kname][1], t, y, R, s, q)
    return (a, b) if q is not None else ((a,), (b,))


def _rel_ll(a, b):
    return abs(a - b) / abs(b)


def _check_against_singles(got, model_of, cases, het, what):
    """Every row of the panel's (ll, predict, gradient rows) against the single-series calls, at TOL."""
    ll, (mean, var, llp), rows, qoffs = got
    worst = 0.0
    for i, case in enumerate(cases):
        w_ll, w_pred, w_row = _single(model_of(i), case, het)
        e = [_rel_ll(ll[i], w_ll), _rel_ll(rows[i, 0], w_ll), rel(rows[i, 1:], w_row[1:])]
        if w_pred is not None:
            sl = slice(qoffs[i], qoffs[i + 1])
            e += [rel(mean[sl], w_pred[0]), rel(var[sl], w_pred[1]), _rel_ll(llp[i], w_pred[2])]
        else:
            assert qoffs[i] == qoffs[i + 1]
            e += [_rel_ll(llp[i], w_ll)]             # (the series with no query still returns its ll)
        print(f"{what} series {i} (n {case[0].size}, k {case[3].size}) against the single-series calls: " + " ".join(f"{x:.2e}" for x in e))
        worst = max(worst, max(e))
    assert worst <= TOL, (what, worst)


# ---- 1. geometry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@HET
def test_geometry_against_the_references_and_the_single_series_calls(kname, het):
    cases = _panel(LENGTHS, QUERIES)
    for t, _, _, tq in cases:
        if tq.size >= 4 and t.size >= 37:
            assert np.intersect1d(tq, t).size >= 1          # (ties between queries and training times are present)
    model = _model(kname)
    got = _calls([model], cases, het)
    ll, (mean, var, llp), rows, qoffs = got
    assert ll.shape == (7,) and llp.shape == (7,) and mean.shape == var.shape == (sum(QUERIES),)
    tol = MATERNS[kname][2]
    for i, (t, y, s, tq) in enumerate(cases):
        ref_ss, ref_d = _refs(kname, LENGTHS, QUERIES, het, i)
        sl = slice(qoffs[i], qoffs[i + 1])
        e = [_rel_ll(ll[i], ref_ss[0]), _rel_ll(llp[i], ref_ss[0]), _rel_ll(rows[i, 0], ref_ss[0])]
        if tq.size:
            e += [rel(mean[sl], ref_ss[1]), rel(var[sl], ref_ss[2])]
        print(f"{kname} rs {het} series {i} (n {t.size}, k {tq.size}) against the state-space reference: " + " ".join(f"{x:.2e}" for x in e))
        assert max(e) <= TOL, (i, e)
        for g in (ll[i], llp[i], rows[i, 0]):
            np.testing.assert_allclose(g, ref_d[0], atol=tol, rtol=tol)
        if tq.size:
            np.testing.assert_allclose(mean[sl], ref_d[1], atol=tol, rtol=tol)
            np.testing.assert_allclose(var[sl], ref_d[2], atol=tol, rtol=tol)
    _check_against_singles(got, lambda i: model, cases, het, f"{kname} rs {het}")


# ---- 2. one full workgroup ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname,het", [("m12", True), ("m32", False), ("m52", True)])
def test_one_full_workgroup_and_the_limit(kname, het):
    """2048 steps is the limit: eight steps per lane on all 256 lanes.  ll and gradient on lengths (2048, 3, 2047); predict on
    (1536, 3, 2047) with (512, 2, 1) queries -- 2048, 5 and 2048 merged steps; one query more is refused.  Against the
    single-series calls at 1e-9 and the dense GP at 1e-6 (the log-likelihoods)."""
    from pssgp import _backend as Bk
    model = _model(kname)
    full = _panel((2048, 3, 2047), (0, 0, 0))
    offs, _, ts, ys, rs, _ = _concat(full, het)
    ll = Bk.gp_panel_ll([model], offs, ts, ys, rs)
    rows = Bk.gp_panel_ll_grad([model], offs, ts, ys, rs)
    tol = MATERNS[kname][2]
    for i, case in enumerate(full):
        w_ll, _, w_row = _single(model, case, het)
        e = [_rel_ll(ll[i], w_ll), _rel_ll(rows[i, 0], w_ll), rel(rows[i, 1:], w_row[1:])]
        print(f"{kname} rs {het} n {case[0].size}: ll, gradient row against the single-series calls " + " ".join(f"{x:.2e}" for x in e))
        assert max(e) <= TOL, e
        s = case[2] if het else np.zeros(case[0].size)
        np.testing.assert_allclose(ll[i], dense_het(MATERNS[kname][1], case[0], case[1], R, s), atol=tol, rtol=tol)
    at_limit = _panel((1536, 3, 2047), (512, 2, 1))
    offs, qoffs, ts, ys, rs, tq = _concat(at_limit, het)
    mean, var, llp = Bk.gp_panel_predict([model], offs, qoffs, ts, ys, rs, tq)
    for i, case in enumerate(at_limit):
        w_mean, w_var, w_ll = _single(model, case, het)[1]
        sl = slice(qoffs[i], qoffs[i + 1])
        e = [rel(mean[sl], w_mean), rel(var[sl], w_var), _rel_ll(llp[i], w_ll)]
        print(f"{kname} rs {het} n {case[0].size} k {case[3].size}: predict against the single-series call " + " ".join(f"{x:.2e}" for x in e))
        assert max(e) <= TOL, e
    over = _panel((1536, 3, 2047), (513, 2, 1))
    offs, qoffs, ts, ys, rs, tq = _concat(over, het)
    with pytest.raises(Bk.PgpsError) as err:
        Bk.gp_panel_predict([model], offs, qoffs, ts, ys, rs, tq)
    assert err.value.code == E_INVALID
    long_ = _panel((2049, 3), (0, 0))
    offs, _, ts, ys, rs, _ = _concat(long_, het)
    with pytest.raises(Bk.PgpsError) as err:
        Bk.gp_panel_ll([model], offs, ts, ys, rs)
    assert err.value.code == E_INVALID


# ---- 3. a row depends on nothing else ----------------------------------------------------------------------------------------
class _BatchScratch:
    """pgps_set_batch_scratch for the block, restored on every exit."""

    def __init__(self, nbytes):
        from pssgp import _backend as Bk
        self.ctx, self.nbytes = Bk.get_context(), nbytes

    def __enter__(self):
        self.ctx.set_batch_scratch(self.nbytes)

    def __exit__(self, *exc):
        self.ctx.set_batch_scratch(0)


class _CountLaunches:
    """The context's launch counter on the slot the panel kernels use (PGPS_K_FILTER_APPLY = 1); .launches() reads and resets."""

    def __init__(self):
        from pssgp import _backend as Bk
        self.ctx = Bk.get_context()
        self.name = self.ctx.lib.pgps_kernel_name(1).decode()

    def __enter__(self):
        self.ctx.profile_enable(2)
        self.ctx.profile_read(reset=True)
        return self

    def launches(self):
        return int(self.ctx.profile_read(reset=True)[self.name][1])

    def __exit__(self, *exc):
        self.ctx.profile_enable(0)
        self.ctx.profile_read(reset=True)


def _same_bits(a, b, what):
    assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64)), what


def _rows_equal(got, want, order, what):
    """Row order[j] of `want` (the panel in its own order) and row j of `got` (the panel in `order`) hold the same bits."""
    ll, pred, rows, qoffs = got
    w_ll, (w_mean, w_var, w_llp), w_rows, w_qoffs = want
    for j, i in enumerate(order):
        _same_bits(ll[j], w_ll[i], (what, "ll", i))
        _same_bits(rows[j], w_rows[i], (what, "gradient row", i))
        if pred is None:                # (the series without queries, alone)
            assert qoffs[-1] == 0
            continue
        mean, var, llp = pred
        _same_bits(llp[j], w_llp[i], (what, "predict ll", i))
        a, b = slice(qoffs[j], qoffs[j + 1]), slice(w_qoffs[i], w_qoffs[i + 1])
        _same_bits(mean[a], w_mean[b], (what, "mean", i))
        _same_bits(var[a], w_var[b], (what, "var", i))


@pytest.mark.parametrize("kname", KNAMES)
@HET
def test_a_row_depends_on_nothing_but_its_series(kname, het):
    cases = _panel(LENGTHS, QUERIES)
    S = len(cases)
    models = [_model(kname)]
    want = _calls(models, cases, het)
    _rows_equal(_calls(models, cases, het), want, range(S), "repeated")
    _rows_equal(_calls(models, cases, het, order=range(S - 1, -1, -1)), want, range(S - 1, -1, -1), "reversed")
    for i in range(S):
        _rows_equal(_calls(models, cases, het, order=[i]), want, [i], "alone")
    # a budget of one byte: no second series ever fits, every series is a group of its own -- S launches per call; and a
    # budget that holds a few of the series: groups of uneven size
    with _BatchScratch(1), _CountLaunches() as count:
        got = _calls(models, cases, het)
        n = count.launches()
    assert n == 3 * S, n
    _rows_equal(got, want, range(S), "one series per group")
    with _BatchScratch(300 * 1024), _CountLaunches() as count:
        got = _calls(models, cases, het)
        n = count.launches()
    print(f"{kname} rs {het}: {n} launches for three calls under a 300 KiB budget")
    _rows_equal(got, want, range(S), "a few series per group")


# ---- 4. per-series models ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@HET
def test_per_series_models(kname, het):
    cases = _panel(LENGTHS, QUERIES)
    S = len(cases)
    rng = np.random.RandomState(5)
    pars = [(rng.uniform(0.5, 2.0), rng.uniform(0.3, 1.0), rng.uniform(0.05, 0.3)) for _ in range(S)]
    models = [_model(kname, Rv, v, ell) for v, ell, Rv in pars]
    got = _calls(models, cases, het)
    _check_against_singles(got, lambda i: models[i], cases, het, f"{kname} rs {het} per-series models")
    # rows swapped (the table reversed) must move the results: the references themselves differ by far more than the tolerance
    for i in (0, 2):
        a, b = _single(models[i], cases[i], het)[0], _single(models[S - 1 - i], cases[i], het)[0]
        assert _rel_ll(a, b) > 1e4 * TOL, (i, a, b)
    swapped = _calls(models[::-1], cases, het)
    assert _rel_ll(swapped[0][0], got[0][0]) > 1e4 * TOL and _rel_ll(swapped[0][2], got[0][2]) > 1e4 * TOL
    # one shared row and S identical rows: the same bits
    _rows_equal(_calls([models[3]], cases, het), _calls([models[3]] * S, cases, het), range(S), "shared row")


# ---- 5. rs at missing rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
def test_rs_at_missing_rows_does_not_reach_the_arithmetic(kname):
    cases = _panel(LENGTHS, QUERIES)
    nan_cases = []
    for t, y, s, tq in cases:
        s = s.copy()
        s[np.isnan(y)] = np.nan
        nan_cases.append((t, y, s, tq))
    assert sum(int(np.isnan(c[2]).sum()) for c in nan_cases) > 100
    models = [_model(kname)]
    _rows_equal(_calls(models, nan_cases, True), _calls(models, cases, True), range(len(cases)), "NaN in rs at the missing rows")


# ---- 6. the ABI -----------------------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_abi_errors_and_device_forms():
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    lib = ctx.lib
    cases = _panel(LENGTHS, QUERIES)
    S = len(cases)
    offs, qoffs, ts, ys, rs, tq = _concat(cases, True)
    offs, qoffs = offs.astype(np.int64), qoffs.astype(np.int64)
    table, d = Bk._gp_rows([_model("m32")])
    tableS = np.ascontiguousarray(np.repeat(table, S, axis=0))
    K = int(qoffs[-1])
    ll, out = np.empty(S), np.empty((S, 2 + d * d + 2 * d))
    mean, var = np.empty(K), np.empty(K)

    def ll_call(S_=S, offs_=offs, d_=d, nm=1, table_=table, ts_=ts, ys_=ys, rs_=rs, ll_=ll, fn="pgps_gp_panel_ll_f64"):
        return getattr(lib, fn)(ctx.handle, S_, _p(offs_), d_, nm, _p(table_), _p(ts_), _p(ys_), _p(rs_), _p(ll_))

    def predict_call(qoffs_=qoffs, tq_=tq, mean_=mean, var_=var, ll_=ll, offs_=offs):
        return lib.pgps_gp_panel_predict_f64(ctx.handle, S, _p(offs_), _p(qoffs_), d, 1, _p(table), _p(ts), _p(ys), _p(rs), _p(tq_),
                                             _p(mean_), _p(var_), _p(ll_))

    def bad_row(col, value):
        t = table.copy()
        t[0, col] = value
        return t

    empty = offs.copy()
    empty[3] = empty[2]                                 # an empty series
    too_long = np.array([0, 2049], np.int64)
    no_queries = np.zeros(S + 1, np.int64)
    decreasing = qoffs.copy()
    decreasing[2] = decreasing[1] - 1
    over = qoffs.copy()
    over[1:] += 2048 - 257 - 50 + 1                     # series 0: one merged step above the limit
    invalid = {
        "S < 1": ll_call(S_=0), "offs null": ll_call(offs_=None), "models null": ll_call(table_=None), "ts null": ll_call(ts_=None),
        "ys null": ll_call(ys_=None), "ll null": ll_call(ll_=None), "out null": ll_call(ll_=None, fn="pgps_gp_panel_ll_grad_f64"),
        "an empty series": ll_call(offs_=empty), "a series above the limit": ll_call(S_=1, offs_=too_long),
        "nmodels not 1 or S": ll_call(nm=2, table_=tableS), "lam <= 0": ll_call(table_=bad_row(0, 0.0)),
        "R < 0": ll_call(table_=bad_row(-1, -0.1)), "R = 0 without rs": ll_call(table_=bad_row(-1, 0.0), rs_=None),
        "qoffs null": predict_call(qoffs_=None), "tq null": predict_call(tq_=None), "mean null": predict_call(mean_=None),
        "var null": predict_call(var_=None), "no query at all": predict_call(qoffs_=no_queries),
        "qoffs decreasing": predict_call(qoffs_=decreasing), "merged length above the limit": predict_call(qoffs_=over),
        "an empty series (predict)": predict_call(offs_=empty),
    }
    assert {k: v for k, v in invalid.items() if v != E_INVALID} == {}
    assert ll_call(d_=0) == E_UNSUPPORTED_DIM and ll_call(d_=4) == E_UNSUPPORTED_DIM
    # R = 0 is accepted with rs (R + rs[k] > 0), rs null and ll null are accepted by predict; the context still works
    assert ll_call(table_=bad_row(-1, 0.0)) == 0
    assert predict_call(ll_=None) == 0
    assert ll_call() == 0 and ll_call(nm=S, table_=tableS) == 0
    # the _dev forms on device pointers give the bits of the host forms (with and without rs)
    for rs_ in (rs, None):
        host = (Bk.gp_panel_ll(table, offs, ts, ys, rs_), Bk.gp_panel_predict(table, offs, qoffs, ts, ys, rs_, tq),
                Bk.gp_panel_ll_grad(table, offs, ts, ys, rs_))
        data = Bk.PanelData(offs, ts, ys, rs_)
        try:
            _same_bits(Bk.panel.gp_panel_ll_dev(data, table), host[0], "ll")
            for a, b in zip(Bk.panel.gp_panel_predict_dev(data, table, qoffs, tq), host[1]):
                _same_bits(a, b, "predict")
            _same_bits(Bk.panel.gp_panel_ll_grad_dev(data, table), host[2], "gradient rows")
        finally:
            data.close()


# ---- 7. the class on the device route ------------------------------------------------------------------------------------------
class _Spy:
    """Counts the calls of the _backend.panel wrappers and of the single-series entry points of _backend (restored on exit)."""
    PANEL = ("gp_panel_ll_dev", "gp_panel_ll_grad_dev", "gp_panel_predict_dev")
    SINGLE = ("gp", "gp_predict", "gp_ll_het", "gp_predict_het", "gp_ll_grad_adj_het", "gp_ll_grad")

    def __enter__(self):
        from pssgp import _backend as Bk
        self.calls, self._saved = [], []
        for mod, names in ((Bk.panel, self.PANEL), (Bk, self.SINGLE)):
            for name in names:
                fn = getattr(mod, name)
                self._saved.append((mod, name, fn))
                setattr(mod, name, self._wrap(name, fn))
        series_cls = Bk.Series
        for name in ("gp_ll", "gp_predict", "gp_ll_grad_adj", "gp_ll_grad_adj_raw", "gp_ll_grad"):
            fn = getattr(series_cls, name)
            self._saved.append((series_cls, name, fn))
            setattr(series_cls, name, self._wrap("Series." + name, fn))
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
        for mod, name, fn in self._saved:
            setattr(mod, name, fn)


def _kernel(kname, variance=1.0, ell=0.5):
    import pssgp.kernels as Kn
    return getattr(Kn, MATERNS[kname][0])(variance=variance, lengthscales=ell)


@pytest.mark.parametrize("kname", KNAMES)
@HET
def test_the_class_on_the_device_route(kname, het):
    from pssgp.model import StateSpaceGP
    from pssgp.panel import StateSpaceGPPanel
    cases = _panel(LENGTHS, QUERIES)
    S = len(cases)
    rng = np.random.RandomState(9)
    perms = [rng.permutation(c[0].size) for c in cases]
    obs = [c[2][p] for c, p in zip(cases, perms)] if het else None
    # input times out of order, queries out of order and repeated
    panel = StateSpaceGPPanel([(c[0][p], c[1][p]) for c, p in zip(cases, perms)], _kernel(kname), noise_variance=R,
                              observation_variances=obs)
    picks = [rng.randint(0, c[3].size, c[3].size + 3) if c[3].size else np.zeros(0, int) for c in cases]
    Xnews = [c[3][p] for c, p in zip(cases, picks)]
    with _Spy() as spy:
        lls = panel.log_likelihoods()
        assert spy.take() == ["gp_panel_ll_dev"]
        out = panel.predict_f(Xnews)
        assert spy.take() == ["gp_panel_predict_dev"]
        lls_g, grads = panel.log_likelihoods_and_grads()
        assert spy.take() == ["gp_panel_ll_grad_dev"]
        total, grad = panel.log_likelihood_and_grad()
        assert spy.take() == ["gp_panel_ll_grad_dev"]
    assert lls.shape == (S,) and grads.shape == (S, 3)
    assert abs(float(total) - np.sum(lls_g)) <= 1e-12 * abs(np.sum(lls_g))
    assert np.max(np.abs(grad - np.sum(grads, axis=0))) <= 1e-12 * np.max(np.abs(grad))
    assert abs(float(panel.maximum_log_likelihood_objective()) - np.sum(lls)) <= 1e-12 * abs(np.sum(lls))
    empty = panel.predict_f([np.zeros(0)] * S)
    assert all(m.shape == (0, 1) and v.shape == (0, 1) for m, v in empty)
    for i, (t, y, s, tq) in enumerate(cases):
        m = StateSpaceGP((t[:, None], y[:, None]), _kernel(kname), noise_variance=R, parallel=True,
                         observation_variances=s if het else None)
        w_obj = float(m.maximum_log_likelihood_objective())
        w_ll, w_g = m.log_likelihood_and_grad(method="adjoint")
        e = [_rel_ll(lls[i], w_obj), _rel_ll(lls_g[i], float(w_ll)), rel(grads[i], w_g)]
        assert out[i][0].shape == out[i][1].shape == (Xnews[i].size, 1)
        if tq.size:
            w_mean, w_var = m.predict_f(tq[:, None])
            e += [rel(out[i][0][:, 0], w_mean[picks[i], 0]), rel(out[i][1][:, 0], w_var[picks[i], 0])]
        print(f"{kname} rs {het} series {i}: the class against StateSpaceGP alone " + " ".join(f"{x:.2e}" for x in e))
        assert max(e) <= TOL, (i, e)
    # per-series thetas: row s is the single model with row s assigned; the panel's own parameters are untouched
    thetas = np.stack([rng.uniform(0.5, 2.0, S), rng.uniform(0.3, 1.0, S), rng.uniform(0.05, 0.3, S)], axis=1)
    lls_t, grads_t = panel.log_likelihoods_and_grads(thetas)
    for i in (0, 2, 5):
        t, y, s, _ = cases[i]
        m = StateSpaceGP((t[:, None], y[:, None]), _kernel(kname, thetas[i, 0], thetas[i, 1]), noise_variance=thetas[i, 2],
                         parallel=True, observation_variances=s if het else None)
        m.maximum_log_likelihood_objective()
        w_ll, w_g = m.log_likelihood_and_grad(method="adjoint")
        assert _rel_ll(lls_t[i], float(w_ll)) <= TOL and rel(grads_t[i], w_g) <= TOL
    assert (float(panel.kernel.variance), float(panel.kernel.lengthscales), panel.noise_variance) == (1.0, 0.5, R)


def test_a_long_series_leaves_the_panel_call():
    from pssgp.model import StateSpaceGP
    from pssgp.panel import StateSpaceGPPanel
    cases = _panel((37, 3000, 300), (4, 20, 0))
    panel = StateSpaceGPPanel([(c[0], c[1]) for c in cases], _kernel("m32"), noise_variance=R)
    with _Spy() as spy:
        lls = panel.log_likelihoods()
        calls = spy.take()
        assert calls.count("gp_panel_ll_dev") == 1 and len(calls) == 2, calls      # (one panel call, one single-series call)
        out = panel.predict_f([c[3] for c in cases])
        calls = spy.take()
        assert calls.count("gp_panel_predict_dev") == 1 and len(calls) == 2, calls
    for i, (t, y, _, tq) in enumerate(cases):
        m = StateSpaceGP((t[:, None], y[:, None]), _kernel("m32"), noise_variance=R, parallel=True)
        assert _rel_ll(lls[i], float(m.maximum_log_likelihood_objective())) <= TOL
        assert out[i][0].shape == (tq.size, 1)
        if tq.size:
            w_mean, w_var = m.predict_f(tq[:, None])
            assert rel(out[i][0], w_mean) <= TOL and rel(out[i][1], w_var) <= TOL
