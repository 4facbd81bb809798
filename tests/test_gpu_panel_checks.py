"""GPU tests of the panel's predictive checks (pgps_gp_panel_loo_*) and of StateSpaceGPPanel's
one_step_ahead / leave_one_out / loo_log_predictive_densities on the device route: the one-step-ahead and leave-one-out laws of
every row of S series, one workgroup per series, scalar noise and per-observation variances.  ctypes -> C ABI.
Data: het_refs.series with a different seed per series (a read from a neighbour's rows moves a result), 20 % of y missing.
References (none is the code under test): loo_refs.ss_checks (numpy filter + smoother with a per-step R, then the cavity
formula) at loo_refs.TOL = 1e-9, loo_refs.dense_checks at the zoo's 1e-6, the single-series device call _backend.gp_loo at
1e-9 (scalar noise), the loop of StateSpaceGP models at 1e-9 (class level).  Every case asserts from the numpy reference, before
the device is touched, that the cavity subtraction is benign: (R_k - v) / R_k >= 0.05."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import loo_refs
from loo_refs import FIELDS, MATERNS, R, TOL, dense_checks, err, sde_of, series, ss_checks

pytestmark = pytest.mark.gpu

KNAMES = ("m12", "m32", "m52")
HET = pytest.mark.parametrize("het", [False, True], ids=["scalar", "rs"])
# odd sizes, one and two rows, a multiple of the 256 lanes and its two neighbours
LENGTHS = (257, 1, 700, 37, 256, 2, 255)
MIN_GAP = 0.05
E_INVALID, E_UNSUPPORTED_DIM, E_NUMERIC = -1, -2, -5


def _model(kname, Rv=R, variance=1.0, ell=0.5):
    import pssgp.kernels as Kn
    from pssgp import _backend as Bk
    sde = getattr(Kn, MATERNS[kname][0])(variance=variance, lengthscales=ell).get_sde()
    return (Bk.nilpotent_form(sde.F), np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1), Rv)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _panel(lengths, first_seed=0):
    """((t, y, s),) of the panel's series, read-only; series i has seed first_seed + i."""
    return tuple(_frozen(*series(n, seed=first_seed + i)) for i, n in enumerate(lengths))


def _concat(cases, het):
    offs = np.concatenate([[0], np.cumsum([c[0].size for c in cases])]).astype(np.int64)
    cat = lambda j: np.concatenate([c[j] for c in cases])
    return offs, cat(0), cat(1), (cat(2) if het else None)


def _call(models, cases, het, **kw):
    from pssgp import _backend as Bk
    offs, ts, ys, rs = _concat(cases, het)
    out = Bk.gp_panel_loo(models, offs, ts, ys, rs, **kw)
    assert Bk.get_context().status() == 0                   # (the status word is clean after every accepted call)
    out["offs"] = offs
    return out


def _row(out, i):
    """The dict of series i cut out of a panel result."""
    a, b = out["offs"][i], out["offs"][i + 1]
    cut = {k: v[a:b] for k, v in out.items() if k not in ("ll", "loo_lpd", "offs")}
    cut["ll"], cut["loo_lpd"] = out["ll"][i], out["loo_lpd"][i]
    return cut


_REF_CACHE = {}


def _refs(kname, case, het, Rv=R):
    """(state-space reference, dense reference) of one series, computed once per (kernel, data, noise); the gap of the cavity
    subtraction is asserted here, from numpy alone."""
    t, y, s = case
    key = (kname, t.tobytes(), y.tobytes(), s.tobytes() if het else None, Rv)
    if key not in _REF_CACHE:
        Rk = Rv + s if het else Rv
        ss = ss_checks(sde_of(kname), t, y, Rk)
        assert ss["gap"] >= MIN_GAP, (kname, t.size, het, ss["gap"])
        _REF_CACHE[key] = (ss, dense_checks(MATERNS[kname][1], t, y, Rk))
    return _REF_CACHE[key]


def _rel(a, b):
    return abs(a - b) / abs(b)


def _gaps(got, kname, case, het, Rv=R):
    """(largest error against the state-space reference: four arrays, two sums, the two per-row log densities at the observed
    rows; against the dense one at the observed rows).  The log densities must be NaN exactly at the NaN rows of y."""
    ss, dn = _refs(kname, case, het, Rv)
    obs = ~np.isnan(case[1])
    e_ss = [err(got[f], ss[f]) for f in FIELDS] + [_rel(got[k], ss[k]) for k in ("ll", "loo_lpd")]
    for name in ("osa_log_density", "loo_log_density"):
        assert np.array_equal(np.isnan(got[name]), ~obs), name
        e_ss.append(err(got[name][obs], ss[name][obs]))
    e_dn = [err(np.asarray(got[f])[obs], dn[f]) for f in FIELDS] + [_rel(got[k], dn[k]) for k in ("ll", "loo_lpd")]
    return max(e_ss), max(e_dn)


def _check_panel(out, kname, cases, het, what, model_of=None):
    """Every series of a panel result against both references (and, scalar noise, against _backend.gp_loo on it alone)."""
    from pssgp import _backend as Bk
    worst = [0.0, 0.0, 0.0]
    for i, case in enumerate(cases):
        got = _row(out, i)
        e_ss, e_dn = _gaps(got, kname, case, het)
        e_one = 0.0
        if not het:
            form, P, H, Rv = model_of(i) if model_of else _model(kname)
            one = Bk.gp_loo(form, P, H, Rv, case[0], case[1])
            e_one = max([err(got[f], one[f]) for f in FIELDS] + [_rel(got[k], one[k]) for k in ("ll", "loo_lpd")])
        print(f"{what} series {i} (n {case[0].size}): state-space {e_ss:.2e} (bound {TOL:.0e}), dense {e_dn:.2e} "
              f"(bound {MATERNS[kname][2]:.0e}), single-series call {e_one:.2e} (bound {TOL:.0e})")
        worst = [max(w, e) for w, e in zip(worst, (e_ss, e_dn, e_one))]
    assert worst[0] <= TOL and worst[1] <= MATERNS[kname][2] and worst[2] <= TOL, (what, worst)


# ---- 1. geometry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@HET
def test_geometry_against_the_references_and_the_single_series_call(kname, het):
    from pssgp import _backend as Bk
    cases = _panel(LENGTHS)
    for case in cases:
        _refs(kname, case, het)                             # (the gaps, before the device is touched)
    out = _call([_model(kname)], cases, het)
    n = int(out["offs"][-1])
    assert out["ll"].shape == out["loo_lpd"].shape == (len(cases),)
    assert all(out[f].shape == (n,) for f in FIELDS + ("osa_log_density", "loo_log_density"))
    _check_panel(out, kname, cases, het, f"{kname} rs {het}")
    # the one-step-ahead log densities of the observed rows sum to the panel's log-likelihoods
    offs, ts, ys, rs = _concat(cases, het)
    ll = Bk.gp_panel_ll([_model(kname)], offs, ts, ys, rs)
    worst = 0.0
    for i in range(len(cases)):
        total = float(np.nansum(_row(out, i)["osa_log_density"]))
        worst = max(worst, _rel(total, ll[i]), _rel(out["ll"][i], ll[i]))
    print(f"{kname} rs {het}: one-step-ahead log densities summed against gp_panel_ll {worst:.2e} (bound 1e-10)")
    assert worst <= 1e-10


# ---- 2. a full workgroup and the limit -----------------------------------------------------------------------------------------
class _Chunk:
    """pgps_set_chunk for the block, restored on every exit."""

    def __init__(self, steps):
        from pssgp import _backend as Bk
        self.ctx, self.steps = Bk.get_context(), steps

    def __enter__(self):
        self.ctx.set_chunk(self.steps)

    def __exit__(self, *exc):
        self.ctx.set_chunk(0)


@pytest.mark.parametrize("kname,het", [("m12", True), ("m32", False), ("m52", True), ("m52", False)])
def test_a_full_workgroup_and_the_limit(kname, het):
    """1024 and 2048 rows: four and eight steps per lane on all 256 lanes, the LDS-staged road of the Kalman pass and of the
    smoother's loads (2048 is the limit; one row more is refused).  With them in the panel: a run of missing rows 252..260
    across lane-chunk boundaries (n = 1024: lanes of four steps) and a series with repeated times."""
    from pssgp import _backend as Bk
    run = _frozen(*series(1024, seed=21, run=(252, 9)))
    assert np.all(np.isnan(run[1][252:261]))
    rep = _frozen(*loo_refs.repeated_times(300))
    cases = _panel((1024, 2048), 11) + (run, rep)
    for case in cases:
        _refs(kname, case, het)
    _check_panel(_call([_model(kname)], cases, het), kname, cases, het, f"{kname} rs {het} full workgroups")
    over = _panel((3, 2049), 11)
    offs, ts, ys, rs = _concat(over, het)
    with pytest.raises(Bk.PgpsError) as bad:
        Bk.gp_panel_loo([_model(kname)], offs, ts, ys, rs)
    assert bad.value.code == E_INVALID


@pytest.mark.parametrize("kname,het", [("m12", False), ("m32", True), ("m52", True)])
@pytest.mark.parametrize("chunk", [3, 1])
def test_pinned_chunks(kname, het, chunk):
    """n = 700 under pgps_set_chunk(3) -- the chunk covers the series and is no whole sub-tile of four steps: direct stores --
    and under pgps_set_chunk(1), which does not cover it: the series takes its own three steps per lane.  A 37-row neighbour
    takes the pinned chunk in both."""
    cases = _panel((700, 37), 31)
    for case in cases:
        _refs(kname, case, het)
    free = _call([_model(kname)], cases, het)
    with _Chunk(chunk):
        out = _call([_model(kname)], cases, het)
    _check_panel(out, kname, cases, het, f"{kname} rs {het} chunk {chunk}")
    if chunk == 1:          # (series 0: its own steps per lane, as without a pinned chunk)
        for f in FIELDS:
            _same_bits(_row(out, 0)[f], _row(free, 0)[f], f)


# ---- 3. a row depends on nothing but its series, bit for bit -------------------------------------------------------------------
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
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


def _rows_equal(got, want, order, what):
    """Series order[j] of `want` and series j of `got` hold the same bits: four arrays and both sums."""
    for j, i in enumerate(order):
        g, w = _row(got, j), _row(want, i)
        for k in FIELDS + ("ll", "loo_lpd"):
            _same_bits(g[k], w[k], (what, k, i))


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _raw(table, d, offs, ts, ys, rs, keep=(True, True, True, True), fn="pgps_gp_panel_loo_f64", over=()):
    """The C entry point itself: (code, the four arrays or None where not asked for, sums)."""
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    S, n = offs.size - 1, int(offs[-1])
    arrays = [np.full(n, 7.0) if k else None for k in keep]
    sums = np.full((S, 2), 7.0)
    a = dict(S=S, offs=offs, d=d, nm=table.shape[0], table=table, ts=ts, ys=ys, rs=rs, sums=sums)
    a.update(over)              # (what a rejected call is given instead; the outputs keep the sizes of the valid call)
    code = getattr(ctx.lib, fn)(ctx.handle, a["S"], _p(a["offs"]), a["d"], a["nm"], _p(a["table"]), _p(a["ts"]), _p(a["ys"]),
                                _p(a["rs"]), *(_p(x) for x in arrays), _p(a["sums"]))
    return code, arrays, sums


@pytest.mark.parametrize("kname", KNAMES)
@HET
def test_a_row_depends_on_nothing_but_its_series(kname, het):
    from pssgp import _backend as Bk
    cases = _panel(LENGTHS)
    S = len(cases)
    models = [_model(kname)]
    want = _call(models, cases, het)
    pick = lambda order: [cases[i] for i in order]
    _rows_equal(_call(models, cases, het), want, range(S), "called again")
    last = [0, 1, 2, 3, 5, 6, 4]                             # the 256-row series last: row n of its view is past the arrays
    _rows_equal(_call(models, pick(last), het), want, last, "the 256-row series last")
    twice = [2, 0, 2, 4, 4]
    _rows_equal(_call(models, pick(twice), het), want, twice, "series repeated")
    # a changed neighbour: other data on both sides of series 2 and 4
    other = _panel(LENGTHS, 50)
    mixed = [other[0], other[1], cases[2], other[3], cases[4], other[5], other[6]]
    got = _call(models, mixed, het)
    for j in (2, 4):
        for k in FIELDS + ("ll", "loo_lpd"):
            _same_bits(_row(got, j)[k], _row(want, j)[k], ("a changed neighbour", k, j))
    assert not np.array_equal(_row(got, 0)["loo_mean"], _row(want, 0)["loo_mean"])
    # a budget of one byte: every series is a group of its own -- S launches; a budget that holds a few: groups of uneven size
    with _BatchScratch(1), _CountLaunches() as count:
        got = _call(models, cases, het)
        n = count.launches()
    assert n == S, n
    _rows_equal(got, want, range(S), "one series per group")
    # (a series' scan records alone are 256 lanes x about 8, 23 and 45 doubles at d = 1, 2, 3: the budget follows d^2)
    budget = 64 * 1024 * len(models[0][2]) ** 2
    with _BatchScratch(budget), _CountLaunches() as count:
        got = _call(models, cases, het)
        n = count.launches()
    print(f"{kname} rs {het}: {n} launches under a {budget // 1024} KiB budget, {S} series")
    assert 1 < n < S, n
    _rows_equal(got, want, range(S), "a few series per group")
    # every subset of the four arrays null: the sums and the remaining arrays keep their bits, a null array is not touched
    offs, ts, ys, rs = _concat(cases, het)
    table, d = Bk._gp_rows(models)
    for keep in itertools.product((True, False), repeat=4):
        code, arrays, sums = _raw(table, d, offs, ts, ys, rs, keep)
        assert code == 0, (keep, code)
        _same_bits(sums[:, 0], want["ll"], ("ll", keep))
        _same_bits(sums[:, 1], want["loo_lpd"], ("loo_lpd", keep))
        for f, a in zip(FIELDS, arrays):
            if a is not None:
                _same_bits(a, want[f], (f, keep))
    assert Bk.get_context().status() == 0


# ---- 4. rs at missing rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
def test_rs_at_missing_rows_reaches_the_two_variances_of_those_rows_alone(kname):
    cases = _panel(LENGTHS)
    nan_cases = []
    for t, y, s in cases:
        s = s.copy()
        s[np.isnan(y)] = np.nan
        nan_cases.append((t, y, s))
    models = [_model(kname)]
    fin, nan = _call(models, cases, True), _call(models, nan_cases, True)
    missing = np.isnan(np.concatenate([c[1] for c in cases]))
    assert int(missing.sum()) > 100
    for k in ("ll", "loo_lpd", "osa_mean", "loo_mean"):
        _same_bits(nan[k], fin[k], k)
    worst = 0.0
    for k in ("osa_var", "loo_var"):
        _same_bits(nan[k][~missing], fin[k][~missing], k)
        assert np.all(np.isnan(nan[k][missing])) and np.all(np.isfinite(fin[k][missing]))
        # finite values there: ... + R + rs[k] as stored, against the reference
        for i, case in enumerate(cases):
            m = np.isnan(case[1])
            if m.any():
                worst = max(worst, err(_row(fin, i)[k][m], _refs(kname, case, True)[0][k][m]))
    print(f"{kname}: the variances at the missing rows against the state-space reference {worst:.2e} (bound {TOL:.0e})")
    assert worst <= TOL


# ---- 5. constant rs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
def test_constant_rs_is_the_scalar_call_at_the_sum(kname):
    cases = _panel(LENGTHS)
    c = 0.05
    const = [(t, y, np.full(t.size, c)) for t, y, _ in cases]
    for case in cases:
        _refs(kname, case, False, R + c)
    het = _call([_model(kname, R)], const, True)
    scalar = _call([_model(kname, R + c)], cases, False)
    worst, equal = 0.0, True
    for k in FIELDS + ("ll", "loo_lpd"):
        worst = max(worst, err(het[k], scalar[k]))
        equal = equal and np.array_equal(het[k].view(np.uint64), scalar[k].view(np.uint64))
    print(f"{kname}: rs = {c} with noise {R} against the scalar call at {R + c}: {worst:.2e} (bound {TOL:.0e}); bits equal: {equal}")
    assert worst <= TOL
    for i, case in enumerate(cases):
        e_ss, e_dn = _gaps(_row(het, i), kname, case, False, R + c)
        assert e_ss <= TOL and e_dn <= MATERNS[kname][2], (i, e_ss, e_dn)


# ---- 6. per-series models ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@HET
def test_per_series_models(kname, het):
    cases = _panel(LENGTHS)
    S = len(cases)
    rng = np.random.RandomState(5)
    pars = [(rng.uniform(0.5, 2.0), rng.uniform(0.3, 1.0), rng.uniform(0.08, 0.3)) for _ in range(S)]
    models = [_model(kname, Rv, v, ell) for v, ell, Rv in pars]
    got = _call(models, cases, het)
    # every series against the numpy reference at ITS row of the table
    import pssgp.kernels as Kn
    worst = 0.0
    for i, ((t, y, s), (v, ell, Rv)) in enumerate(zip(cases, pars)):
        sde = getattr(Kn, MATERNS[kname][0])(variance=v, lengthscales=ell).get_sde()
        ss = ss_checks(sde, t, y, Rv + s if het else Rv)
        assert ss["gap"] >= MIN_GAP, (i, ss["gap"])
        g = _row(got, i)
        worst = max([worst] + [err(g[f], ss[f]) for f in FIELDS] + [_rel(g[k], ss[k]) for k in ("ll", "loo_lpd")])
    print(f"{kname} rs {het}: per-series models against the state-space reference {worst:.2e} (bound {TOL:.0e})")
    assert worst <= TOL
    # swapping two rows of the table moves exactly those two series' results
    a, b = 2, 4
    swapped = list(models)
    swapped[a], swapped[b] = models[b], models[a]
    moved = _call(swapped, cases, het)
    for i in range(S):
        for k in FIELDS + ("ll", "loo_lpd"):
            same = np.array_equal(np.asarray(_row(moved, i)[k]).view(np.uint64), np.asarray(_row(got, i)[k]).view(np.uint64))
            assert same == (i not in (a, b)), (i, k)
    # one shared row and S identical rows: the same bits
    _rows_equal(_call([models[3]], cases, het), _call([models[3]] * S, cases, het), range(S), "shared row")


# ---- 7. the ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_rejections_and_device_form():
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    cases = _panel(LENGTHS)
    S = len(cases)
    offs, ts, ys, rs = _concat(cases, True)
    table, d = Bk._gp_rows([_model("m32")])
    tableS = np.ascontiguousarray(np.repeat(table, S, axis=0))

    def bad_row(col, value):
        t = table.copy()
        t[0, col] = value
        return t

    def bad_rs(value, observed=True):
        r = rs.copy()
        r[np.flatnonzero(~np.isnan(ys) if observed else np.isnan(ys))[40]] = value
        return r

    empty = offs.copy()
    empty[3] = empty[2]
    call = lambda **over: _raw(table, d, offs, ts, ys, rs, over=over)[0]
    dev = Bk.PanelData(offs, ts, ys, rs)
    try:
        n = int(offs[-1])
        dres = dev._buffer("checks", 8 * (2 * S + 4 * n))
        dptr = [dres + 8 * (2 * S + i * n) for i in range(4)]

        def dev_call(**over):
            a = dict(S=S, offs=offs, d=d, nm=1, table=table, ts=dev.ts, ys=dev.ys, rs=dev.rs, sums=dres)
            a.update(over)
            return ctx.lib.pgps_gp_panel_loo_dev_f64(ctx.handle, a["S"], _p(a["offs"]), a["d"], a["nm"], _p(a["table"]), a["ts"],
                                                     a["ys"], a["rs"], *dptr, a["sums"])

        for name, fn in (("host", call), ("dev", dev_call)):
            invalid = {
                "S < 1": fn(S=0), "offs null": fn(offs=None), "models null": fn(table=None), "ts null": fn(ts=None),
                "ys null": fn(ys=None), "sums null": fn(sums=None), "an empty series": fn(offs=empty),
                "a series above the limit": fn(S=1, offs=np.array([0, 2049], np.int64)),
                "nmodels not 1 or S": fn(nm=2, table=tableS), "lam <= 0": fn(table=bad_row(0, 0.0)),
                "R < 0": fn(table=bad_row(-1, -0.1)), "R = 0 without rs": fn(table=bad_row(-1, 0.0), rs=None),
            }
            assert {k: v for k, v in invalid.items() if v != E_INVALID} == {}, name
            assert fn(d=0) == E_UNSUPPORTED_DIM and fn(d=4) == E_UNSUPPORTED_DIM, name
        # the host form's scan of rs: finite and R + rs[k] > 0 at the observed rows; a missing row is not looked at
        assert call(rs=bad_rs(np.nan)) == E_INVALID and call(rs=bad_rs(np.inf)) == E_INVALID
        assert call(rs=bad_rs(-2.0 * R)) == E_INVALID
        assert call(table=bad_row(-1, 0.0), rs=bad_rs(0.0)) == E_INVALID
        assert call(rs=bad_rs(np.nan, observed=False)) == 0
        # a non-finite sum (a NaN time in one series): PGPS_E_NUMERIC from the host form
        t_nan = ts.copy()
        t_nan[offs[3] + 5] = np.nan
        assert call(ts=t_nan) == E_NUMERIC
        ctx.status()
        # accepted: R = 0 with rs, S rows of models; the status word is clean after every accepted call
        for ok in (call(), call(table=bad_row(-1, 0.0)), call(nm=S, table=tableS), dev_call(), dev_call(nm=S, table=tableS)):
            assert ok == 0
            assert ctx.status() == 0
        # the _dev form on device pointers gives the bits of the host form (with and without rs, with and without arrays)
        for rs_ in (rs, None):
            host = Bk.gp_panel_loo(table, offs, ts, ys, rs_)
            data = Bk.PanelData(offs, ts, ys, rs_)
            try:
                got = Bk.panel.gp_panel_loo_dev(data, table)
                for k in FIELDS + ("ll", "loo_lpd", "osa_log_density", "loo_log_density"):
                    _same_bits(got[k], host[k], ("dev", k))
                only = Bk.panel.gp_panel_loo_dev(data, table, osa=False, loo=True)
                assert "osa_mean" not in only and "osa_log_density" not in only
                _same_bits(only["loo_var"], host["loo_var"], "loo alone")
                none = Bk.panel.gp_panel_loo_dev(data, table, osa=False, loo=False)
                assert sorted(none) == ["ll", "loo_lpd"]
                _same_bits(none["ll"], host["ll"], "ll alone")
                _same_bits(none["loo_lpd"], host["loo_lpd"], "loo_lpd alone")
            finally:
                data.close()
        assert ctx.status() == 0
    finally:
        dev.close()


# ---- 8. the class on the device route ------------------------------------------------------------------------------------------
class _Spy:
    """Records the calls of _backend.panel.gp_panel_loo_dev (with its osa / loo flags), of the single model's _checks, and the
    sizes of the device-to-host copies (restored on exit)."""

    def __enter__(self):
        from pssgp import _backend as Bk
        from pssgp.checks import ModelChecks
        from pssgp._backend.context import Context
        self.calls, self.copies = [], []
        self._saved = [(Bk.panel, "gp_panel_loo_dev", Bk.panel.gp_panel_loo_dev), (ModelChecks, "_checks", ModelChecks._checks),
                       (Context, "d2h", Context.d2h)]
        panel_fn, single_fn, d2h = (s[2] for s in self._saved)

        def panel_call(data, models, osa=True, loo=True):
            self.calls.append(("gp_panel_loo_dev", osa, loo))
            return panel_fn(data, models, osa=osa, loo=loo)

        def single_call(model, osa, loo):
            self.calls.append(("single", model.data[0].shape[0]))
            return single_fn(model, osa, loo)

        def copy(ctx, arr, dptr):
            self.copies.append(arr.nbytes)
            return d2h(ctx, arr, dptr)

        Bk.panel.gp_panel_loo_dev, ModelChecks._checks, Context.d2h = panel_call, single_call, copy
        return self

    def take(self):
        out, self.calls, self.copies = (self.calls, self.copies), [], []
        return out

    def __exit__(self, *exc):
        for owner, name, fn in self._saved:
            setattr(owner, name, fn)


def _kernel(kname, variance=1.0, ell=0.5):
    import pssgp.kernels as Kn
    return getattr(Kn, MATERNS[kname][0])(variance=variance, lengthscales=ell)


CLASS_LENGTHS = (257, 1, 300, 37, 2)


@pytest.mark.parametrize("kname", KNAMES)
@HET
def test_the_class_on_the_device_route(kname, het):
    from pssgp.model import StateSpaceGP
    from pssgp.panel import StateSpaceGPPanel
    cases = _panel(CLASS_LENGTHS, 70)
    S = len(cases)
    n_all = sum(CLASS_LENGTHS)
    rng = np.random.RandomState(9)
    perms = [rng.permutation(c[0].size) for c in cases]
    obs = [c[2][p] for c, p in zip(cases, perms)] if het else None
    # input times out of order: rows come back in input order
    panel = StateSpaceGPPanel([(c[0][p], c[1][p]) for c, p in zip(cases, perms)], _kernel(kname), noise_variance=R,
                              observation_variances=obs)
    with _Spy() as spy:
        osa = panel.one_step_ahead()
        assert spy.take() == ([("gp_panel_loo_dev", True, False)], [8 * (2 * S + 2 * n_all)])
        loo = panel.leave_one_out()
        assert spy.take() == ([("gp_panel_loo_dev", False, True)], [8 * (2 * S + 2 * n_all)])
        lpd = panel.loo_log_predictive_densities()
        assert spy.take() == ([("gp_panel_loo_dev", False, False)], [8 * 2 * S])      # (no per-row array is copied)
        total = panel.loo_log_predictive_density()
        assert spy.take() == ([("gp_panel_loo_dev", False, False)], [8 * 2 * S])
    assert lpd.shape == (S,) and abs(float(total) - np.sum(lpd)) <= 1e-12 * abs(np.sum(lpd))
    worst, worst_sum = 0.0, 0.0
    for i, ((t, y, s), p) in enumerate(zip(cases, perms)):
        m = StateSpaceGP((t[:, None], y[:, None]), _kernel(kname), noise_variance=R, parallel=True,
                         observation_variances=s if het else None)
        obs_rows = ~np.isnan(y[p])
        for got, want in ((osa[i], m.one_step_ahead()), (loo[i], m.leave_one_out())):
            for g, w, part in zip(got, want, ("mean", "var", "log_density")):
                assert g.shape == (t.size, 1) and g.dtype == w.dtype
                if part == "log_density":
                    assert np.array_equal(np.isnan(g[:, 0]), ~obs_rows)
                    worst = max(worst, err(g[obs_rows, 0], w[p][obs_rows, 0]))
                else:
                    worst = max(worst, err(g[:, 0], w[p][:, 0]))
        worst = max(worst, _rel(lpd[i], float(m.loo_log_predictive_density())))
        worst_sum = max(worst_sum, _rel(float(np.nansum(loo[i][2])), lpd[i]))
    print(f"{kname} rs {het}: the class against the loop of StateSpaceGP models {worst:.2e} (bound {TOL:.0e}); the scores against "
          f"the sums of leave_one_out()'s log densities {worst_sum:.2e} (bound 1e-12)")
    assert worst <= TOL and worst_sum <= 1e-12
    # per-series thetas: row s is the single model with row s assigned; the panel's own parameters are left as they were
    thetas = np.stack([rng.uniform(0.5, 2.0, S), rng.uniform(0.3, 1.0, S), rng.uniform(0.08, 0.3, S)], axis=1)
    loo_t, lpd_t = panel.leave_one_out(thetas), panel.loo_log_predictive_densities(thetas)
    for i in (0, 2, 4):
        t, y, s = cases[i]
        m = StateSpaceGP((t[:, None], y[:, None]), _kernel(kname, thetas[i, 0], thetas[i, 1]), noise_variance=thetas[i, 2],
                         parallel=True, observation_variances=s if het else None)
        want = m.leave_one_out()
        assert err(loo_t[i][0][:, 0], want[0][perms[i], 0]) <= TOL and err(loo_t[i][1][:, 0], want[1][perms[i], 0]) <= TOL
        assert _rel(lpd_t[i], float(m.loo_log_predictive_density())) <= TOL
    assert (float(panel.kernel.variance), float(panel.kernel.lengthscales), panel.noise_variance) == (1.0, 0.5, R)
    # the single model's errors
    with pytest.raises(ValueError):
        bad = thetas.copy()
        bad[1, 2] = 0.0 if not het else -1.0
        panel.leave_one_out(bad)
    assert panel.noise_variance == R


@HET
def test_a_long_series_is_spliced_back_from_its_own_model(het):
    from pssgp.model import StateSpaceGP
    from pssgp.panel import StateSpaceGPPanel
    cases = _panel((37, 2100, 300), 90)
    obs = [c[2] for c in cases] if het else None
    panel = StateSpaceGPPanel([(c[0], c[1]) for c in cases], _kernel("m32"), noise_variance=R, observation_variances=obs)
    with _Spy() as spy:
        loo = panel.leave_one_out()
        calls, _ = spy.take()
        assert calls == [("gp_panel_loo_dev", False, True), ("single", 2100)], calls
        lpd = panel.loo_log_predictive_densities()
        calls, _ = spy.take()
        assert calls == [("gp_panel_loo_dev", False, False), ("single", 2100)], calls
    worst = 0.0
    for i, (t, y, s) in enumerate(cases):
        m = StateSpaceGP((t[:, None], y[:, None]), _kernel("m32"), noise_variance=R, parallel=True,
                         observation_variances=s if het else None)
        want = m.leave_one_out()
        assert loo[i][0].shape == (t.size, 1)
        worst = max(worst, err(loo[i][0], want[0]), err(loo[i][1], want[1]), _rel(lpd[i], float(m.loo_log_predictive_density())))
    print(f"rs {het}: a panel with a 2100-row series against the loop of StateSpaceGP models {worst:.2e} (bound {TOL:.0e})")
    assert worst <= TOL
