"""GPU tests of the batched fused entry points -- pgps_gp_ll_batch_* (DESIGN.md 4g), pgps_gp_predict_batch_* (4q),
pgps_gp_ll_grad_adj_batch_* (4r) -- at the launch geometries where the carry crosses workgroups, on data that REMEMBERS.

The batched kernels run the single call's bodies behind gp_batch_select / gp_adj_batch_select; their own are the per-model
slices of the scan records, moments and kept states, the (workgroups, models) grids, the rule batch_steps_per_lane, the group
loop and form 1 of the predict.  They never take the forgetting shortcut: every workgroup folds the records of all workgroups
before (Kalman pass) or after (smoother) its own.  On data that forgets every term of that fold but the nearest is nil, so
a wrong slice, stride or fold length beyond the nearest record moves nothing; here, in every launch, some rows' carries are
made of several workgroups' records (their totals remember) and others' are not (they forget), both asserted FROM THE
REFERENCE before the device is touched (het_refs.workgroup_forgetting: log2 max|A|, log2 max|E| of each workgroup total;
remembers >= -60, forgets <= -120; nothing in these kernels branches on a threshold, the bands only prove the two kinds of
row are there).

Shapes (batch_refs.SHAPES: N, pgps_set_chunk, spacing; K = 50 queries of het_refs.queries -- one before, one after the series,
ties; 20 % of the rows NaN), each read back through pgps_get_batch_chunk for N and N + K and held to the table:
  P1  2600, 4, 2e-4   three workgroups of 1024; the last has staged, ragged and empty waves; rows 1020..1029 missing
  P2  4696, 8, 2e-4   three workgroups of 2048, two sub-tiles per lane
  P3  5000, 1, 2e-4   twenty workgroups of 256 steps, unstaged: the carry of the last is a fold over nineteen records
  P4  2600, 3, 2e-4   unstaged at three steps per lane, four workgroups
  P5  9000, 16, 2e-4  three workgroups of 4096, four sub-tiles per lane
  P6  6744, 8, 0.05 with rows 2048..4095 at 2e-4: only workgroup 1 remembers, between forgetting ones
  P7  5000, 0, 0.05   the default rule with B = 6 (7 for Matern-1/2): 4 steps per lane, five workgroups; everything forgets
  AUTO16 / AUTO8  7680 + 512 queries on the 2e-4 grid with B = 512 / 256: the rule's own 16 / 8 steps per lane
Which totals are held to the remembering band: every interior workgroup (P1 .. P5, AUTO8); workgroup 1 alone at P6, where
workgroup 2 must forget; none at P7 (the grid forgets whatever the setting).  With two workgroups (AUTO16) there is no interior
one: the data's totals A of both and E of the first are held to the band.  The one exception: Matern-1/2 at a span of 4096
steps (P5, AUTO16), where no allowed setting remembers (its best, (0.4, 2.5, 0.5), has log2 max|A| = -61): there the
rememberer is asserted for Matern-3/2 and -5/2 only.

Settings (variance, lengthscale, R): batch_refs.SETTINGS, and (0.4, 2.5, 0.5) for Matern-1/2.  Bounds: the project's 1e-9,
max norm relative to the largest entry (het_refs.rel) for mean, variance and adjoints, 1e-9 relative for ll.

Two things about the data and the reference (batch_refs.py).  The times of het_refs.spaced_series are moved by 0.1: on the
2e-4 grid the query 0.07 before the first training time would otherwise lie before the call's start time 0, a first step of
negative length.  And O.get_ssm's process noise is replaced by Pinf - F_k Pinf F_k^T on steps longer than a lengthscale
(lam dt > 1), where the reference's 2d x 2d matrix exponential has lost it: before that repair the rows at lengthscales
0.005 and 0.001 missed 1e-9 by far (Matern-5/2 at P1: ll 2.4e-6, variance 1.0 of the largest entry), the single call gp_predict
had the batch's bits (test 7), and the dense GP sided with the device; after it the reference agrees with the dense GP to
1e-12 at every row of P1 and P7.  No setting had to be replaced.

Measured on an MI355X, the largest over kernels, shapes and rows: predict mean 2.0e-13, variance 8.6e-13, ll 1.3e-14; ll_batch
against predict_batch's ll 1.4e-15; adjoints Abar 2.0e-11, Ubar 1.5e-11, Hbar 1.8e-11, Rbar 7.9e-13; the mixture 7.0e-14 against
the reference rows and 3.8e-18 against numpy on the device rows; test 7's rows have the single call's bits at P1, P2 and P6."""
import numpy as np
import pytest

import batch_refs as R
from het_refs import rel
from tests.conftest import relerr
from tests.test_gpu_adjoint import _check_stats, _rel

pytestmark = pytest.mark.gpu

KNAMES = R.KNAMES
LANES, WAVE, SUBTILE = R.LANES, 64, 4
TOL = 1e-9
REMEMBERS, FORGETS = -60.0, -120.0
GEOMETRY_SHAPES = ("P1", "P2", "P3", "P4", "P5", "P6", "P7")
# the interior workgroups held to the remembering band: "all", a set, or None
REMEMBERING = {"P1": "all", "P2": "all", "P3": "all", "P4": "all", "P5": "all", "P6": {1}, "P7": None}
SLOTS = ("k_filter_reduce", "k_filter_apply", "k_smoother_apply", "k_ll_finalize")


# ---- knobs, counters -------------------------------------------------------------------------------------------------------
class _Knobs:
    """pgps_set_chunk / _batch_form / _batch_scratch / _shortcut for the block; all four restored on every exit."""

    def __init__(self, chunk=0, form=0, scratch=0, shortcut=1):
        from pssgp import _backend as Bk
        self.ctx, self.values = Bk.get_context(), (chunk, form, scratch, shortcut)

    def __enter__(self):
        chunk, form, scratch, shortcut = self.values
        try:
            self.ctx.set_chunk(chunk)
            self.ctx.set_batch_form(form)
            self.ctx.set_batch_scratch(scratch)
            self.ctx.set_shortcut(shortcut)
        except BaseException:
            self.__exit__()
            raise
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.set_chunk(0)
        self.ctx.set_shortcut(1)
        self.ctx.set_batch_form(0)
        self.ctx.set_batch_scratch(0)


class _CountLaunches:
    """The context's launch counters (tests/test_gpu_panel.py's, on every slot); .launches() reads and resets: {slot: count}."""

    def __init__(self):
        from pssgp import _backend as Bk
        self.ctx = Bk.get_context()

    def __enter__(self):
        self.ctx.profile_enable(0x7f)
        self.ctx.profile_read(reset=True)
        return self

    def launches(self):
        return {name: int(v[1]) for name, v in self.ctx.profile_read(reset=True).items()}

    def __exit__(self, *exc):
        self.ctx.profile_enable(0)
        self.ctx.profile_read(reset=True)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b, what):
    for i, (x, z) in enumerate(zip(a, b)):
        assert np.array_equal(_bits(x), _bits(z)), f"{what}: part {i} differs"


# ---- models, geometry, roads ----------------------------------------------------------------------------------------------
def _model(kname, setting):
    from pssgp import _backend as Bk
    sde = R.sde(kname, setting)
    form = Bk.nilpotent_form(sde.F)
    assert form is not None
    return form, np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1), setting[2]


def _models(kname, rows=None):
    return [_model(kname, s) for s in (R.settings(kname) if rows is None else rows)]


def _geometry(shape, B, with_queries):
    """Steps per lane and workgroups of a B-model call over the shape's N (or N + K) steps under its pgps_set_chunk, read from
    the library (pgps_get_batch_chunk) and held to batch_refs.SHAPES."""
    from pssgp import _backend as Bk
    n, chunk, _, k, want_lc, nb_n, nb_nk = R.SHAPES[shape]
    rows = n + k if with_queries else n
    ctx = Bk.get_context()
    ctx.set_chunk(chunk)
    try:
        lc, nb = ctx.get_batch_chunk(B, rows)
    finally:
        ctx.set_chunk(0)
    waves = ""
    for w in range(LANES // WAVE):
        base = ((nb - 1) * LANES + w * WAVE) * lc
        waves += "s" if base + WAVE * lc <= rows and lc % SUBTILE == 0 else ("r" if base < rows else "e")
    print(f"shape {shape} B {B} rows {rows}: {lc} steps per lane, {nb} workgroups of {LANES * lc} steps, last workgroup's waves {waves}")
    assert (lc, nb) == (want_lc, nb_nk if with_queries else nb_n), (shape, B, rows, lc, nb)
    if shape == "P1":
        assert waves == "ssre"
    return lc, nb


def _held(f, which):
    """The entries of a (workgroups, 2) forgetting table a band is asserted on."""
    nb = f.shape[0]
    if nb < 3:                                  # no interior workgroup: the data's totals but E of the last (-inf: no gain)
        return [f[b, 0] for b in range(nb)] + [f[b, 1] for b in range(nb - 1)]
    blocks = range(1, nb - 1) if which == "all" else sorted(which)
    return [x for b in blocks for x in f[b]]


def _roads(kname, shape, with_queries, lc, nb, remembering, rememberer=None, forgetter=None):
    """Asserts from the reference, before any device call, that the batch holds a row whose held totals remember and one
    whose interior totals all forget."""
    rememberer = rememberer or R.REMEMBERER[kname]
    forgetter = forgetter or R.FORGETTER
    ff = R.forgetting(kname, forgetter, shape, with_queries, lc)
    fr = R.forgetting(kname, rememberer, shape, with_queries, lc)
    for name, setting, f in (("forgetter", forgetter, ff), ("rememberer", rememberer, fr)):
        print(f"{kname} {shape}{' merged' if with_queries else ''} {name} {setting}: log2 max|A| " + " ".join(f"{x:.0f}" for x in f[:, 0])
              + "  log2 max|E| " + " ".join(f"{x:.0f}" for x in f[:, 1]))
        assert f.shape[0] == nb
    assert all(x <= FORGETS for x in _held(ff, "all")), (kname, shape, forgetter, ff)
    if remembering is None:
        print(f"{kname} {shape}: every total of this grid forgets, whatever the setting (no rememberer)")
        return
    if kname == "m12" and LANES * lc >= 4096:
        print(f"{kname} {shape}: no allowed Matern-1/2 setting remembers over {LANES * lc} steps (the one exception): asserted "
              "for Matern-3/2 and -5/2 only")
        return
    assert all(x >= REMEMBERS for x in _held(fr, remembering)), (kname, shape, rememberer, fr)
    if remembering != "all":                    # ... and the other interior totals of that row forget
        others = set(range(1, nb - 1)) - set(remembering)
        assert all(x <= FORGETS for x in _held(fr, others)), (kname, shape, rememberer, fr)


def _predict_errors(got, refs):
    """[worst mean, var, ll error over the rows] of (mean (B, K), var (B, K), ll (B,)) against [(ll, mean, var)]"""
    mean, var, ll = got
    assert mean.shape == (len(refs), refs[0][1].size) and var.shape == mean.shape and ll.shape == (len(refs),)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var)) and np.all(np.isfinite(ll)) and np.all(var > 0.0)
    return [max(rel(mean[b], r[1]) for b, r in enumerate(refs)), max(rel(var[b], r[2]) for b, r in enumerate(refs)),
            max(abs(ll[b] - r[0]) / abs(r[0]) for b, r in enumerate(refs))]


def _check_predict(got, refs, what):
    e = _predict_errors(got, refs)
    print(f"{what} against the state-space reference [mean var ll] " + " ".join(f"{x:.2e}" for x in e))
    assert max(e) <= TOL, (what, e)
    return e


def _check_grad(rows, refs, d, what):
    from pssgp import _backend as Bk
    assert rows.shape == (len(refs), 2 + d * d + 2 * d) and np.all(np.isfinite(rows))
    stats = [Bk.split_grad_stats(row, d) for row in rows]
    e = [max(abs(s[0] - r[0]) / abs(r[0]) for s, r in zip(stats, refs))] + \
        [max(_rel(s[i], r[i]) for s, r in zip(stats, refs)) for i in (1, 2, 3, 4)]
    print(f"{what} against the reverse sweep [ll Abar Ubar Hbar Rbar] " + " ".join(f"{x:.2e}" for x in e))
    for s, r in zip(stats, refs):
        _check_stats(s, r, TOL)
    return e


def _dim(kname):
    return R.sde(kname, R.SETTINGS[0]).F.shape[0]


def _setup(kname, shape, with_queries, B=None):
    """Geometry from the library and the roads from the reference: (chunk, models, t, y, tq)."""
    models = _models(kname)
    lc, nb = _geometry(shape, B or len(models), with_queries)
    _roads(kname, shape, with_queries, lc, nb, REMEMBERING[shape])
    return (R.SHAPES[shape][1], models) + R.case(shape)


def _predict_refs(kname, shape, rows=None, shift=0.0):
    return [R.predict_ref(kname, s, shape, shift) for s in (R.settings(kname) if rows is None else rows)]


def _grad_refs(kname, shape, rows=None, shift=0.0):
    return [R.grad_ref(kname, s, shape, shift) for s in (R.settings(kname) if rows is None else rows)]


# ---- 1. predict, the three-launch form --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("shape", GEOMETRY_SHAPES)
def test_predict_batch_against_the_reference(kname, shape):
    from pssgp import _backend as Bk
    chunk, models, t, y, tq = _setup(kname, shape, True)
    assert tq[0] < t[0] and tq[-1] > t[-1] and np.intersect1d(tq, t).size >= 5
    if shape == "P1":
        assert np.all(np.isnan(y[1020:1030]))
    refs = _predict_refs(kname, shape)
    with _Knobs(chunk=chunk):
        got = Bk.gp_predict_batch(models, t, y, tq)[:3]
        again = Bk.gp_predict_batch(models, t, y, tq)[:3]
    _check_predict(got, refs, f"{kname} {shape} predict_batch")
    _same(got, again, "two calls")


# ---- 2. log-likelihood ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("shape", GEOMETRY_SHAPES)
def test_ll_batch_against_the_reference_and_the_predict(kname, shape):
    from pssgp import _backend as Bk
    chunk, models, t, y, tq = _setup(kname, shape, False)
    refs = _predict_refs(kname, shape)
    with _Knobs(chunk=chunk):
        ll = Bk.gp_ll_batch(models, t, y)
        again = Bk.gp_ll_batch(models, t, y)
        ll_p = Bk.gp_predict_batch(models, t, y, tq)[2]
    e = max(abs(ll[b] - r[0]) / abs(r[0]) for b, r in enumerate(refs))
    e_p = float(np.max(np.abs(ll - ll_p) / np.abs(ll_p)))
    print(f"{kname} {shape} ll_batch against the state-space reference {e:.2e}, against predict_batch's ll {e_p:.2e}")
    assert ll.shape == (len(models),) and np.all(np.isfinite(ll))
    assert e <= TOL and e_p <= 1e-12
    _same([ll], [again], "two calls")


# ---- 3. log-likelihood and adjoints -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("shape", ["P1", "P2", "P3", "P5", "P6"])
def test_grad_batch_against_the_reverse_sweep(kname, shape):
    """The host-array entry point and a resident Series; the four-launch road by launch count (without a pinned chunk
    N = 2600 would take the one-launch form only)."""
    from pssgp import _backend as Bk
    chunk, models, t, y, _ = _setup(kname, shape, False)
    refs = _grad_refs(kname, shape)
    d = _dim(kname)
    with _Knobs(chunk=chunk), _CountLaunches() as count:
        host = Bk.gp_ll_grad_adj_batch(models, t, y)
        n = count.launches()
        ser = Bk.Series(t, y)
        try:
            res = ser.gp_ll_grad_adj_batch(models)
        finally:
            ser.close()
    print(f"{kname} {shape} grad_batch launches " + " ".join(f"{s} {n[s]}" for s in SLOTS))
    assert [n[s] for s in SLOTS] == [1, 1, 1, 1], n
    _check_grad(host, refs, d, f"{kname} {shape} grad_batch (host arrays)")
    _check_grad(res, refs, d, f"{kname} {shape} grad_batch (resident series)")
    _same([host], [res], "host arrays and the resident series")


# ---- 4. the automatic rule's own 16 and 8 steps per lane ----------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("B,lc,nb", [(512, 16, 2), (256, 8, 4)], ids=["AUTO16", "AUTO8"])
def test_the_automatic_rule_at_sixteen_and_eight_steps_per_lane(kname, B, lc, nb):
    """7680 + 512 = 8192 merged steps, the rows cycle through four settings: four references serve the call, the copies of a
    setting are bit-identical, and the default 64 MiB budget cuts B = 512 into more than one group (by launch count)."""
    from pssgp import _backend as Bk
    four = R.AUTO_SETTINGS[kname]
    t, y, tq = R.case("AUTO")
    ctx = Bk.get_context()
    ctx.set_chunk(0)
    geo = (ctx.get_batch_chunk(B, t.size + tq.size), ctx.get_batch_chunk(B, t.size))
    print(f"AUTO B {B}: (steps per lane, workgroups) of {t.size + tq.size} merged steps {geo[0]}, of {t.size} steps {geo[1]}")
    assert geo == ((lc, nb), (lc, nb))
    for with_queries in (True, False):
        _roads(kname, "AUTO", with_queries, lc, nb, "all", rememberer=four[0], forgetter=R.AUTO_FORGETTER[kname])
    models = [_model(kname, four[b % 4]) for b in range(B)]
    p_refs, g_refs = _predict_refs(kname, "AUTO", four), _grad_refs(kname, "AUTO", four)
    d = _dim(kname)
    with _Knobs(), _CountLaunches() as count:
        got = Bk.gp_predict_batch(models, t, y, tq)[:3]
        n_p = count.launches()
        ll = Bk.gp_ll_batch(models, t, y)
        count.launches()
        rows = Bk.gp_ll_grad_adj_batch(models, t, y)
        n_g = count.launches()
    print(f"{kname} AUTO B {B}: groups of the predict {n_p['k_filter_reduce']}, of the gradient {n_g['k_filter_reduce']}")
    assert n_p["k_smoother_apply"] == n_p["k_filter_reduce"] == n_p["k_filter_apply"] and n_g["k_ll_finalize"] == n_g["k_filter_reduce"]
    if B == 512:                                # (256 models of d = 1 fit the budget at once)
        assert n_p["k_filter_reduce"] > 1 and n_g["k_filter_reduce"] > 1, (n_p, n_g)
    for b in range(4, B):
        _same([x[b] for x in got] + [ll[b], rows[b]], [x[b % 4] for x in got] + [ll[b % 4], rows[b % 4]], f"copy {b} of setting {b % 4}")
    _check_predict(tuple(x[:4] for x in got), p_refs, f"{kname} AUTO B {B} predict_batch")
    e = max(abs(ll[b] - p_refs[b][0]) / abs(p_refs[b][0]) for b in range(4))
    print(f"{kname} AUTO B {B} ll_batch against the state-space reference {e:.2e}")
    assert e <= TOL
    _check_grad(rows[:4], g_refs, d, f"{kname} AUTO B {B} grad_batch")


# ---- 5. form 1: one workgroup per model --------------------------------------------------------------------------------------
def _form1_steps(rows):
    """one_workgroup_steps (pgps_inst.hip): steps per lane of the ONE workgroup, whole 4-step sub-tiles"""
    return (-(-rows // LANES) + 3) // 4 * 4


@pytest.mark.parametrize("kname", KNAMES)
def test_form_one_at_twenty_steps_per_lane(kname):
    """P2's data with no chunk pinned: 4746 merged steps in one workgroup per model, 20 steps per lane; one launch for the one
    group (the merge is not on a counted slot).  One workgroup: no carry crosses a boundary; the rows are P2's."""
    from pssgp import _backend as Bk
    models = _models(kname)
    t, y, tq = R.case("P2")
    assert _form1_steps(t.size + tq.size) == 20
    print(f"form 1, {t.size + tq.size} merged steps: one workgroup, {_form1_steps(t.size + tq.size)} steps per lane (one_workgroup_steps)")
    _roads(kname, "P2", True, 8, 3, "all")
    refs = _predict_refs(kname, "P2")
    with _Knobs(form=1), _CountLaunches() as count:
        got = Bk.gp_predict_batch(models, t, y, tq)[:3]
        n = count.launches()
        again = Bk.gp_predict_batch(models, t, y, tq)[:3]
    assert [n[s] for s in SLOTS] == [0, 1, 0, 0], n
    _check_predict(got, refs, f"{kname} P2 form 1")
    _same(got, again, "two calls")


@pytest.mark.parametrize("kname", KNAMES)
def test_form_one_at_eighty_steps_per_lane(kname):
    """20 000 + 480 = 20 480 merged steps, B = 3: 80 steps per lane; the first 4096 rows on the 2e-4 grid, 0.05 after."""
    from pssgp import _backend as Bk
    rows = (R.SETTINGS[0], R.SETTINGS[2], R.SETTINGS[4])
    t, y, tq = R.case("LONG")
    assert t.size + tq.size == 20480 and _form1_steps(20480) == 80
    print("form 1, 20480 merged steps: one workgroup, 80 steps per lane (one_workgroup_steps)")
    refs = _predict_refs(kname, "LONG", rows)
    with _Knobs(form=1), _CountLaunches() as count:
        got = Bk.gp_predict_batch(_models(kname, rows), t, y, tq)[:3]
        n = count.launches()
    assert [n[s] for s in SLOTS] == [0, 1, 0, 0], n
    _check_predict(got, refs, f"{kname} LONG form 1")


def test_form_one_gives_way_to_form_two_above_its_limit():
    """65 550 merged steps > kBatchOneMax = 65 536: the three launches run although form 1 is asked for (by launch count
    alone; no reference at this size)."""
    from pssgp import _backend as Bk
    t, y, tq = R.case("OVER")
    assert t.size + tq.size == 65550
    rows = (R.SETTINGS[0], R.SETTINGS[2])
    with _Knobs(form=1), _CountLaunches() as count:
        lc, nb = count.ctx.get_batch_chunk(2, t.size + tq.size)
        got = Bk.gp_predict_batch(_models("m32", rows), t, y, tq)[:3]
        n = count.launches()
    print(f"form 1 asked for at 65550 merged steps: {lc} steps per lane, {nb} workgroups, launches {n}")
    assert [n[s] for s in SLOTS] == [1, 1, 1, 0], n
    assert all(np.all(np.isfinite(x)) for x in got) and np.all(got[1] > 0.0)


# ---- 6. groups ----------------------------------------------------------------------------------------------------------------
def _up(nbytes):
    return (nbytes + 255) // 256 * 256


def _records(d):
    """(NFILT, NSMTH, NX, NST): doubles of a filter record (A, b, C, J, eta), a smoother record (E, g, L), a kept state
    (mean and packed covariance) and the adjoint statistics (pgps_math.h Dim<D>, pgps_gpadj.hip.h)"""
    sym = d * (d + 1) // 2
    return d * d + d + sym + sym + d, d * d + d + sym, d + sym, d * d + 2 * d + 1


def _predict_bytes_per_model(d, rows, lc, nb):
    """launch_gp_predict_batch's layout of ONE model (fp64, form 2), every part rounded up to 256 bytes: the workgroup and
    lane records of the filter and of the smoother, the log-likelihood partials, the filtered means and covariances."""
    nf, ns, _, _ = _records(d)
    nl = nb * LANES
    return _up(nb * nf * 8) + _up(nl * nf * 8) + _up(nb * ns * 8) + _up(nl * ns * 8) + _up(nb * 8) + _up(rows * d * 8) + _up(rows * d * d * 8)


def _grad_bytes_per_model(d, lc, nb):
    """launch_gp_adj_batch's two layouts of ONE model: the same records and partials, the kept states (steps per lane x NX x
    lanes) and the workgroup partials of the statistics."""
    nf, ns, nx, nst = _records(d)
    nl = nb * LANES
    return _up(nb * nf * 8) + _up(nl * nf * 8) + _up(nb * ns * 8) + _up(nl * ns * 8) + _up(nb * 8) + _up(lc * nx * nl * 8) + _up(nb * nst * 8)


@pytest.mark.parametrize("kname", KNAMES)
def test_groups_of_four_and_two_and_of_one_at_p2(kname):
    """Budgets from the documented layout that split the first six rows into 4 + 2 and into six groups of one: the reference,
    the bits of the ungrouped call, and the reversed table gives the reversed rows (on remembering data a slice mix-up
    would move a result)."""
    from pssgp import _backend as Bk
    rows = R.settings(kname)[-6:]               # (Matern-1/2: its rememberer is the seventh row)
    n, chunk, _, k, lc, nb, nb_q = R.SHAPES["P2"]
    assert _geometry("P2", 6, True) == (lc, nb_q) and _geometry("P2", 6, False) == (lc, nb)
    _roads(kname, "P2", True, lc, nb_q, "all")
    _roads(kname, "P2", False, lc, nb, "all")
    models = _models(kname, rows)
    t, y, tq = R.case("P2")
    d = _dim(kname)
    p_refs, g_refs = _predict_refs(kname, "P2", rows), _grad_refs(kname, "P2", rows)
    with _Knobs(chunk=chunk):
        base_p = Bk.gp_predict_batch(models, t, y, tq)[:3]
        base_g = Bk.gp_ll_grad_adj_batch(models, t, y)
        rev_p = Bk.gp_predict_batch(models[::-1], t, y, tq)[:3]
        rev_g = Bk.gp_ll_grad_adj_batch(models[::-1], t, y)
    _check_predict(base_p, p_refs, f"{kname} P2 predict_batch, one group")
    _check_grad(base_g, g_refs, d, f"{kname} P2 grad_batch, one group")
    _same([x[::-1] for x in rev_p] + [rev_g[::-1]], list(base_p) + [base_g], "the reversed table")
    per_p, per_g = _predict_bytes_per_model(d, n + k, lc, nb_q), _grad_bytes_per_model(d, lc, nb)
    for groups, models_per_budget in ((2, 4.5), (6, 1.5)):
        with _Knobs(chunk=chunk, scratch=int(models_per_budget * per_p)), _CountLaunches() as count:
            got_p = Bk.gp_predict_batch(models, t, y, tq)[:3]
            n_p = count.launches()
        with _Knobs(chunk=chunk, scratch=int(models_per_budget * per_g)), _CountLaunches() as count:
            got_g = Bk.gp_ll_grad_adj_batch(models, t, y)
            n_g = count.launches()
        print(f"{kname} P2: {per_p} / {per_g} bytes per model (predict / gradient), budgets of {models_per_budget} models: "
              f"{n_p['k_filter_reduce']} / {n_g['k_filter_reduce']} groups")
        assert n_p["k_filter_reduce"] == groups and n_g["k_filter_reduce"] == groups, (n_p, n_g)
        _check_predict(got_p, p_refs, f"{kname} P2 predict_batch, {groups} groups")
        _check_grad(got_g, g_refs, d, f"{kname} P2 grad_batch, {groups} groups")
        _same(list(got_p) + [got_g], list(base_p) + [base_g], f"{groups} groups and one")


# ---- 7. what DESIGN.md 4q states: the single call's bits -----------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("shape", ["P1", "P2", "P6"])
def test_rows_have_the_bits_of_the_single_call_at_its_geometry(kname, shape):
    """Under a pinned chunk form 2 has the single call's geometry; with the forgetting shortcut off for the single call (the
    batch never takes it) row b has the bits of gp_predict on model b: mean, var, ll."""
    from pssgp import _backend as Bk
    chunk, models, t, y, tq = _setup(kname, shape, True)
    with _Knobs(chunk=chunk, shortcut=0) as ctx:
        assert ctx.get_chunk(t.size + tq.size) == ctx.get_batch_chunk(len(models), t.size + tq.size)
        mean, var, ll = Bk.gp_predict_batch(models, t, y, tq)[:3]
        single = [Bk.gp_predict(f, P, H, r, t, y, tq) for f, P, H, r in models]
    differing = [b for b, s in enumerate(single)
                 if not (np.array_equal(_bits(mean[b]), _bits(s[0])) and np.array_equal(_bits(var[b]), _bits(s[1]))
                         and np.array_equal(_bits(ll[b]), _bits(s[2])))]
    e = [max(rel(mean[b], s[0]) for b, s in enumerate(single)), max(rel(var[b], s[1]) for b, s in enumerate(single)),
         max(abs(ll[b] - s[2]) / abs(s[2]) for b, s in enumerate(single))]
    print(f"{kname} {shape}: batch rows against gp_predict (shortcut off) [mean var ll] " + " ".join(f"{x:.2e}" for x in e)
          + f"; rows whose bits differ: {differing}")
    assert not differing, differing


# ---- 8. a start time other than zero -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
def test_a_start_time_other_than_zero(kname):
    """t0 = -0.3 at P1: the references on t + 0.3 (their first step starts from 0)."""
    from pssgp import _backend as Bk
    t0 = -0.3
    chunk, models, t, y, tq = _setup(kname, "P1", True)
    _geometry("P1", len(models), False)
    p_refs, g_refs = _predict_refs(kname, "P1", shift=-t0), _grad_refs(kname, "P1", shift=-t0)
    with _Knobs(chunk=chunk):
        got = Bk.gp_predict_batch(models, t, y, tq, t0=t0)[:3]
        ll = Bk.gp_ll_batch(models, t, y, t0=t0)
        rows = Bk.gp_ll_grad_adj_batch(models, t, y, t0=t0)
        ser = Bk.Series(t, y, t0=t0)
        try:
            res = ser.gp_ll_grad_adj_batch(models)
        finally:
            ser.close()
    _check_predict(got, p_refs, f"{kname} P1 t0 {t0} predict_batch")
    e = max(abs(ll[b] - r[0]) / abs(r[0]) for b, r in enumerate(p_refs))
    print(f"{kname} P1 t0 {t0} ll_batch against the state-space reference {e:.2e}")
    assert e <= TOL
    _check_grad(rows, g_refs, _dim(kname), f"{kname} P1 t0 {t0} grad_batch")
    _same([rows], [res], "host arrays and the resident series")


# ---- 9. the mixture over groups --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
def test_mixture_over_groups_of_four_and_two(kname):
    """gp_predict_batch(mix = weights) at P2 under the 4 + 2 budget: numpy's two-pass mixture of the reference rows at 1e-9,
    of the device rows at 1e-12 (test_gpu_predict_batch.py's bound for k_mix_moments)."""
    from pssgp import _backend as Bk
    from pssgp.model import StateSpaceGP
    rows = R.settings(kname)[-6:]
    n, chunk, _, k, lc, _, nb_q = R.SHAPES["P2"]
    assert _geometry("P2", 6, True) == (lc, nb_q)
    _roads(kname, "P2", True, lc, nb_q, "all")
    models = _models(kname, rows)
    t, y, tq = R.case("P2")
    refs = _predict_refs(kname, "P2", rows)
    w = np.random.RandomState(9).uniform(0.2, 1.0, 6)
    w /= w.sum()
    budget = int(4.5 * _predict_bytes_per_model(_dim(kname), n + k, lc, nb_q))
    with _Knobs(chunk=chunk):
        mean, var, ll = Bk.gp_predict_batch(models, t, y, tq)[:3]
    with _Knobs(chunk=chunk, scratch=budget), _CountLaunches() as count:
        none_m, none_v, ll_mix, (mm, mv) = Bk.gp_predict_batch(models, t, y, tq, mix=w)
        n_l = count.launches()
    assert none_m is None and none_v is None and n_l["k_filter_reduce"] == 2, n_l
    _same([ll_mix], [ll], "ll with and without the mixture")
    ref_m, ref_v = StateSpaceGP._mix_moments_host(np.stack([r[1] for r in refs]), np.stack([r[2] for r in refs]), w)
    dev_m, dev_v = StateSpaceGP._mix_moments_host(mean, var, w)
    e_ref, e_dev = [rel(mm, ref_m), rel(mv, ref_v)], [relerr(mm, dev_m), relerr(mv, dev_v)]
    print(f"{kname} P2 mixture [mean var] against the reference rows " + " ".join(f"{x:.2e}" for x in e_ref)
          + ", against numpy on the device rows " + " ".join(f"{x:.2e}" for x in e_dev))
    assert max(e_ref) <= TOL and max(e_dev) <= 1e-12
