"""GPU tests of the multi-output kernels (k_gpm_reduce / k_gpm_apply / k_gpm_smooth; k_gpm_gfwd /
k_gpm_gback / k_gpm_gfinal, section 4t) at the launch geometries a realistic call has, which test_gpu_multi_output.py (at most
1600 merged steps, four steps per lane, three workgroups, never split into rounds) and test_gpu_multi_grad.py (5000 steps only
at M = 3, rounds only at 700 steps in one workgroup) never reach.  These kernels have no LDS-staged road and no forgetting
shortcut -- the carry across workgroups is always the general fold -- so what can break them is indexing: long lane chunks, a
ragged last lane with empty waves after it, many workgroups, several column groups with a partial last group, rounds of unequal
size (their own c_base, their own leading dimension ldm = G * MC of the kept means, fPs rewritten by group 0 of every round, var
written by the round that holds column 0; one slice of the kept states xs per group in the gradient), and query slots spread
over all of that.

One training series: N = 4696 rows at spacing 0.05 (multi_refs.multi_series), K = 50 queries (het_refs.queries: before the
first time, after the last, ties on training times), M = 2 x tile + 1 = 17 / 9 / 5 columns for Matern-1/2, -3/2, -5/2: three
column groups, the last one holding one column.  Rows 2040..2055 and 4090..4100 are missing, a missing run across a workgroup
boundary at every chunk below.

  pgps_set_chunk   steps per workgroup   workgroups at 4696 / 4746 steps
  1                256                   19 / 19     spine folds of up to 18 entries, one step per lane
  4                1024                  5 / 5       what the default picks at this size
  8                2048                  3 / 3       long chunks, a ragged last lane at 4746 steps, empty waves
  16               4096                  2 / 2       the large-call default; the last workgroup holds 600 / 650 steps in 38 / 41 lanes
  0                the library's                     the call a user makes (batch_steps_per_lane; not asserted)

Under an explicit chunk (steps per lane, workgroups) are read from the library (pgps_get_chunk: geometry() and multi_geometry()
agree whenever a chunk is set) and held to this table before the call.

References (multi_refs.py, het_refs.py, oracle/np_grad.py; none is the code under test): the numpy Kalman filter + RTS smoother
with one covariance and a (d, M) matrix of means at the project's 1e-9, the oracle's reverse sweep per column summed over the
columns at 1e-9 (max norm of a statistic, floor 1e-6), rtol 1e-11 on log-likelihoods against a device twin, bit equality where
the same arithmetic runs.  Kernels: variance 1, lengthscale 0.5; R = 0.1.  Every checked call follows the same call on other
data under the library's own geometry and budget (_fresh), so nothing an earlier call left in the context's staging buffers or
scratch can pass for its result."""
import functools

import numpy as np
import pytest

from het_refs import R, queries, sde_of
from multi_refs import merged_rows, multi_series, ss_multi
from oracle import np_grad as G
from tests.conftest import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-9
KNAMES = ("m12", "m32", "m52")
# compiled tile widths (MultiTile / MultiGradTile): d = 1 -> 8, d = 2 -> 4, d = 3 -> 2 columns per tile
TILE = {"m12": 8, "m32": 4, "m52": 2}
# doubles of a column-tiled filtering / smoothing element: d^2 + d (d + 1) + 2 d MC, d^2 + d (d + 1) / 2 + d MC
FE = {"m12": 19, "m32": 26, "m52": 33}
SE = {"m12": 10, "m32": 15, "m52": 21}
DIM = {"m12": 1, "m32": 2, "m52": 3}
LANES = 256
N, K, SPACING = 4696, 50, 0.05
MISSING = tuple(range(2040, 2056)) + tuple(range(4090, 4101))
# pgps_set_chunk -> (steps per lane, workgroups) at N and at N + K steps
GEOMETRY = {1: (1, 19), 4: (4, 5), 8: (8, 3), 16: (16, 2)}
NAMES = ("Abar", "Ubar", "Hbar", "Rbar")
REDUCE = "k_filter_reduce"                  # the launch counter's slot 0: one k_gpm_reduce per round


def _m(kname, extra=1):
    return 2 * TILE[kname] + extra


class _Chunk:
    """pgps_set_chunk for the block, restored on every exit."""

    def __init__(self, steps):
        from pssgp import _backend as Bk
        self.ctx, self.steps = Bk.get_context(), steps

    def __enter__(self):
        self.ctx.set_chunk(self.steps)
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.set_chunk(0)


class _BatchScratch:
    """pgps_set_batch_scratch for the block, restored on every exit."""

    def __init__(self, nbytes):
        from pssgp import _backend as Bk
        self.ctx, self.nbytes = Bk.get_context(), nbytes

    def __enter__(self):
        self.ctx.set_batch_scratch(self.nbytes)

    def __exit__(self, *exc):
        self.ctx.set_batch_scratch(0)


class _CountReduce:
    """The context's launch counter on the filter-reduce slot alone, switched off on every exit; .launches() reads and resets."""

    def __init__(self):
        from pssgp import _backend as Bk
        self.ctx = Bk.get_context()

    def __enter__(self):
        self.ctx.profile_enable(1)
        self.ctx.profile_read(reset=True)
        return self

    def launches(self):
        return int(self.ctx.profile_read(reset=True)[REDUCE][1])

    def __exit__(self, *exc):
        self.ctx.profile_enable(0)
        self.ctx.profile_read(reset=True)


def _form(kname):
    from pssgp import _backend as Bk
    sde = sde_of(kname)
    return Bk.nilpotent_form(sde.F), np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _fresh(call, form, P, H, t, Y, *rest, chunk=0, budget=0, **kw):
    """call(form, P, H, R, t, Y, ...) under pgps_set_chunk(chunk) and pgps_set_batch_scratch(budget), after the same call on
    OTHER data of the same shape (1 - Y: the same rows missing) under the library's own geometry and budget.  The host-array
    entry points stage their results in buffers the context keeps, the partial sums live in its scratch, and every test here
    runs the same data: an element that a kernel fails to write under one geometry or budget would otherwise still hold the
    correct value another call left there.  After the other call it holds a wrong one."""
    call(form, P, H, R, t, 1.0 - Y, *rest, **kw)
    with _Chunk(chunk), _BatchScratch(budget):
        return call(form, P, H, R, t, Y, *rest, **kw)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _case(m, k=K):
    """(t, Y (N, m), tq (k,)): computed once, read-only."""
    t, Y = multi_series(N, m, SPACING, extra_missing=MISSING)
    return _frozen(t, Y, queries(t, k))


@functools.lru_cache(maxsize=None)
def _ref(kname, m, k=K, shift=0.0):
    """(mean (k, m), var (k, 1), ll (m,)) of ss_multi on t + shift, in the order and shapes _check_columns takes them."""
    t, Y, tq = _case(m, k)
    ll, mean, var = ss_multi(sde_of(kname), t + shift, Y, R, tq + shift)
    return _frozen(mean, var[:, None], ll)


@functools.lru_cache(maxsize=None)
def _oracle(kname, m, shift=0.0):
    """The oracle's reverse sweep of every column on t + shift: (ll (m,), [Abar, Ubar, Hbar, Rbar] summed over the columns, per
    statistic sum_c max|stat_c|), as test_gpu_multi_grad._oracle."""
    sde = sde_of(kname)
    t, Y, _ = _case(m)
    cols = [G.ll_grad_stats(sde.F, sde.P0, sde.H, R, t + shift, Y[:, j]) for j in range(m)]
    ll = np.array([c[0] for c in cols])
    sums = [np.asarray(np.sum([np.asarray(c[i], np.float64) for c in cols], axis=0)) for i in range(1, 5)]
    mags = [float(np.sum([np.max(np.abs(c[i])) for c in cols])) for i in range(1, 5)]
    _frozen(ll, *sums)
    return ll, sums, mags


def _geometry(chunk, rows, want=None):
    """(steps per lane, workgroups) of a `rows`-step call under pgps_set_chunk(chunk), read from the library and held to the
    table; the lanes of the last workgroup that hold steps."""
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    ctx.set_chunk(chunk)
    try:
        lc, nb = ctx.get_chunk(rows)
    finally:
        ctx.set_chunk(0)
    last = rows - (nb - 1) * LANES * lc
    print(f"chunk {chunk} rows {rows}: {lc} steps per lane, {nb} workgroups of {LANES * lc} steps, the last one holds {last} steps in "
          f"{-(-last // lc)} lanes ({'ragged' if last % lc else 'whole'} last lane, {(LANES - -(-last // lc)) // 64} empty waves)")
    assert (lc, nb) == (GEOMETRY[chunk] if want is None else want), (chunk, rows, lc, nb)
    return lc, nb


def _check_columns(got, want, what, ll_rtol=TOL):
    """test_gpu_multi_output._check_columns: mean and var relative to the largest entry, ll relative (floor 1)."""
    mean, var, ll = got
    w_mean, w_var, w_ll = want
    assert mean.shape == w_mean.shape and ll.shape == w_ll.shape and var.shape == (w_mean.shape[0],)
    worst = [0.0, 0.0, 0.0]
    for j in range(w_mean.shape[1]):
        em, ev = relerr(mean[:, j], w_mean[:, j]), relerr(var, w_var[:, j if w_var.shape[1] > 1 else 0])
        el = abs(ll[j] - w_ll[j]) / max(1.0, abs(w_ll[j]))
        worst = [max(a, b) for a, b in zip(worst, (em, ev, el))]
        assert em < TOL and ev < TOL, (what, j, em, ev)
        assert el < ll_rtol, (what, j, ll[j], w_ll[j])
    print(f"{what}: worst column mean {worst[0]:.2e} var {worst[1]:.2e} ll {worst[2]:.2e}")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))


def _check_stats(got, want, what):
    """test_gpu_multi_grad._check_stats: got = (ll (M,), Abar, Ubar, Hbar, Rbar) of the device; want = (ll (M,), [sums])."""
    ll, stats = got[0], got[1:]
    w_ll, w_stats = want
    assert ll.shape == w_ll.shape
    el = float(np.max(np.abs(ll - w_ll) / np.abs(w_ll)))
    assert el <= TOL, (what, ll, w_ll)
    es = []
    for name, a, b in zip(NAMES, stats, w_stats):
        e = _rel(a, b)
        es.append(e)
        assert np.shape(a) == np.shape(b) and e <= TOL, (what, name, e)
    print(f"{what}: worst column ll {el:.2e} " + " ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, es)))


def _guard(kname, m, shift=0.0):
    """Cancellation between the columns cannot hide an error: the sum is no smaller than 1/16 of its terms' magnitudes.  A
    condition on the data, asserted from the oracle before the device is touched."""
    ll, sums, mags = _oracle(kname, m, shift)
    for name, s, mag in zip(NAMES, sums, mags):
        ratio = mag / max(1e-300, float(np.max(np.abs(s))))
        print(f"{kname} M {m} {name}: sum_c max|stat_c| / max|sum_c stat_c| = {ratio:.2f}")
        assert mag <= 16.0 * float(np.max(np.abs(s))), (name, mag, float(np.max(np.abs(s))))
    return ll, sums


def _align256(x):
    return (x + 255) & ~255


def _two_group_budget(kname, m, fixed_doubles, group_doubles):
    """A pgps_set_batch_scratch that holds exactly two column groups, from the launch functions' own layout: the parts the
    groups share (each aligned to 256 bytes) + 2.5 x one group's bytes."""
    groups = -(-m // TILE[kname])
    assert groups == 3
    return sum(_align256(8 * x) for x in fixed_doubles) + (5 * 8 * group_doubles) // 2


def _predict_budget(kname, m, rows, nb):
    """launch_gp_multi: llpart (groups x MC x nb) and fPs (rows x SYM) are shared; a group holds its spine, lane prefixes, the
    smoother's spine and lane suffixes and its kept means (rows x MC x d)."""
    d, mc = DIM[kname], TILE[kname]
    nl = LANES * nb
    return _two_group_budget(kname, m, (3 * mc * nb, rows * d * (d + 1) // 2),
                             nb * FE[kname] + nl * FE[kname] + nb * SE[kname] + nl * SE[kname] + rows * mc * d)


def _grad_budget(kname, m, lc, nb):
    """launch_gp_multi_grad: llpart and gpart (groups x nb x NST) are shared; a group holds its spines, lane prefixes and
    suffixes and its kept states xs (nl x Lc x NX, NX = SYM + MC d)."""
    d, mc = DIM[kname], TILE[kname]
    nl, nst, nx = LANES * nb, d * d + 2 * d + 1, d * (d + 1) // 2 + mc * d
    return _two_group_budget(kname, m, (3 * mc * nb, 3 * nb * nst),
                             nb * FE[kname] + nl * FE[kname] + nb * SE[kname] + nl * SE[kname] + nl * lc * nx)


# ---- 1. predict and log-likelihood at every geometry ------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("chunk", [1, 4, 8, 16, 0])
def test_predict_and_ll_against_the_reference(kname, chunk):
    from pssgp import _backend as Bk
    m = _m(kname)
    form, P, H = _form(kname)
    t, Y, tq = _case(m)
    assert tq[0] < t[0] and tq[-1] > t[-1] and np.intersect1d(tq, t).size >= 5
    assert np.all(np.isnan(Y[list(MISSING)])) and not np.isnan(Y[N // 2, 0])
    want = _ref(kname, m)
    if chunk:
        _geometry(chunk, N), _geometry(chunk, N + K)
    else:
        print(f"chunk 0: the library's own choice for {-(-m // TILE[kname])} column groups over {N} / {N + K} steps")
    got = _fresh(Bk.gp_predict_multi, form, P, H, t, Y, tq, chunk=chunk)
    again = _fresh(Bk.gp_predict_multi, form, P, H, t, Y, tq, chunk=chunk)
    ll = _fresh(Bk.gp_ll_multi, form, P, H, t, Y, chunk=chunk)
    ll_again = _fresh(Bk.gp_ll_multi, form, P, H, t, Y, chunk=chunk)
    assert all(np.all(np.isfinite(a)) for a in got) and np.all(np.isfinite(ll))
    _check_columns(got, want, f"{kname} M {m} chunk {chunk} predict")
    e_ll = float(np.max(np.abs(ll - want[2]) / np.maximum(1.0, np.abs(want[2]))))
    print(f"{kname} M {m} chunk {chunk} gp_ll_multi: worst column {e_ll:.2e}")
    assert e_ll < TOL
    assert _same(got, again) and _same((ll,), (ll_again,)), "two calls differ"


# ---- 2. vector loads ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
def test_vector_loads_and_a_scalar_last_group(kname):
    """M = 2 x tile + 2 is even: the two full groups take the 16-byte loads of Y and stores of the means, the last group (two
    columns) the scalar ones.  A column does not depend on what the other groups hold: columns 0 .. 2 x tile - 1 have the bits
    of a call on those columns alone."""
    from pssgp import _backend as Bk
    m, full = _m(kname, 2), 2 * TILE[kname]
    form, P, H = _form(kname)
    t, Y, tq = _case(m)
    _geometry(8, N), _geometry(8, N + K)
    got = _fresh(Bk.gp_predict_multi, form, P, H, t, Y, tq, chunk=8)
    ll = _fresh(Bk.gp_ll_multi, form, P, H, t, Y, chunk=8)
    part = _fresh(Bk.gp_predict_multi, form, P, H, t, np.ascontiguousarray(Y[:, :full]), tq, chunk=8)
    ll_part = _fresh(Bk.gp_ll_multi, form, P, H, t, np.ascontiguousarray(Y[:, :full]), chunk=8)
    want = _ref(kname, m)
    _check_columns(got, want, f"{kname} M {m} chunk 8 predict")
    assert float(np.max(np.abs(ll - want[2]) / np.maximum(1.0, np.abs(want[2])))) < TOL
    assert np.array_equal(_bits(got[0][:, :full]), _bits(part[0])), "a column's mean depends on the other groups"
    assert np.array_equal(_bits(got[1]), _bits(part[1])), "the variance depends on the other groups"
    assert np.array_equal(_bits(got[2][:full]), _bits(part[2])) and np.array_equal(_bits(ll[:full]), _bits(ll_part))


# ---- 3. rounds of predict -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("chunk", [4, 8])
def test_predict_does_not_depend_on_the_rounds(kname, chunk):
    """The default budget holds the three column groups in one round; pgps_set_batch_scratch(1) makes three rounds of one
    group (ldm = tile); a budget for exactly two groups makes rounds of two and one, so ldm changes between the rounds, fPs is
    rewritten by the second round's group 0 and var comes from the first round alone.  Same bits, and the rounds are counted.
    Before every one of the three calls the same call runs on other data in ONE round (as _fresh): a round that wrote the wrong
    columns would otherwise leave the columns it skipped with the bits of the call before -- the right ones."""
    from pssgp import _backend as Bk
    m = _m(kname)
    form, P, H = _form(kname)
    t, Y, tq = _case(m)
    nb = _geometry(chunk, N + K)[1]
    two = _predict_budget(kname, m, N + K, nb)
    got, rounds = {}, {}
    with _CountReduce() as count:
        for name, budget in (("default", 0), ("one group", 1), ("two groups", two)):
            Bk.gp_predict_multi(form, P, H, R, t, 1.0 - Y, tq)              # (as _fresh, outside the count)
            count.launches()
            with _Chunk(chunk), _BatchScratch(budget):
                got[name] = Bk.gp_predict_multi(form, P, H, R, t, Y, tq)
            rounds[name] = count.launches()
    print(f"{kname} M {m} chunk {chunk}: two-group budget {two} bytes, k_gpm_reduce launches {rounds}")
    assert rounds == {"default": 1, "one group": 3, "two groups": 2}
    _check_columns(got["default"], _ref(kname, m), f"{kname} M {m} chunk {chunk} predict, one round")
    for name in ("one group", "two groups"):
        for what, a, b in zip(("mean", "var", "ll"), got["default"], got[name]):
            assert np.array_equal(_bits(a), _bits(b)), f"{what} depends on the rounds ({name} per round)"


# ---- 4. many queries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
def test_predict_with_many_queries(kname):
    """K = 1500 at four steps per lane: 6196 merged steps in seven workgroups, the query slots spread over all of them."""
    from pssgp import _backend as Bk
    k, m = 1500, _m(kname)
    form, P, H = _form(kname)
    t, Y, tq = _case(m, k)
    assert np.all(np.diff(tq) >= 0) and np.intersect1d(tq, t).size >= k // 8
    isq = merged_rows(t, Y, tq)[2]
    per_workgroup = np.add.reduceat(isq.astype(int), np.arange(0, N + k, 4 * LANES))
    print(f"query slots per workgroup: {per_workgroup.tolist()}")
    assert per_workgroup.size == 7 and per_workgroup.min() >= 1
    _geometry(4, N + k, (4, 7))
    got = _fresh(Bk.gp_predict_multi, form, P, H, t, Y, tq, chunk=4)
    assert all(np.all(np.isfinite(a)) for a in got)
    _check_columns(got, _ref(kname, m, k), f"{kname} M {m} chunk 4 with {k} queries")


# ---- 5. against the single-column device call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
def test_against_the_single_column_device_call(kname):
    from pssgp import _backend as Bk
    m = _m(kname)
    form, P, H = _form(kname)
    t, Y, tq = _case(m)
    _geometry(8, N + K)
    mean, var, ll = _fresh(Bk.gp_predict_multi, form, P, H, t, Y, tq, chunk=8)
    with _Chunk(8):
        for j in (0, TILE[kname], m - 1):       # one column of every group
            m1, v1, l1 = Bk.gp_predict(form, P, H, R, t, np.ascontiguousarray(Y[:, j]), tq)
            em, ev = relerr(mean[:, j], m1), relerr(var, v1)
            print(f"{kname} chunk 8 column {j}: mean {em:.2e} var {ev:.2e} ll {ll[j]!r} against {l1!r}")
            assert em < TOL and ev < TOL, (j, em, ev)
            np.testing.assert_allclose(ll[j], l1, rtol=1e-11, atol=0.0)


# ---- 6. a start time other than zero ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
def test_a_start_time_other_than_zero(kname):
    """t0 = -0.3 at eight steps per lane: the references on t + 0.3 (their first step starts from 0).  t0 may reach the first
    step of the series alone: every other lane takes the time before its chunk from ts."""
    from pssgp import _backend as Bk
    m, t0 = _m(kname), -0.3
    form, P, H = _form(kname)
    t, Y, tq = _case(m)
    ll_o, sums = _guard(kname, m, -t0)
    want = _ref(kname, m, K, -t0)
    _geometry(8, N), _geometry(8, N + K)
    got = _fresh(Bk.gp_predict_multi, form, P, H, t, Y, tq, chunk=8, t0=t0)
    ll = _fresh(Bk.gp_ll_multi, form, P, H, t, Y, chunk=8, t0=t0)
    grad = _fresh(Bk.gp_ll_grad_multi, form, P, H, t, Y, chunk=8, t0=t0)
    _check_columns(got, want, f"{kname} M {m} chunk 8 t0 {t0} predict")
    assert float(np.max(np.abs(ll - want[2]) / np.maximum(1.0, np.abs(want[2])))) < TOL
    _check_stats(grad, (ll_o, sums), f"{kname} M {m} chunk 8 t0 {t0} gradient")
    np.testing.assert_allclose(grad[0], ll, rtol=1e-11, atol=0.0)


# ---- 7. the gradient at every geometry ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("chunk", [1, 4, 8, 16])
def test_gradient_against_the_oracle(kname, chunk):
    """The kept states xs (nlanes x Lc x NX per group, strided (k - k0) x NX x nlanes) at 1, 4, 8 and 16 steps per lane, three
    groups side by side in one round, 19 to 2 workgroups."""
    from pssgp import _backend as Bk
    m = _m(kname)
    form, P, H = _form(kname)
    t, Y, _ = _case(m)
    ll_o, sums = _guard(kname, m)
    _geometry(chunk, N)
    got = _fresh(Bk.gp_ll_grad_multi, form, P, H, t, Y, chunk=chunk)
    again = _fresh(Bk.gp_ll_grad_multi, form, P, H, t, Y, chunk=chunk)
    ll = _fresh(Bk.gp_ll_multi, form, P, H, t, Y, chunk=chunk)
    assert all(np.all(np.isfinite(a)) for a in got)
    _check_stats(got, (ll_o, sums), f"{kname} M {m} chunk {chunk} gradient")
    np.testing.assert_allclose(got[0], ll, rtol=1e-11, atol=0.0)
    assert _same(got, again), "two calls differ"


# ---- 8. rounds of the gradient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("chunk", [8, 16])
def test_gradient_does_not_depend_on_the_rounds(kname, chunk):
    """As test 3 for the adjoint pass: one round of three groups, three rounds of one, rounds of two and one.  gpart is indexed
    by the group's place in the CALL, the slices of xs by its place in the round."""
    from pssgp import _backend as Bk
    m = _m(kname)
    form, P, H = _form(kname)
    t, Y, _ = _case(m)
    ll_o, sums = _guard(kname, m)
    lc, nb = _geometry(chunk, N)
    two = _grad_budget(kname, m, lc, nb)
    got, rounds = {}, {}
    with _CountReduce() as count:
        for name, budget in (("default", 0), ("one group", 1), ("two groups", two)):
            Bk.gp_ll_grad_multi(form, P, H, R, t, 1.0 - Y)                  # (as _fresh, outside the count)
            count.launches()
            with _Chunk(chunk), _BatchScratch(budget):
                got[name] = Bk.gp_ll_grad_multi(form, P, H, R, t, Y)
            rounds[name] = count.launches()
    print(f"{kname} M {m} chunk {chunk}: two-group budget {two} bytes, k_gpm_reduce launches {rounds}")
    assert rounds == {"default": 1, "one group": 3, "two groups": 2}
    _check_stats(got["default"], (ll_o, sums), f"{kname} M {m} chunk {chunk} gradient, one round")
    for name in ("one group", "two groups"):
        assert _same(got["default"], got[name]), f"the gradient depends on the rounds ({name} per round)"
