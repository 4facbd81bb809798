"""GPU tests of the per-observation-noise kernels (k_gph_*) and the predictive-check kernels (k_gpl_*;
section 4w) at the launch geometries a realistic call has, which test_gpu_het_noise.py and test_gpu_loo.py (at most three steps
per lane, at most three workgroups) never reach:

  the LDS-staged road of the Kalman pass and of the smoother (whole sub-tiles of four steps per lane, a whole wave inside N);
  staged and unstaged waves in one workgroup (a ragged tail at four or eight steps per lane), an empty wave next to them;
  two sub-tiles per lane (eight steps per lane: the smoother's prefetch of the sub-tile before);
  the forgetting shortcut for the carry across workgroups (tried once a workgroup spans 2048 steps, decided per
  workgroup from the data), the general fold, and both side by side in one launch;
  a start time t0 other than zero.

Shapes (N, pgps_set_chunk, spacing of the times; het_refs.spaced_series), each checked against pgps_get_chunk before use:
  A  2600, 4, 0.05    three workgroups of 1024 steps; in the last one two waves are staged, one is ragged, one is empty; the
                      shortcut is not tried; rows 1020..1029 missing across the first workgroup boundary
  B  4696, 8, 0.05    three workgroups of 2048 steps, two sub-tiles per lane, a ragged tail; the shortcut is tried and every
                      workgroup total forgets
  C  4696, 8, 2e-4    the same geometry on a dense grid: Matern-3/2 and -5/2 remember (the general fold), Matern-1/2 forgets
  D  6744, 8, 0.05 but rows 2048..4095 at 2e-4: four workgroups; for Matern-3/2 and -5/2 workgroup 1 remembers and the others
                      forget, so the shortcut and the fold run side by side in the Kalman pass and in the smoother
  E  5000, 0, 0.05    the default geometry: four steps per lane, five workgroups

Which road a workgroup takes is asserted FROM THE REFERENCE, before the device is touched: het_refs.workgroup_forgetting gives
log2 max |A| and log2 max |E| of every workgroup total; the kernels' threshold is 2^-120, "forgets" here means <= -200 and
"remembers" >= -60, so no branch hangs on rounding.  The totals held to a band are those of the interior workgroups, the ones
whose reading decides something: A of a workgroup is read by its right neighbour in the Kalman pass, E by its left neighbour
in the smoother.  On the device A of the FIRST workgroup's total is exactly zero whatever the data (the first element of a
series carries the prior: filt_first) and so is E of the LAST (the last step has no smoother gain): there the shortcut is
always taken, with the fold's bits; A of the last and E of the first are read by nobody.

References (het_refs.py, loo_refs.py; none is the code under test): the numpy Kalman filter + RTS smoother at the project's
1e-9 (max norm relative to the largest entry) at every shape, dense algebra at kernel_zoo's 1e-6 at A.  Kernels: Matern-1/2,
-3/2, -5/2 with variance 1 and lengthscale 0.5; R = 0.1."""
import functools

import numpy as np
import pytest

from het_refs import MATERNS, R, dense_het, merged, queries, rel, sde_of, spaced_series, ss_het, workgroup_forgetting
from loo_refs import FIELDS, TOL, dense_checks, err, ss_checks
from oracle import np_oracle as O
from test_gpu_het_noise import _scalar_namesakes

pytestmark = pytest.mark.gpu

KNAMES = ("m12", "m32", "m52")
LANES, WAVE, SUBTILE = 256, 64, 4           # lanes per workgroup and per wave, steps per LDS-staged sub-tile (pgps_fused.hip.h)
SHORTCUT_SPAN = 2048                        # the launch code tries the shortcut from this many steps per workgroup
FORGETS, REMEMBERS = -200.0, -60.0          # log2 bands either side of the kernels' 2^-120
K = 50


def _spacing_d(n):
    sp = np.full(n, 0.05)
    sp[2048:4096] = 2e-4
    return sp


# name -> (N, pgps_set_chunk, spacing, steps per lane, workgroups, waves of the last workgroup of the N-step / (N + K)-step
# series: s staged, r ragged (unstaged), e empty)
SHAPES = {"A": (2600, 4, 0.05, 4, 3, "ssre"), "B": (4696, 8, 0.05, 8, 3, "sree"), "C": (4696, 8, 2e-4, 8, 3, "sree"),
          "D": (6744, 8, _spacing_d, 8, 4, "sree"), "E": (5000, 0, 0.05, 4, 5, "sssr"),
          # test 3's: B's size on D's spacing pattern (at B's own spacing 2048 steps forget through F alone, whatever the noise)
          "S": (4696, 8, _spacing_d, 8, 3, "sree")}
# the interior workgroups whose totals remember, per (shape, kernel); every other interior total forgets
REMEMBERING = {("C", "m32"): {1}, ("C", "m52"): {1}, ("D", "m32"): {1}, ("D", "m52"): {1}}
SHORTCUT_SHAPES = ("B", "C", "D")


class _Chunk:
    """pgps_set_chunk for the block, restored on every exit (with the shortcut setting)."""

    def __init__(self, steps):
        from pssgp import _backend as Bk
        self.ctx, self.steps = Bk.get_context(), steps

    def __enter__(self):
        self.ctx.set_chunk(self.steps)
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.set_shortcut(1)
        self.ctx.set_chunk(0)


def _form(kname):
    from pssgp import _backend as Bk
    sde = sde_of(kname)
    return Bk.nilpotent_form(sde.F), np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _case(shape, k=K):
    """(t, y, s, tq) of a shape: computed once, read-only."""
    n, _, spacing = SHAPES[shape][:3]
    t, y, s = spaced_series(n, spacing(n) if callable(spacing) else spacing)
    if shape == "A":
        y[1020:1030] = np.nan
    if shape == "S":
        s[2048:4096] = 1e9 * R
    return _frozen(t, y, s, queries(t, k))


@functools.lru_cache(maxsize=None)
def _ssm(kname, shape, k=0):
    """O.get_ssm of the shape's training times (k = 0) or of their merge with its k queries: shared by every reference."""
    t, y, s, tq = _case(shape, k or K)
    return O.get_ssm(sde_of(kname), merged(t, y, s, tq)[0] if k else t, 1.0)


@functools.lru_cache(maxsize=None)
def _loo_ref(kname, shape):
    t, y = _case(shape)[:2]
    return ss_checks(sde_of(kname), t, y, R, ssm=_ssm(kname, shape))


@functools.lru_cache(maxsize=None)
def _het_ref(kname, shape, k=K):
    """(ll, mean, var) of the state-space reference with the shape's s at its k queries"""
    t, y, s, tq = _case(shape, k)
    return ss_het(sde_of(kname), t, y, R, s, tq, ssm=_ssm(kname, shape, k))


@functools.lru_cache(maxsize=None)
def _forgetting(kname, shape, het, k=0):
    """workgroup_forgetting of the series a call filters: the training rows (k = 0) or their merge with the k queries, under
    R (het False) or R + s"""
    t, y, s, tq = _case(shape, k or K)
    Rk = R + s if het else np.full(t.size, R)
    if k:
        t, y, Rk, _ = merged(t, y, Rk, tq)
    return workgroup_forgetting(sde_of(kname), t, y, Rk, LANES * SHAPES[shape][3], ssm=_ssm(kname, shape, k))


def _geometry(shape, rows):
    """Steps per lane, workgroups and the last workgroup's waves of a `rows`-step call under the shape's pgps_set_chunk, read
    from the library (pgps_get_chunk: the geometry() every fused launch calls) and held to the table above."""
    from pssgp import _backend as Bk
    _, chunk, _, want_lc, want_nb, want_waves = SHAPES[shape]
    ctx = Bk.get_context()
    ctx.set_chunk(chunk)
    try:
        lc, nb = ctx.get_chunk(rows)
    finally:
        ctx.set_chunk(0)
    waves = ""
    for w in range(LANES // WAVE):
        base = ((nb - 1) * LANES + w * WAVE) * lc
        waves += "s" if base + WAVE * lc <= rows and lc % SUBTILE == 0 else ("r" if base < rows else "e")
    tried = LANES * lc >= SHORTCUT_SPAN
    print(f"shape {shape} rows {rows}: {lc} steps per lane ({lc // SUBTILE} sub-tiles), {nb} workgroups of {LANES * lc} steps, last "
          f"workgroup's waves {waves}, shortcut {'tried' if tried else 'not tried'}")
    assert (lc, nb, waves) == (want_lc, want_nb, want_waves), (shape, rows, lc, nb, waves)
    assert tried == (shape not in ("A", "E"))
    return lc, nb, tried


def _roads(kname, shape, het, k=0, remembering=None):
    """Asserts from the reference which interior workgroup totals forget and which remember; True where all of them forget
    (the shortcut is taken everywhere: both settings of pgps_set_shortcut give the same bits)."""
    f = _forgetting(kname, shape, het, k)
    nb = f.shape[0]
    want = REMEMBERING.get((shape, kname), set()) if remembering is None else remembering
    print(f"{kname} {shape} {'R + s' if het else 'R'}{f' merged with {k} queries' if k else ''}: log2 max|A| "
          + " ".join(f"{x:.0f}" for x in f[:, 0]) + "  log2 max|E| " + " ".join(f"{x:.0f}" for x in f[:, 1]))
    assert nb == SHAPES[shape][4] and f[nb - 1, 1] == -np.inf
    assert want <= set(range(1, nb - 1))
    for b in range(1, nb - 1):
        for x in f[b]:
            assert (x >= REMEMBERS) if b in want else (x <= FORGETS), (kname, shape, b, x)
    return not want


def _loo_errors(got, ref, rows=slice(None)):
    return [err(np.asarray(got[f])[rows], ref[f]) for f in FIELDS] + [abs(got[x] - ref[x]) / abs(ref[x]) for x in ("ll", "loo_lpd")]


def _het_errors(got, ref):
    """got, ref: (ll, mean, var)"""
    return [abs(got[0] - ref[0]) / abs(ref[0]), rel(got[1], ref[1]), rel(got[2], ref[2])]


def _same_bits(a, b, what):
    for name in a:
        assert np.array_equal(_bits(a[name]), _bits(b[name])), f"{what}: {name} differs"


# ---- 1. the predictive checks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("shape", ["A", "B", "C", "D", "E"])
def test_loo_against_the_references(kname, shape):
    from pssgp import _backend as Bk
    n, chunk = SHAPES[shape][:2]
    form, P, H = _form(kname)
    t, y = _case(shape)[:2]
    ref = _loo_ref(kname, shape)
    if _geometry(shape, n)[2]:
        _roads(kname, shape, False)
    if shape == "A":
        assert np.all(np.isnan(y[1020:1030]))
    with _Chunk(chunk):
        got = Bk.gp_loo(form, P, H, R, t, y)
        again = Bk.gp_loo(form, P, H, R, t, y)
        ll = float(Bk.gp(form, P, H, R, t, y)["ll"])              # (existing code: the log-likelihood of the same series)
    e = _loo_errors(got, ref)
    e_ll = abs(got["ll"] - ll) / abs(ll)
    print(f"{kname} {shape} loo against the state-space reference [osa_mean osa_var loo_mean loo_var ll loo_lpd] "
          + " ".join(f"{x:.2e}" for x in e) + f"; ll against gp {e_ll:.2e}; gap {ref['gap']:.3f}")
    assert max(e) <= TOL, e
    assert e_ll <= 1e-12
    nan = np.isnan(y)
    if shape == "A":
        e_dn = _loo_errors(got, dense_checks(MATERNS[kname][1], t, y, R), ~nan)
        print(f"{kname} {shape} loo against the dense reference " + " ".join(f"{x:.2e}" for x in e_dn))
        assert max(e_dn) <= MATERNS[kname][2], e_dn
    for name in ("osa", "loo"):
        logd = got[f"{name}_log_density"]
        assert logd.shape == (n,) and np.array_equal(np.isnan(logd), nan)
        assert np.all(np.isfinite(got[f"{name}_mean"])) and np.all(np.isfinite(got[f"{name}_var"]))
        assert err(logd[~nan], ref[f"{name}_log_density"][~nan]) <= TOL
    _same_bits({f: got[f] for f in FIELDS + ("ll", "loo_lpd")}, again, "two calls")


# ---- 2. per-observation noise: log-likelihood and predict -----------------------------------------------------------------
def _het_calls(kname, shape, k=K, t0=0.0):
    from pssgp import _backend as Bk
    form, P, H = _form(kname)
    t, y, s, tq = _case(shape, k)
    ll = Bk.gp_ll_het(form, P, H, R, t, y, s, t0=t0)
    mean, var, ll_p = Bk.gp_predict_het(form, P, H, R, t, y, s, tq, t0=t0)
    return {"ll": ll, "mean": mean, "var": var, "ll_p": ll_p}


def _het_check(got, ref, what):
    e = _het_errors((got["ll_p"], got["mean"], got["var"]), ref) + [abs(got["ll"] - ref[0]) / abs(ref[0])]
    print(f"{what} against the state-space reference [ll_p mean var ll] " + " ".join(f"{x:.2e}" for x in e))
    assert np.all(np.isfinite(got["mean"])) and np.all(np.isfinite(got["var"]))
    assert max(e) <= TOL, (what, e)


@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("shape", ["A", "B", "C", "D", "E"])
def test_het_ll_and_predict_against_the_references(kname, shape):
    n, chunk = SHAPES[shape][:2]
    t, y, s, tq = _case(shape)
    assert tq[0] < t[0] and tq[-1] > t[-1] and np.intersect1d(tq, t).size >= 5
    ref = _het_ref(kname, shape)
    if _geometry(shape, n)[2] & _geometry(shape, n + K)[2]:
        _roads(kname, shape, True)
        _roads(kname, shape, True, K)
    with _Chunk(chunk):
        got = _het_calls(kname, shape)
    _het_check(got, ref, f"{kname} {shape} het")
    if shape == "A":
        tol = MATERNS[kname][2]
        for a, b in zip((got["ll_p"], got["mean"], got["var"]), dense_het(MATERNS[kname][1], t, y, R, s, tq)):
            np.testing.assert_allclose(a, b, atol=tol, rtol=tol)


@pytest.mark.parametrize("kname", KNAMES)
def test_het_predict_with_many_queries(kname):
    """A with 1500 queries: 4100 merged steps, five workgroups (the last holds four steps: one lane), the query slots spread
    over staged and ragged waves."""
    from pssgp import _backend as Bk
    k = 1500
    n, chunk = SHAPES["A"][:2]
    form, P, H = _form(kname)
    t, y, s, tq = _case("A", k)
    assert np.all(np.diff(tq) >= 0) and np.intersect1d(tq, t).size >= k // 8
    with _Chunk(chunk) as ctx:
        assert ctx.get_chunk(n + k) == (4, 5)
        mean, var, ll_p = Bk.gp_predict_het(form, P, H, R, t, y, s, tq)
    e = _het_errors((ll_p, mean, var), _het_ref(kname, "A", k))
    print(f"{kname} A with {k} queries against the state-space reference [ll_p mean var] " + " ".join(f"{x:.2e}" for x in e))
    assert max(e) <= TOL, e
    tol = MATERNS[kname][2]
    for a, b in zip((ll_p, mean, var), dense_het(MATERNS[kname][1], t, y, R, s, tq)):
        np.testing.assert_allclose(a, b, atol=tol, rtol=tol)


# ---- 3. large error bars make a workgroup remember ------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
def test_large_error_bars_make_a_workgroup_remember(kname):
    """Shape S: rows 2048..4095 (workgroup 1) on the dense grid with s = 1e9 R -- observations that say nothing -- so its total
    is a product of F alone over a span of 0.4: it remembers whatever the kernel (Matern-1/2 included, whose total forgets on
    the same grid under the generator's s: shape C), while workgroup 0 forgets.  The decision comes from R + s_k, which only
    the het reduce sees."""
    n, chunk = SHAPES["S"][:2]
    assert _geometry("S", n)[2] & _geometry("S", n + K)[2]
    _roads(kname, "S", True, 0, {1})
    _roads(kname, "S", True, K, {1})
    ref = _het_ref(kname, "S")
    got = {}
    with _Chunk(chunk) as ctx:
        for on in (1, 0):
            ctx.set_shortcut(on)
            got[on] = _het_calls(kname, "S")
    for on in (1, 0):
        _het_check(got[on], ref, f"{kname} S het, shortcut {on}")
    e = [rel(got[1][x], got[0][x]) for x in got[1]]
    print(f"{kname} S: shortcut on against off " + " ".join(f"{x:.2e}" for x in e))
    assert max(e) <= 1e-12, e


# ---- 4. both roads --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("shape", SHORTCUT_SHAPES)
def test_loo_with_and_without_the_shortcut(kname, shape):
    from pssgp import _backend as Bk
    n, chunk = SHAPES[shape][:2]
    form, P, H = _form(kname)
    t, y = _case(shape)[:2]
    assert _geometry(shape, n)[2]
    all_forget = _roads(kname, shape, False)
    got = {}
    with _Chunk(chunk) as ctx:
        for on in (1, 0):
            ctx.set_shortcut(on)
            out = Bk.gp_loo(form, P, H, R, t, y)
            got[on] = {f: out[f] for f in FIELDS + ("ll", "loo_lpd")}
    for on in (1, 0):
        e = _loo_errors(got[on], _loo_ref(kname, shape))
        assert max(e) <= TOL, (on, e)
    if all_forget:
        _same_bits(got[1], got[0], "shortcut on and off")
    e = [err(got[1][f], got[0][f]) for f in got[1]]
    print(f"{kname} {shape} loo: shortcut on against off " + " ".join(f"{x:.2e}" for x in e)
          + (" (every total forgets: the same bits)" if all_forget else " (the general fold runs)"))
    assert max(e) <= 1e-12, e


@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("shape", SHORTCUT_SHAPES)
def test_het_with_and_without_the_shortcut(kname, shape):
    n, chunk = SHAPES[shape][:2]
    assert _geometry(shape, n)[2] & _geometry(shape, n + K)[2]
    all_forget = _roads(kname, shape, True) & _roads(kname, shape, True, K)
    got = {}
    with _Chunk(chunk) as ctx:
        for on in (1, 0):
            ctx.set_shortcut(on)
            got[on] = _het_calls(kname, shape)
    for on in (1, 0):
        _het_check(got[on], _het_ref(kname, shape), f"{kname} {shape} het, shortcut {on}")
    if all_forget:
        _same_bits(got[1], got[0], "shortcut on and off")
    e = [rel(got[1][x], got[0][x]) for x in got[1]]
    print(f"{kname} {shape} het: shortcut on against off " + " ".join(f"{x:.2e}" for x in e)
          + (" (every total forgets: the same bits)" if all_forget else " (the general fold runs)"))
    assert max(e) <= 1e-12, e


# ---- 5. the adjoint pair ----------------------------------------------------------------------------------------------------
def _rbar_by_differences(kname, shape, s):
    """d ll / d R of the state-space reference by Richardson-extrapolated central differences (steps 1e-3 R and 5e-4 R, as
    test_gpu_het_noise.py's dense gradient takes them: ll is analytic in R, the truncation error is O(h^4))."""
    t, y = _case(shape)[:2]
    ssm = _ssm(kname, shape)

    def central(h):
        return (ss_het(sde_of(kname), t, y, R + h, s, ssm=ssm) - ss_het(sde_of(kname), t, y, R - h, s, ssm=ssm)) / (2.0 * h)

    h = 1e-3 * R
    return (4.0 * central(0.5 * h) - central(h)) / 3.0


def _rbar_err(got, fd, ll):
    """The difference in units of |ll| / R.  What limits the reference is the rounding of ll in the difference quotient,
    eps |ll| / h with h a fixed fraction of R -- not the size of Rbar, which is the small remainder of two sums that cancel
    where R + s is close to the noise the data has (the per-observation case) and is not where it is R alone (the floor's)."""
    return abs(got - fd) / (abs(ll) / R)


# The floor of the difference quotient, measured on an MI355X on the scalar-noise model (s = 0, noise variance R) at the same
# shape against the existing device gradient pgps_gp_ll_grad_adj_dev_f64 (correct to 1e-9 by tests/test_gpu_adjoint.py),
# _rbar_err; the per-observation case is held to 10 x that floor, as test_gpu_het_noise.py holds its dense gradient.
RBAR_FLOOR = {("A", "m12"): 2.728e-12, ("A", "m32"): 2.632e-13, ("A", "m52"): 1.200e-12,
              ("B", "m12"): 5.367e-12, ("B", "m32"): 2.692e-12, ("B", "m52"): 2.206e-12}


@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("shape", ["A", "B"])
def test_het_adjoint_at_four_and_eight_steps_per_lane(kname, shape):
    """The xs scratch of the adjoint pair is Lc * NX * nlanes: four and eight steps per lane, three workgroups, a ragged tail.
    Constant s against the scalar adjoint at R + s; the generator's s: ll against the state-space reference, Rbar against its
    difference quotient in R.  Measured on an MI355X (_rbar_err): the floor -- s = 0, the scalar device gradient against the
    difference quotient -- is 2.728e-12 / 2.632e-13 / 1.200e-12 at A and 5.367e-12 / 2.692e-12 / 2.206e-12 at B (Matern-1/2 /
    -3/2 / -5/2), the bounds are 10 x that; the per-observation Rbar measured 4.377e-13 / 6.599e-13 / 1.662e-12 at A and
    2.831e-13 / 2.781e-12 / 2.558e-12 at B.  With constant s every statistic had the scalar call's bits.  The floor is
    measured again and printed by every run; it is the reference's error, not the code's, and is held to the same bound."""
    from pssgp import _backend as Bk
    n, chunk = SHAPES[shape][:2]
    form, P, H = _form(kname)
    t, y, s, tq = _case(shape)
    _geometry(shape, n)
    c = 0.037
    with _Chunk(chunk):
        const = Bk.gp_ll_grad_adj_het(form, P, H, R, t, y, np.full(n, c))
        w_const = _scalar_namesakes(kname, t, y, tq, R + c)[2]
        stats = Bk.gp_ll_grad_adj_het(form, P, H, R, t, y, s)
        w_plain = _scalar_namesakes(kname, t, y, tq, R)[2]
    e = [abs(const[0] - w_const[0]) / abs(w_const[0])] + [rel(a, b) for a, b in zip(const[1:], w_const[1:])]
    print(f"{kname} {shape} adjoint, constant s against R + c [ll Abar Ubar Hbar Rbar] " + " ".join(f"{x:.2e}" for x in e))
    assert max(e) <= TOL, e
    ll_ref = _het_ref(kname, shape)[0]
    assert abs(stats[0] - ll_ref) <= TOL * abs(ll_ref)
    assert all(np.all(np.isfinite(a)) for a in stats)
    floor = _rbar_err(w_plain[4], _rbar_by_differences(kname, shape, np.zeros(n)), w_plain[0])
    fd = _rbar_by_differences(kname, shape, s)
    e_het = _rbar_err(stats[4], fd, stats[0])
    print(f"{kname} {shape} Rbar: floor (s = 0, scalar device gradient {w_plain[4]:.6e}) {floor:.3e}, per-observation "
          f"{stats[4]:.6e} against the difference quotient {fd:.6e}: {e_het:.3e}")
    assert floor <= 10.0 * RBAR_FLOOR[shape, kname], (floor, RBAR_FLOOR[shape, kname])
    assert e_het <= 10.0 * RBAR_FLOOR[shape, kname], (e_het, RBAR_FLOOR[shape, kname])


# ---- 6. constant s equals the scalar entry points ---------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("shape", ["A", "B"])
def test_constant_s_equals_the_scalar_entry_points(kname, shape):
    """test_gpu_het_noise.py's comparison at the staged geometries; it also puts the scalar gp_predict on them."""
    from pssgp import _backend as Bk
    n, chunk = SHAPES[shape][:2]
    form, P, H = _form(kname)
    t, y, _, tq = _case(shape)
    c = 0.037
    s = np.full(n, c)
    _geometry(shape, n), _geometry(shape, n + K)
    with _Chunk(chunk):
        ll = Bk.gp_ll_het(form, P, H, R, t, y, s)
        mean, var, ll_p = Bk.gp_predict_het(form, P, H, R, t, y, s, tq)
        stats = Bk.gp_ll_grad_adj_het(form, P, H, R, t, y, s)
        w_ll, (w_mean, w_var, w_llp), w_stats = _scalar_namesakes(kname, t, y, tq, R + c)
    e = [abs(ll - w_ll) / abs(w_ll), abs(ll_p - w_llp) / abs(w_llp), rel(mean, w_mean), rel(var, w_var),
         abs(stats[0] - w_stats[0]) / abs(w_stats[0])] + [rel(a, b) for a, b in zip(stats[1:], w_stats[1:])]
    print(f"{kname} {shape}: constant s against R + c, [ll ll_p mean var | ll Abar Ubar Hbar Rbar] " + " ".join(f"{x:.2e}" for x in e))
    assert max(e) <= TOL, e
    # ... and the scalar predict itself against the reference at R + c
    e_w = _het_errors((w_llp, w_mean, w_var), ss_het(sde_of(kname), t, y, R, s, tq, ssm=_ssm(kname, shape, K)))
    print(f"{kname} {shape}: scalar gp_predict at R + c against the state-space reference " + " ".join(f"{x:.2e}" for x in e_w))
    assert max(e_w) <= TOL, e_w


# ---- 7. a start time other than zero ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
def test_a_start_time_other_than_zero(kname):
    """t0 = -0.3 at A: the references on t + 0.3 (their first step starts from 0)."""
    from pssgp import _backend as Bk
    chunk = SHAPES["A"][1]
    form, P, H = _form(kname)
    t, y, s, tq = _case("A")
    t0 = -0.3
    with _Chunk(chunk):
        loo = Bk.gp_loo(form, P, H, R, t, y, t0=t0)
        het = _het_calls(kname, "A", t0=t0)
    e = _loo_errors(loo, ss_checks(sde_of(kname), t - t0, y, R))
    print(f"{kname} A t0 {t0} loo " + " ".join(f"{x:.2e}" for x in e))
    assert max(e) <= TOL, e
    _het_check(het, ss_het(sde_of(kname), t - t0, y, R, s, tq - t0), f"{kname} A t0 {t0} het")
