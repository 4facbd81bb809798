"""The resident one-launch filter + smoother (csrc/pgps_resident.hip.h) under a deterministic start skew.

The launch's grid-wide hand-offs are only exercised by the rest of the suite with every workgroup starting at about the
same moment.  Here one workgroup is held back (pgps_debug_resident_delay: 200 us, ten phases and more) before it publishes
its phase-1 total (the filtering spine) or its phase-2 total (the smoothing spine and the log-likelihood partial), and the
launch's spine records start as NaN, so a record read before its owner published it cannot match by luck.  Every output
of every form of the launch -- pkfs, pkf, the fused gp with smoothed moments and the fused log-likelihood alone -- is
compared with the three-launch path (shortcut off) and with the C oracle (the sequential restatement of the reference),
on data whose workgroup totals forget their past, remember it, or both, with the forgetting shortcut on and off.  The
wall-clock stamps the hook leaves show that the skew took effect.

The second half pins ragged series whose last workgroup is mostly padding behind a near-singular filtered covariance
(an almost exact observation at the series' last step)."""
import numpy as np
import pytest

from oracle import c_oracle as C
from tests.conftest import make_times, relerr, sample_series_fast

pytestmark = pytest.mark.gpu
PGPS_FAMILY_RESIDENT = 12
DELAY_US = 200              # a phase takes 15 - 20 us at 2^20 steps; every spin of the launch gives up only after ~1 s
TOL_3L = 1e-9               # against the three launches: same algebra, other bracketing
TOL_ORACLE = {"forgets": 1e-9, "remembers": 1e-8, "mixed": 1e-8}     # (test_gpu_resident.py: 1e-8 where the filter remembers)

GEOMETRIES = {"2^20x16": 1 << 20, "2^19x8": 1 << 19, "ragged": (1 << 19) + 4097}
FORMS = ("pkfs", "pkf", "gp", "gp_ll")
OUTPUTS = {"pkfs": ("fms", "fPs", "sms", "sPs", "ll"), "pkf": ("fms", "fPs", "ll"),
           "gp": ("fms", "fPs", "sms", "sPs", "ll"), "gp_ll": ("ll",)}


def _B():
    from pssgp import _backend
    return _backend


@pytest.fixture()
def ctx():
    c = _B().get_context()
    c.set_resident(1)
    c.set_shortcut(1)
    yield c
    c.debug_resident_delay(-1)
    c.set_resident(-1)
    c.set_shortcut(1)
    c.set_chunk(0)
    assert c.status() == 0


def _m32(ls=1.0, var=1.0):
    from pssgp.kernels import Matern32
    return Matern32(variance=var, lengthscales=ls)


def _nblocks(n):
    """The launch's geometry (pgps_res_inst.hip): 8 steps per lane while the series fits 2048 steps per CU, else 16."""
    lc = 8 if n <= 256 * 8 * 256 else 16
    return -(-n // (256 * lc))


# ------------------------------------------------------------------------------------------------
# data sets and their references (computed once per module)
# ------------------------------------------------------------------------------------------------
def _make(kind, n):
    B = _B()
    if kind == "remembers":
        # test_forgetting_shortcut_steps_aside_where_the_filter_remembers: lengthscale 2e4, long stretches without
        # observations covering whole workgroups (|A| of their totals O(1): the general fold behind the grid-wide wait)
        sde = _m32(ls=2.0e4).get_sde()
        t = make_times(n, seed=32)
        Fs, Qs = B.discretise(sde.F, sde.P0, t, 0.0)
        ssm = (sde.P0, Fs, Qs, sde.H, np.array([[0.1]]))
        y = sample_series_fast(ssm, seed=32)
        y[3000:int(0.343 * n)] = np.nan
        y[int(0.534 * n):int(0.534 * n) + 10] = np.nan
        y[int(0.687 * n):] = np.nan
    elif kind == "mixed":
        # test_resident_hand_offs_when_some_workgroups_remember_and_others_forget: stretches a million times denser
        rng = np.random.default_rng(n % 1000)
        sde = _m32(ls=1.0).get_sde()
        dt = 0.05 * rng.uniform(0.5, 1.5, n)
        for _ in range(3):
            a = int(rng.integers(0, n))
            dt[a:a + int(rng.integers(3000, 30000))] *= 1e-6
        t = np.cumsum(dt)
        Fs, Qs = B.discretise(sde.F, sde.P0, t, 0.0)
        ssm = (sde.P0, Fs, Qs, sde.H, np.array([[0.1]]))
        y = np.sin(0.7 * t) + 0.3 * rng.standard_normal(n)
        y[n // 3: n // 3 + 5000] = np.nan
    else:
        # config c2: every workgroup total forgets (the control)
        sde = _m32().get_sde()
        t = make_times(n, seed=11)
        Fs, Qs = B.discretise(sde.F, sde.P0, t, 0.0)
        ssm = (sde.P0, Fs, Qs, sde.H, np.array([[0.1]]))
        y = sample_series_fast(ssm, seed=11, nan_frac=0.05)
    return dict(kind=kind, n=n, sde=sde, t=t, ssm=ssm, y=y, r=0.1)


def _run(form, d):
    B = _B()
    if form == "pkfs":
        sms, sPs, fms, fPs, ll = B.pkfs(d["ssm"], d["y"], return_filtered=True, return_loglikelihood=True)
        return dict(fms=fms, fPs=fPs, sms=sms, sPs=sPs, ll=np.array([float(ll)]))
    if form == "pkf":
        fms, fPs, ll = B.pkf(d["ssm"], d["y"], return_loglikelihood=True)
        return dict(fms=fms, fPs=fPs, ll=np.array([float(ll)]))
    sde = d["sde"]
    smooth = form == "gp"
    out = B.gp(B.nilpotent_form(sde.F), sde.P0, np.asarray(sde.H).reshape(-1), d["r"], d["t"], d["y"],
               want_filtered=smooth, want_smoothed=smooth)
    got = {k: out[k] for k in OUTPUTS[form] if k != "ll"}
    got["ll"] = np.array([float(out["ll"])])
    return got


_CACHE = {}


def _dataset(kind, n):
    """(data, three-launch results of every form with the shortcut off, C oracle)"""
    key = (kind, n)
    if key not in _CACHE:
        c = _B().get_context()
        d = _make(kind, n)
        c.set_resident(0)
        c.set_shortcut(0)
        try:
            assert c.get_family(n, 2) != PGPS_FAMILY_RESIDENT
            three = {form: _run(form, d) for form in FORMS}
        finally:
            c.set_shortcut(1)
            c.set_resident(1)
        fms, fPs, sms, sPs, ll = C.kfs(d["ssm"], d["y"])
        oracle = dict(fms=fms, fPs=fPs, sms=sms, sPs=sPs, ll=np.array([ll]))
        _CACHE.clear()                  # one data set at a time: the parametrisation runs them in order
        _CACHE[key] = (d, three, oracle)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------
# the hook's evidence
# ------------------------------------------------------------------------------------------------
_LAST_STAMP = [0]


def _check_skew(ctx, n, tile, phase):
    """The stamps of THIS launch (newer than any seen before: a call that took another road would leave the previous
    launch's) show the armed workgroup waiting the whole delay and publishing after every other workgroup's publish of the
    same phase -- and, where phase 1 is held back, after workgroup 0 has run its Kalman pass and arrived a second time."""
    st = ctx.resident_stamps()
    nb = _nblocks(n)
    assert st.shape[0] == nb
    slot = 10 if phase == 1 else 11
    begin, ticks, pub = st[tile, 12], st[tile, 13], st[tile, slot]
    assert ticks > 0 and begin > _LAST_STAMP[0], "the delay did not run in this launch"
    assert pub - begin >= ticks, (pub, begin, ticks)
    others = np.delete(st[:, slot], tile)
    assert np.all(others > 0) and pub > others.max(), "the delayed workgroup was not the last to publish"
    if phase == 1:
        assert pub > st[0, 11] > 0, "workgroup 0's second arrival came after the delayed phase-1 publish"
    _LAST_STAMP[0] = int(st[:, 10:13].max())


def _compare(got, three, oracle, form, tol_oracle, tag, bad):
    for name in OUTPUTS[form]:
        g = np.asarray(got[name])
        if not np.all(np.isfinite(g)):
            bad.append(f"{tag} {name}: {int(np.sum(~np.isfinite(g)))} non-finite values")
            continue
        e3 = relerr(g, three[name])
        eo = relerr(g, oracle[name])
        if not e3 < TOL_3L:
            bad.append(f"{tag} {name}: rel err {e3:.3e} against the three launches")
        if not eo < tol_oracle:
            bad.append(f"{tag} {name}: rel err {eo:.3e} against the C oracle")


DELAYS = {"tile8-phase1": (8, 1), "tile1-phase1": (1, 1), "last-phase2": (-1, 2), "tile0-phase2": (0, 2)}


@pytest.mark.parametrize("delay", list(DELAYS))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("geom", list(GEOMETRIES))
@pytest.mark.parametrize("kind", ["remembers", "mixed", "forgets"])
def test_resident_hand_offs_under_start_skew(ctx, kind, geom, form, delay):
    """Tile 8 shares workgroup 0's counter shard (the grid-wide wait a second arrival of workgroup 0 could satisfy while
    tile 8 has not published), tile 1 is workgroup 0's right neighbour (the one-neighbour hand-off), the last tile's
    phase-2 total is what phase 3 and the log-likelihood sum wait for, and workgroup 0's is the log-likelihood sum's own.
    Shortcut on and off; every output finite and equal to both references."""
    n = GEOMETRIES[geom]
    d, three, oracle = _dataset(kind, n)
    tile, phase = DELAYS[delay]
    if tile < 0:
        tile = _nblocks(n) - 1
    if form in ("pkfs", "pkf"):
        assert ctx.get_family(n, 2, what=2 if form == "pkfs" else 0) == PGPS_FAMILY_RESIDENT
    bad = []
    for shortcut in (1, 0):
        ctx.set_shortcut(shortcut)
        ctx.debug_resident_delay(tile, phase, DELAY_US)
        try:
            got = _run(form, d)
        finally:
            ctx.debug_resident_delay(-1)
        assert ctx.status() == 0, "a spin of the resident launch gave up"
        _check_skew(ctx, n, tile, phase)
        _compare(got, three[form], oracle, form, TOL_ORACLE[kind], f"shortcut={shortcut}", bad)
    assert not bad, "\n".join(bad)


def test_resident_skewed_calls_on_changing_series(ctx):
    """Three skewed calls back to back on different series (other Fs, Qs and ys: a stale record of the previous call is
    a wrong one): each result equals its own references."""
    n = 1 << 19
    for kind in ("remembers", "mixed", "remembers"):
        d, three, oracle = _dataset(kind, n)
        bad = []
        ctx.debug_resident_delay(8, 1, DELAY_US)
        try:
            got = _run("pkfs", d)
        finally:
            ctx.debug_resident_delay(-1)
        assert ctx.status() == 0
        _check_skew(ctx, n, 8, 1)
        _compare(got, three["pkfs"], oracle, "pkfs", TOL_ORACLE[kind], kind, bad)
        assert not bad, "\n".join(bad)


def test_resident_delay_hook_disarms_and_validates(ctx):
    """The hook is diagnostics only: once disarmed, a launch neither waits nor writes wall-clock stamps (those of the armed
    launch before it stay as they were while the cycle stamps of mode 2 are new); out-of-range arguments are refused."""
    n = 1 << 17
    d = _make("forgets", n)
    ctx.debug_resident_delay(3, 1, DELAY_US)
    try:
        _run("pkfs", d)
    finally:
        ctx.debug_resident_delay(-1)
    _check_skew(ctx, n, 3, 1)
    armed = ctx.resident_stamps()
    ctx.set_resident(2)
    _run("pkfs", d)
    st = ctx.resident_stamps()
    assert st.shape == armed.shape
    assert np.array_equal(st[:, 10:14], armed[:, 10:14]) and np.all(st[:, 0] > 0) and np.all(st[:, 0] != armed[:, 0])
    for args in ((256, 1, 200), (0, 3, 200), (0, 0, 200), (0, 1, -1), (0, 1, 10001), (-2, 1, 200)):
        with pytest.raises(Exception):
            ctx.debug_resident_delay(*args)


# ------------------------------------------------------------------------------------------------
# ragged series behind a near-singular filtered covariance
# ------------------------------------------------------------------------------------------------
_ORACLE_NS = {}


def _near_singular(n, rfac):
    """Matern-3/2 observed at every step with R = rfac x variance: the filtered covariance of the last step is close to
    singular (eigenvalue ~ R along h), and the padded steps behind it (F = I, Q = 0) predict from exactly that P."""
    key = (n, rfac)
    if key not in _ORACLE_NS:
        B = _B()
        var = 1.0
        sde = _m32(ls=1.0, var=var).get_sde()
        t = make_times(n, seed=n % 991)
        Fs, Qs = B.discretise(sde.F, sde.P0, t, 0.0)
        R = rfac * var
        ssm = (sde.P0, Fs, Qs, sde.H, np.array([[R]]))
        y = sample_series_fast(ssm, seed=n % 991)
        ref = C.kfs(ssm, y)
        # the oracle's own conditioning: how far its answer moves when its inputs move by 8 units of round-off
        rng = np.random.default_rng(1)
        u = 8 * 2.0 ** -53
        pert = (sde.P0, Fs * (1 + u * rng.uniform(-1, 1, Fs.shape)), Qs * (1 + u * rng.uniform(-1, 1, Qs.shape)),
                sde.H, np.array([[R * (1 + u)]]))
        alt = C.kfs(pert, y * (1 + u * rng.uniform(-1, 1, n)))
        spread = max(max(relerr(a[-64:], b[-64:]) for a, b in zip(ref[:4], alt[:4])),
                     abs(ref[4] - alt[4]) / max(1.0, abs(ref[4])))
        _ORACLE_NS.clear()
        _ORACLE_NS[key] = (ssm, y, ref, spread)
    return _ORACLE_NS[key]


@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("rfac", [1e-8, 1e-12, 1e-15])
@pytest.mark.parametrize("n", [4096 + 5, (1 << 18) + 17, (1 << 20) - 4095])
def test_ragged_tail_behind_a_near_singular_filtered_covariance(ctx, n, rfac, resident):
    """The last workgroup is mostly padding (5, 17 and 4097 real steps of 4096 / 2048) and the step before the padding has an
    almost exact observation.  Every output finite; ll and the last 64 rows against the C oracle.

    Tolerance: the oracle is a backward-stable sequential pass; `spread` is how far its own answer moves when Fs, Qs, R and
    ys move by 8 units of round-off.  The scan evaluates the same operator in another bracketing, a backward error of
    O(log2 N) such perturbations: 100 x spread, and never tighter than the suite's fp64 tolerance (1e-9)."""
    ssm, y, ref, spread = _near_singular(n, rfac)
    tol = max(1e-9, 100.0 * spread)
    ctx.set_resident(1 if resident else 0)
    assert (ctx.get_family(n, 2) == PGPS_FAMILY_RESIDENT) == resident
    sms, sPs, fms, fPs, ll = _B().pkfs(ssm, y, return_filtered=True, return_loglikelihood=True)
    assert ctx.status() == 0
    got = dict(fms=fms, fPs=fPs, sms=sms, sPs=sPs)
    for name, g in got.items():
        assert np.all(np.isfinite(g)), f"{name}: {int(np.sum(~np.isfinite(g)))} non-finite values"
    for (name, g), want in zip(got.items(), ref[:4]):
        e = relerr(g[-64:], want[-64:])
        assert e < tol, f"{name}: last 64 rows rel err {e:.3e} >= {tol:.1e}"
    e = abs(float(ll) - ref[4]) / max(1.0, abs(ref[4]))
    assert np.isfinite(float(ll)) and e < tol, f"ll: rel err {e:.3e} >= {tol:.1e}"
