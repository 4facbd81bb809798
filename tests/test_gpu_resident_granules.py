"""The resident launch's hand-offs as tagged granules (csrc/pgps_resident.hip.h), at the smallest sizes that still hand off.

A workgroup's total crosses to its neighbour as 8-byte {data, epoch} granules in two arrays the context owns: no flag, nothing
re-zeroed between launches, every granule judged by its tag alone.  So the cases here are the ones a tag can get wrong: a
record of an EARLIER launch taken for this one's (back-to-back launches on changing data, with series of alternating length
so that the records of the tiles beyond the shorter series are older still), the FIRST launch of a fresh context (zeroed
granules against epoch 1), a context whose workspace has moved in between, and a publisher that is late (the delay hook).

Sizes: 5 x 2048 + 3 steps at 8 steps per lane (six workgroups, the last one three steps long) and 2 x 4096 + 77 at 16 (three).
Every form of the launch -- pkfs, pkf, the fused gp with smoothed moments and the fused log-likelihood alone -- with the
forgetting shortcut on and off, on a series whose workgroup totals forget (config c2's model: the one-neighbour road) and on
one that remembers (a length scale of 2 x 10^4 steps, no observations over the whole of workgroup 1: the general fold over
every record).  References: the three-launch path with the shortcut off (1e-9: same algebra, other bracketing) and the C
oracle at the tolerances of test_gpu_resident_skew.py."""
import numpy as np
import pytest

from oracle import c_oracle as C
from tests.conftest import make_times, relerr, sample_series_fast

pytestmark = pytest.mark.gpu
PGPS_FAMILY_RESIDENT = 12
TOL_3L = 1e-9
TOL_ORACLE = {"forgets": 1e-9, "remembers": 1e-8}
SIZES = {"5x2048+3@8": (5 * 2048 + 3, 8), "2x4096+77@16": (2 * 4096 + 77, 16)}
FORMS = ("pkfs", "pkf", "gp", "gp_ll")
OUTPUTS = {"pkfs": ("fms", "fPs", "sms", "sPs", "ll"), "pkf": ("fms", "fPs", "ll"),
           "gp": ("fms", "fPs", "sms", "sPs", "ll"), "gp_ll": ("ll",)}
DELAY_US = 200


def _B():
    from pssgp import _backend
    return _backend


def _reset(c):
    c.debug_resident_delay(-1)
    c.set_resident(-1)
    c.set_shortcut(1)
    c.set_chunk(0)


@pytest.fixture()
def ctx():
    c = _B().get_context()
    c.set_resident(1)
    c.set_shortcut(1)
    yield c
    _reset(c)
    assert c.status() == 0


def _make(kind, size):
    from pssgp.kernels import Matern32
    B = _B()
    n, chunk = SIZES[size]
    dt = 0.05
    if kind == "remembers":
        sde = Matern32(variance=1.0, lengthscales=2.0e4 * dt).get_sde()
        t = make_times(n, seed=32, delta=dt)
    else:
        sde = Matern32(variance=1.0, lengthscales=1.0).get_sde()
        t = make_times(n, seed=11, delta=dt)
    Fs, Qs = B.discretise(sde.F, sde.P0, t, 0.0)
    ssm = (sde.P0, Fs, Qs, sde.H, np.array([[0.1]]))
    if kind == "remembers":
        y = sample_series_fast(ssm, seed=32)
        tile = 256 * chunk
        y[tile - 500:2 * tile + 300] = np.nan           # the whole of workgroup 1 and both of its borders
    else:
        y = sample_series_fast(ssm, seed=11, nan_frac=0.05)
    return dict(kind=kind, n=n, chunk=chunk, sde=sde, t=t, ssm=ssm, y=y, r=0.1)


def _run(form, d, y=None):
    B = _B()
    y = d["y"] if y is None else y
    if form == "pkfs":
        sms, sPs, fms, fPs, ll = B.pkfs(d["ssm"], y, return_filtered=True, return_loglikelihood=True)
        return dict(fms=fms, fPs=fPs, sms=sms, sPs=sPs, ll=np.array([float(ll)]))
    if form == "pkf":
        fms, fPs, ll = B.pkf(d["ssm"], y, return_loglikelihood=True)
        return dict(fms=fms, fPs=fPs, ll=np.array([float(ll)]))
    sde = d["sde"]
    smooth = form == "gp"
    out = B.gp(B.nilpotent_form(sde.F), sde.P0, np.asarray(sde.H).reshape(-1), d["r"], d["t"], y,
               want_filtered=smooth, want_smoothed=smooth)
    got = {k: out[k] for k in OUTPUTS[form] if k != "ll"}
    got["ll"] = np.array([float(out["ll"])])
    return got


def _oracle(d, y=None):
    fms, fPs, sms, sPs, ll = C.kfs(d["ssm"], d["y"] if y is None else y)
    return dict(fms=fms, fPs=fPs, sms=sms, sPs=sPs, ll=np.array([ll]))


_CACHE = {}


def _dataset(kind, size):
    """(data, three-launch results of every form with the shortcut off, C oracle): computed once and never changed"""
    key = (kind, size)
    if key not in _CACHE:
        c = _B().get_context()
        d = _make(kind, size)
        c.set_chunk(0)
        c.set_resident(0)
        c.set_shortcut(0)
        try:
            assert c.get_family(d["n"], 2) != PGPS_FAMILY_RESIDENT
            three = {form: _run(form, d) for form in FORMS}
        finally:
            c.set_shortcut(1)
            c.set_resident(1)
        _CACHE[key] = (d, three, _oracle(d))
    return _CACHE[key]


def _resident(c, d, shortcut=1):
    c.set_resident(1)
    c.set_chunk(d["chunk"])
    c.set_shortcut(shortcut)
    assert c.get_family(d["n"], 2) == PGPS_FAMILY_RESIDENT


def _compare(got, three, oracle, form, tol_oracle, tag, bad):
    for name in OUTPUTS[form]:
        g = np.asarray(got[name])
        if not np.all(np.isfinite(g)):
            bad.append(f"{tag} {name}: {int(np.sum(~np.isfinite(g)))} non-finite values")
            continue
        eo = relerr(g, oracle[name])
        print(f"{tag} {name}: rel err {eo:.3e} against the C oracle" +
              (f", {relerr(g, three[name]):.3e} against the three launches" if three is not None else ""))
        if three is not None and not relerr(g, three[name]) < TOL_3L:
            bad.append(f"{tag} {name}: rel err {relerr(g, three[name]):.3e} against the three launches")
        if not eo < tol_oracle:
            bad.append(f"{tag} {name}: rel err {eo:.3e} against the C oracle")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("kind", ["forgets", "remembers"])
def test_small_series_that_still_hand_off(ctx, kind, size, form):
    """Six and three workgroups: every output of every form equals both references, shortcut on (the neighbour's granules,
    polled) and off (every record behind the grid-wide wait)."""
    d, three, oracle = _dataset(kind, size)
    bad = []
    for shortcut in (1, 0):
        _resident(ctx, d, shortcut)
        got = _run(form, d)
        assert ctx.status() == 0, "a spin of the resident launch gave up"
        _compare(got, three[form], oracle, form, TOL_ORACLE[kind], f"shortcut={shortcut}", bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", ["forgets", "remembers"])
def test_no_launch_takes_a_stale_record(ctx, kind):
    """Forty launches back to back, the observations scaled by the launch's index (the means scale with them: a record of
    any earlier launch is wrong by a factor), the series alternating between six workgroups and three -- the records of
    workgroups 3 .. 5 are two launches old whenever the longer series runs.  Every output of every launch against the C
    oracle on that launch's data."""
    data = [_dataset(kind, size)[0] for size in SIZES]
    bad = []
    for it in range(40):
        d = data[it % 2]
        y = d["y"] * float(it + 1)
        _resident(ctx, d, 1)
        got = _run("pkfs", d, y)
        assert ctx.status() == 0, f"launch {it}: a spin of the resident launch gave up"
        _compare(got, None, _oracle(d, y), "pkfs", TOL_ORACLE[kind], f"launch {it}", bad)
    assert not bad, "\n".join(bad)


def test_fresh_context_and_moved_workspace():
    """The first launch of a context finds zeroed granules and runs at epoch 1; the granule arrays are the context's own, so
    a workspace that other calls have made grow (and move) in between takes no record with it."""
    B = _B()
    small, three_s, oracle_s = _dataset("remembers", "5x2048+3@8")
    other, three_o, oracle_o = _dataset("forgets", "2x4096+77@16")
    shared = B.get_context()
    fresh = None
    bad = []
    try:
        _reset(shared)
        fresh = B.Context(0)
        B._contexts[0] = fresh                      # the module-level entry points (pkfs, gp, discretise) run on it
        _resident(fresh, small, 1)
        got = _run("pkfs", small)                   # the context's first launch of any kind
        assert fresh.status() == 0
        _compare(got, three_s["pkfs"], oracle_s, "pkfs", TOL_ORACLE["remembers"], "first launch", bad)
        # the three-launch path on a longer series lays the workspace out again, far beyond what the resident launch asked for
        n = 1 << 16
        big = dict(small, n=n, t=make_times(n, seed=5))
        Fs, Qs = B.discretise(big["sde"].F, big["sde"].P0, big["t"], 0.0)
        big["ssm"] = (big["sde"].P0, Fs, Qs, big["sde"].H, np.array([[0.1]]))
        big["y"] = sample_series_fast(big["ssm"], seed=5)
        fresh.set_chunk(0)
        fresh.set_resident(0)
        assert fresh.get_family(n, 2) != PGPS_FAMILY_RESIDENT
        three_big = _run("pkfs", big)
        for d, three, oracle, kind in ((other, three_o, oracle_o, "forgets"), (small, three_s, oracle_s, "remembers")):
            for shortcut in (1, 0):
                _resident(fresh, d, shortcut)
                got = _run("pkfs", d)
                assert fresh.status() == 0
                _compare(got, three["pkfs"], oracle, "pkfs", TOL_ORACLE[kind], f"after growth, {kind}, shortcut={shortcut}", bad)
        # and a longer resident series on the grown workspace: 33 workgroups
        fresh.set_chunk(0)
        fresh.set_resident(1)
        assert fresh.get_family(n, 2) == PGPS_FAMILY_RESIDENT
        got = _run("pkfs", big)
        assert fresh.status() == 0
        _compare(got, three_big, _oracle(big), "pkfs", TOL_ORACLE["remembers"], "2^16 steps", bad)
    finally:
        B._contexts[0] = shared
        if fresh is not None:
            fresh.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("delay", ["tile1-phase1", "last-phase2"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("kind", ["forgets", "remembers"])
def test_a_late_publisher_at_the_small_sizes(ctx, kind, size, form, delay):
    """The delay hook holds back workgroup 1's filtering total or the last workgroup's smoothing total (and log-likelihood
    partial) for 200 us while the records start as NaN under tags no epoch equals: a granule taken before its owner stored
    it shows in every word behind it.  The launch before has left the consumers' caches warm with its own records."""
    d, three, oracle = _dataset(kind, size)
    nb = -(-d["n"] // (256 * d["chunk"]))
    tile, phase = (1, 1) if delay == "tile1-phase1" else (nb - 1, 2)
    bad = []
    for shortcut in (1, 0):
        _resident(ctx, d, shortcut)
        _run(form, d, d["y"] * 3.0)                 # other totals, in the same records
        ctx.debug_resident_delay(tile, phase, DELAY_US)
        try:
            got = _run(form, d)
        finally:
            ctx.debug_resident_delay(-1)
        assert ctx.status() == 0, "a spin of the resident launch gave up"
        st = ctx.resident_stamps()
        assert st.shape[0] == nb
        slot = 10 if phase == 1 else 11
        begin, ticks, pub = st[tile, 12], st[tile, 13], st[tile, slot]
        assert ticks > 0 and pub - begin >= ticks, "the delay did not run in this launch"
        others = np.delete(st[:, slot], tile)
        assert np.all(others > 0) and pub > others.max(), "the delayed workgroup was not the last to publish"
        _compare(got, three[form], oracle, form, TOL_ORACLE[kind], f"shortcut={shortcut}", bad)
    assert not bad, "\n".join(bad)
