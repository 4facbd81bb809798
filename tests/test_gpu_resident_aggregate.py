"""The lane's smoothing aggregate of the resident launch (csrc/pgps_resident.hip.h, res_agg_fold): e_0 (x) ... (x) e_{LC-1},
folded left to right inside the Kalman pass, started at the lane's first element, the last element joining it behind the
loop.  What can go wrong is the chain's two ends and its order, so the lengths stand at a lane's, a wave's and a workgroup's
edge -- where the last element comes from the next lane's registers, from the next wave or workgroup through global memory,
or is the series' last element (0, m, P) -- with 8 and 16 steps per lane, array form (pgps_pkfs_*) and fused form (pgps_gp_*).

Reference: the sequential filter + smoother on the CPU (oracle/kalman_seq.c, the C restatement of the reference's
sequential.py).  Tolerances: those of tests/test_gpu_resident.py -- 1e-9 relative (fp64, same algebra in another
bracketing), 1e-8 for the series that remembers (its totals are O(1) over tens of thousands of steps).  Observed on an
MI355X: at most 6e-15 in the ordinary cases, 3.1e-10 (smoothed means, fused form, 8 steps per lane) in the series that
remembers.  Every launch is made twice and must give the same bits.

The host test folds random chains with the library's own smth_combine both ways: from the identity element, and from the
chain's first element as the kernel does (the first link of the former is identity (x) e, which is e bit for bit)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import np_oracle as O
from oracle import c_oracle as C
from tests.conftest import make_times, relerr, sample_series_fast

TOL64 = 1e-9
TOL_REMEMBERS = 1e-8
PGPS_FAMILY_RESIDENT = 12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fms", "fPs", "sms", "sPs", "ll")


def _B():
    from pssgp import _backend
    return _backend


@pytest.fixture()
def ctx():
    c = _B().get_context()
    c.set_resident(1)
    yield c
    c.set_chunk(0)
    c.set_shortcut(1)
    c.set_resident(-1)
    assert c.status() == 0


def _m32(ls=1.0):
    from pssgp.kernels import Matern32
    return Matern32(variance=1.0, lengthscales=ls)


def _array(ssm, y):
    sms, sPs, fms, fPs, ll = _B().pkfs(ssm, y, return_filtered=True, return_loglikelihood=True)
    return dict(fms=fms, fPs=fPs, sms=sms, sPs=sPs, ll=np.array([float(ll)]))


def _fused(sde, t, y, r):
    B = _B()
    out = B.gp(B.nilpotent_form(sde.F), sde.P0, np.asarray(sde.H).reshape(-1), r, t, y, want_filtered=True, want_smoothed=True)
    return dict(fms=out["fms"], fPs=out["fPs"], sms=out["sms"], sPs=out["sPs"], ll=np.array([float(out["ll"])]))


def _problem(n, seed, ls=1.0):
    sde = _m32(ls).get_sde()
    t = make_times(n, seed=seed)
    ssm = tuple(np.asarray(a, np.float64) for a in O.get_ssm(sde, t, 0.1))
    return sde, t, ssm


def _run_and_check(ctx, lc, sde, t, ssm, y, tol, skip_ll=False):
    """array and fused form on the pinned resident launch, twice each, against the sequential oracle"""
    n = len(y)
    ctx.set_chunk(lc)
    assert ctx.get_family(n, 2) == PGPS_FAMILY_RESIDENT
    fms, fPs, sms, sPs, ll = C.kfs(ssm, y)
    want = dict(fms=fms, fPs=fPs, sms=sms, sPs=sPs, ll=np.array([ll]))
    for form, fn in (("array", lambda: _array(ssm, y)), ("fused", lambda: _fused(sde, t, y, 0.1))):
        got, again = fn(), fn()
        for name in NAMES:
            assert np.array_equal(got[name], again[name], equal_nan=True), f"{form} {name}: two runs differ"
            if name == "ll" and skip_ll:
                continue
            e = relerr(got[name], want[name])
            print(f"lc {lc} n {n} {form} {name}: rel err {e:.3e}")
            assert e < tol, f"{form} {name}: rel err {e:.3e} >= {tol}"


def _lengths(lc):
    return [1, 2, lc - 1, lc, lc + 1, 64 * lc - 1, 64 * lc, 64 * lc + 1, 256 * lc - 1, 256 * lc, 256 * lc + 1, 2 * 256 * lc + 77]


@pytest.mark.gpu
@pytest.mark.parametrize("lc,n", [(lc, n) for lc in (8, 16) for n in _lengths(lc)])
def test_aggregate_at_the_edges_of_lane_wave_and_workgroup(ctx, lc, n):
    """One step and two (the chain is its first element alone / never leaves the tail), a lane's chunk less one, full, plus
    one; the same around a wave's 64 lanes and a workgroup's 256; three workgroups, the last one ragged.  20 % of the
    observations missing at random."""
    sde, t, ssm = _problem(n, seed=n)
    y = sample_series_fast(ssm, seed=n, nan_frac=0.2 if n > 4 else 0.0)
    _run_and_check(ctx, lc, sde, t, ssm, y, TOL64)


@pytest.mark.gpu
@pytest.mark.parametrize("lc", [8, 16])
def test_aggregate_with_whole_lanes_missing(ctx, lc):
    """20 % missing at random plus stretches without any observation: one lane's whole chunk, exactly; a stretch over a wave's
    edge that covers whole lanes on both sides of it and begins and ends inside a chunk; and the series' last lanes."""
    n = 2 * 256 * lc + 77
    sde, t, ssm = _problem(n, seed=5)
    y = sample_series_fast(ssm, seed=5, nan_frac=0.2)
    y[70 * lc: 71 * lc] = np.nan
    y[62 * lc + 3: 67 * lc - 2] = np.nan
    y[256 * lc - 1: 256 * lc + lc + 1] = np.nan
    y[n - 3 * lc:] = np.nan
    _run_and_check(ctx, lc, sde, t, ssm, y, TOL64)


@pytest.mark.gpu
@pytest.mark.parametrize("shortcut", [1, 0])
@pytest.mark.parametrize("lc", [8, 16])
def test_aggregate_of_a_series_that_remembers_reaches_other_workgroups(ctx, lc, shortcut):
    """Length scale 2e4 steps (tests/test_gpu_resident.py, test_forgetting_shortcut_steps_aside_*) on three workgroups, the
    end of the first and nearly all of the middle one without observations: the smoothing totals' E is O(1), the general fold combines
    them, and a wrong lane aggregate anywhere shows in every workgroup to its left.  With the shortcut switched off the
    general fold runs whatever the totals are."""
    n = 2 * 256 * lc + 77
    sde, t, ssm = _problem(n, seed=32, ls=2.0e4)
    y = sample_series_fast(ssm, seed=32, nan_frac=0.2)
    y[200 * lc: 500 * lc + 5] = np.nan
    ctx.set_shortcut(shortcut)
    _run_and_check(ctx, lc, sde, t, ssm, y, TOL_REMEMBERS)


def _has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return " fma " in f.read()
    except OSError:
        return False


FLAGS = [["-O2"]] + ([["-O2", "-mfma", "-ffp-contract=fast"]] if _has_fma() else [])


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: " ".join(f))
def test_chain_started_at_its_first_element_is_the_chain_started_at_the_identity(flags, tmp_path):
    """identity (x) e_0 (x) e_1 ... against e_0 (x) e_1 ..., left to right, on random finite elements: single elements over
    forty orders of magnitude, chains of 8 and 16 over seven; every fourth chain ends in an element whose E is exactly zero
    (the series' last element) followed by elements near the identity (the padded steps).  Bit for bit, compiled as is and
    with contraction on as the device compiler does it."""
    so = str(tmp_path / "libresagg.so")
    subprocess.run(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "parallel-gps_amd", "csrc"),
                                      os.path.join(ROOT, "tests", "cpu_math", "res_aggregate.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)            # noqa: E731
    rng = np.random.default_rng(13)
    n, width = 2048, 9
    for lc in (1, 8, 16):
        span = 46.0 if lc == 1 else 8.0             # (a product of 16 factors of up to 1e20 would leave the fp64 range)
        x = rng.standard_normal((n, lc, width)) * np.exp(rng.uniform(-span, span, (n, lc, width)))
        if lc > 4:
            x[::4, lc - 3, 0:4] = 0.0                                          # E = 0: (0, m, P)
            x[::4, lc - 2:, :] = 1e-17 * rng.standard_normal((x[::4].shape[0], 2, width))
            x[::4, lc - 2:, 0] += 1.0                                          # E = I + rounding, g, L ~ rounding
            x[::4, lc - 2:, 3] += 1.0
        x = np.ascontiguousarray(x)
        out = np.empty((2 * n, width))
        assert lib.res_aggregate_chain_f64_d2(p(x), ctypes.c_long(n), ctypes.c_int(lc), p(out)) == width
        assert np.all(np.isfinite(out))
        assert np.array_equal(out[0::2].view(np.uint64), out[1::2].view(np.uint64)), f"chains of {lc} differ"
        if lc == 1:
            assert np.array_equal(out[1::2].view(np.uint64), x[:, 0].view(np.uint64))
