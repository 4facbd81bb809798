"""The resident launch's output stores (csrc/pgps_resident.hip.h): the filtered covariances of a sub-tile leave while the next
sub-tile is computed, its L records wait for them, and the last sub-tile's leave around the chunk's last element.  What can go
wrong is a record drained after it was overwritten, an L record missing when phase 3 reads it, or a store past the series'
end -- so every call here runs on device buffers with guard rows behind row N, pre-filled with a NaN pattern: after the call
the guards hold the pattern and every row below N is finite.

Each case against the C oracle (oracle/c_oracle.py, the tolerance of tests/test_gpu_resident.py: 1e-9) and against the
three-launch path on the same inputs (1e-12: same algebra, other bracketing)."""
from ctypes import c_double, c_int, c_long

import numpy as np
import pytest

from oracle import np_oracle as O
from oracle import c_oracle as C
from tests.conftest import make_times, relerr, sample_series_fast

pytestmark = pytest.mark.gpu
TOL64 = 1e-9
TOL3 = 1e-12
PGPS_FAMILY_RESIDENT = 12
GUARD = 96                      # rows behind row N: more than a sub-tile of a lane (4 steps) and than a lane's chunk (16)
PATTERN = np.uint64(0x7FF8DEAD0000BEEF)     # a quiet NaN with a payload no computation produces


def _B():
    from pssgp import _backend
    return _backend


@pytest.fixture()
def ctx():
    c = _B().get_context()
    yield c
    c.set_chunk(0)
    c.set_resident(-1)
    assert c.status() == 0


class Series:
    """One series on the device, and the calls on it.  want: any of "f" (filtered moments), "s" (smoothed), "ll"."""

    SHAPES = dict(fms=2, fPs=4, sms=2, sPs=4)

    def __init__(self, ctx, n, seed, nan_frac=0.1, nan_at=()):
        from pssgp.kernels import Matern32
        B = _B()
        self.ctx, self.n = ctx, n
        sde = Matern32(variance=1.0, lengthscales=0.7).get_sde()
        t = make_times(n, seed=seed)
        self.ssm = tuple(np.asarray(a, np.float64) for a in O.get_ssm(sde, t, 0.1))
        y = sample_series_fast(self.ssm, seed=seed, nan_frac=nan_frac)
        for k in nan_at:
            y[k] = np.nan
        self.y = y
        P0, Fs, Qs, H, R = self.ssm
        self.R = float(np.asarray(R).reshape(-1)[0])
        lam, N1, N2 = B.nilpotent_form(sde.F)
        self.model = (lam, np.ascontiguousarray(N1, np.float64), np.ascontiguousarray(N2, np.float64),
                      np.ascontiguousarray(sde.P0, np.float64), np.ascontiguousarray(np.asarray(sde.H).reshape(-1), np.float64))
        self.dev = {}
        for name, arr in (("P0", P0), ("Fs", Fs), ("Qs", Qs), ("H", np.asarray(H, np.float64).reshape(-1)), ("ys", y), ("ts", t)):
            arr = np.ascontiguousarray(arr, np.float64)
            self.dev[name] = ctx.malloc(arr.nbytes)
            ctx.h2d(self.dev[name], arr)
        self.out = {k: ctx.malloc((n + GUARD) * m * 8) for k, m in self.SHAPES.items()}
        self.out["ll"] = ctx.malloc(8 * 2)

    def close(self):
        for p in list(self.dev.values()) + list(self.out.values()):
            self.ctx.free(p)

    def oracle(self):
        fms, fPs, sms, sPs, ll = C.kfs(self.ssm, self.y)
        return dict(fms=fms, fPs=fPs.reshape(self.n, 4), sms=sms, sPs=sPs.reshape(self.n, 4), ll=np.array([ll]))

    def _fill(self):
        for k, m in self.SHAPES.items():
            self.ctx.h2d(self.out[k], np.full((self.n + GUARD) * m, PATTERN, np.uint64))
        self.ctx.h2d(self.out["ll"], np.full(2, PATTERN, np.uint64))

    def _collect(self, written):
        """Every buffer back: the guards (and the whole of a buffer that was not requested) hold the pattern, the rows below N
        of a requested one are finite."""
        res = {}
        for k, m in self.SHAPES.items():
            raw = np.empty((self.n + GUARD) * m, np.uint64)
            self.ctx.d2h(raw, self.out[k])
            if k in written:
                assert np.all(raw[self.n * m:] == PATTERN), f"{k}: a store behind row N"
                res[k] = raw[:self.n * m].view(np.float64).reshape(self.n, m).copy()
                assert np.all(np.isfinite(res[k])), f"{k}: a row below N was not written (or is not finite)"
            else:
                assert np.all(raw == PATTERN), f"{k} was not requested and was written"
        raw = np.empty(2, np.uint64)
        self.ctx.d2h(raw, self.out["ll"])
        assert raw[1] == PATTERN
        if "ll" in written:
            res["ll"] = raw[:1].view(np.float64).copy()
            assert np.isfinite(res["ll"][0])
        else:
            assert raw[0] == PATTERN
        return res

    def run(self, form, want=("f", "s", "ll")):
        ctx, n, o, d = self.ctx, self.n, self.out, self.dev
        f = (o["fms"], o["fPs"]) if "f" in want else (None, None)
        s = (o["sms"], o["sPs"]) if "s" in want else (None, None)
        ll = o["ll"] if "ll" in want else None
        self._fill()
        if form == "array" and "s" in want:
            ctx.call("pgps_pkfs_dev_f64", c_long(n), c_int(2), d["P0"], d["Fs"], d["Qs"], d["H"], c_double(self.R), d["ys"],
                     f[0], f[1], s[0], s[1], ll)
        elif form == "array":
            ctx.call("pgps_pkf_dev_f64", c_long(n), c_int(2), d["P0"], d["Fs"], d["Qs"], d["H"], c_double(self.R), d["ys"],
                     f[0], f[1], ll)
        else:
            lam, N1, N2, Pinf, Hh = self.model
            P = _B()._ptr
            ctx.call("pgps_gp_dev_f64", c_long(n), c_int(2), c_double(lam), P(N1), P(N2), P(Pinf), P(Hh), c_double(0.1), d["ts"],
                     c_double(0.0), d["ys"], f[0], f[1], s[0], s[1], ll)
        ctx.synchronize()
        written = set()
        if "f" in want:
            written |= {"fms", "fPs"}
        if "s" in want:
            written |= {"sms", "sPs"}
        if "ll" in want:
            written.add("ll")
        return self._collect(written)

    def resident(self, lc, form, want=("f", "s", "ll")):
        self.ctx.set_resident(1)
        self.ctx.set_chunk(lc)
        assert self.ctx.get_family(self.n, 2, what=2 if "s" in want else 0) == PGPS_FAMILY_RESIDENT
        try:
            return self.run(form, want)
        finally:
            self.ctx.set_chunk(0)

    def three_launches(self, form, want=("f", "s", "ll")):
        self.ctx.set_chunk(0)
        self.ctx.set_resident(0)
        assert self.ctx.get_family(self.n, 2) != PGPS_FAMILY_RESIDENT
        try:
            return self.run(form, want)
        finally:
            self.ctx.set_resident(1)


def _check(got, want, tol):
    for name in got:
        e = relerr(got[name], want[name])
        assert e < tol, f"{name}: rel err {e:.3e} >= {tol}"


def _lengths(lc):
    """The series' end on a sub-tile boundary of a lane (4 steps), at the end of a wave's span (64 lc steps) -- each with one
    step less and one more -- and at a workgroup's end (256 lc), behind two whole workgroups."""
    wg, wave = 256 * lc, 64 * lc
    sub = 2 * wg + 37 * lc + 4
    wend = 2 * wg + 2 * wave
    return [sub - 1, sub, sub + 1, wend - 1, wend, wend + 1, 3 * wg]


CASES = [(lc, n) for lc in (8, 16) for n in _lengths(lc)]


@pytest.mark.parametrize("lc,n", CASES)
def test_series_ends_around_subtile_wave_and_workgroup_boundaries(ctx, lc, n):
    s = Series(ctx, n, seed=n % 1009)
    try:
        want = s.oracle()
        for form in ("array", "fused"):
            got = s.resident(lc, form)
            assert set(got) == set(want)
            _check(got, want, TOL64)
            _check(got, s.three_launches(form), TOL3)
    finally:
        s.close()


@pytest.mark.parametrize("lc", [8, 16])
def test_output_combinations(ctx, lc):
    """filtered + smoothed; smoothed only (the fused device entry point without fms, fPs: the Kalman pass stores nothing);
    the filter alone with the filtered moments; the log-likelihood alone."""
    n = 3 * 256 * lc + 64 * lc + 37 * lc + 5
    s = Series(ctx, n, seed=lc)
    try:
        want = s.oracle()
        for form in ("array", "fused"):
            ref = s.three_launches(form)
            _check(s.resident(lc, form, ("f", "s", "ll")), want, TOL64)
            got = s.resident(lc, form, ("f", "ll"))
            assert set(got) == {"fms", "fPs", "ll"}
            _check(got, want, TOL64)
            _check(got, ref, TOL3)
        ref = s.three_launches("fused")
        got = s.resident(lc, "fused", ("s", "ll"))
        assert set(got) == {"sms", "sPs", "ll"}
        _check(got, want, TOL64)
        _check(got, ref, TOL3)
        full = s.resident(lc, "fused", ("f", "s", "ll"))
        for k in got:                       # the same arithmetic whether or not the filtered moments are stored
            assert np.array_equal(got[k], full[k]), k
        got = s.resident(lc, "fused", ("ll",))
        assert set(got) == {"ll"}
        _check(got, want, TOL64)
        _check(got, ref, TOL3)
    finally:
        s.close()


@pytest.mark.parametrize("lc", [8, 16])
def test_missing_observations_at_the_edges_of_a_subtile(ctx, lc):
    """10 % of the observations missing, and one missing at the first and at the last step of a sub-tile -- the lane's first,
    its second and its last one, whose covariances leave around the chunk's last element -- of a lane in the middle of a
    wave, of a wave's first lane and of its last."""
    wg = 256 * lc
    n = 2 * wg + 777
    edges = []
    for lane_first in (wg + 21 * lc, wg + 64 * lc, wg + 127 * lc):
        edges += [lane_first, lane_first + 3, lane_first + 4, lane_first + 7, lane_first + lc - 4, lane_first + lc - 1]
    s = Series(ctx, n, seed=5 + lc, nan_frac=0.1, nan_at=edges)
    try:
        assert np.all(np.isnan(s.y[edges])) and 0.05 < np.mean(np.isnan(s.y)) < 0.15
        want = s.oracle()
        for form in ("array", "fused"):
            got = s.resident(lc, form)
            _check(got, want, TOL64)
            _check(got, s.three_launches(form), TOL3)
    finally:
        s.close()


@pytest.mark.parametrize("lc", [8, 16])
def test_two_identical_calls_return_identical_bytes(ctx, lc):
    n = 5 * 256 * lc - 3
    s = Series(ctx, n, seed=9)
    try:
        for form in ("array", "fused"):
            a = s.resident(lc, form)
            b = s.resident(lc, form)
            for k in a:
                assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (form, k)
    finally:
        s.close()
