"""GPU tests of the multi-output adjoint pass (pgps_gp_ll_grad_multi_*, _backend.gp_ll_grad_multi, StateSpaceGP with Y (N, M) in
log_likelihood_and_grad): the log-likelihoods of the M columns and the model's adjoints SUMMED over the columns come from one
filter pass and one reverse pass on column tiles (parallel-gps_amd/csrc/pgps_multi_grad.hip.h).  Kernels, noise and data are
those of test_gpu_multi_output.py.  Tolerances are the project's for device adjoints (test_gpu_adjoint.py: 1e-9 relative in the
max-norm of a statistic, with its 1e-6 floor), 1e-9 on every column's log-likelihood against the oracle and rtol 1e-11 against
the multi-column likelihood call."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import np_grad as G

pytestmark = pytest.mark.gpu

TOL = 1e-9
R = 0.1
# compiled tile widths (MultiGradTile in pgps_multi_grad.hip.h): d = 1 -> 8, d = 2 -> 4, d = 3 -> 2 columns per tile
TILE = {"m12": 8, "m32": 4, "m52": 2}
# (N, M): the issue's shapes, then M one below, at and one above every compiled tile width at N = 37
SHAPES = [(1, 1), (2, 2), (37, 3), (300, 5), (700, 9)] + [(37, m) for m in (1, 2, 4, 5, 7, 8, 9)]
NAMES = ("Abar", "Ubar", "Hbar", "Rbar")


def _kernel(kname):
    from pssgp.kernels import Matern12, Matern32, Matern52
    return {"m12": Matern12, "m32": Matern32, "m52": Matern52}[kname](variance=1.3, lengthscales=0.7)


def _model(kname):
    from pssgp import _backend as Bk
    sde = _kernel(kname).get_sde()
    return sde, (Bk.nilpotent_form(sde.F), np.asarray(sde.P0), np.asarray(sde.H).reshape(-1))


def _data(n, m, seed=0, extra_missing=()):
    """Sorted times, M noisy sines (the training half of test_gpu_multi_output._data).  From 30 rows on at least 10 % of the rows
    are missing in every column, among them row 0, the last row and a run of 5."""
    rng = np.random.RandomState(seed + 7 * n + m)
    t = 0.2 + np.sort(rng.rand(n)) * (n / 80.0 + 0.1)
    Y = np.sin(3.0 * t)[:, None] * rng.uniform(0.5, 2.0, (1, m)) + 0.3 * rng.randn(n, m)
    if n >= 30:
        miss = rng.rand(n) < 0.10
        miss[[0, n - 1]] = True
        miss[n // 3:n // 3 + 5] = True
        miss[list(extra_missing)] = True
        Y[miss] = np.nan
    return t, Y


@functools.lru_cache(maxsize=None)
def _oracle(kname, n, m, extra_missing=()):
    """The oracle's reverse sweep of every column: (ll (M,), [Abar, Ubar, Hbar, Rbar] summed over the columns, per statistic
    sum_c max|stat_c|).  Computed once, shared by the tests."""
    sde, _ = _model(kname)
    t, Y = _data(n, m, extra_missing=extra_missing)
    cols = [G.ll_grad_stats(sde.F, sde.P0, sde.H, R, t, Y[:, j]) for j in range(m)]
    ll = np.array([c[0] for c in cols])
    sums = [np.asarray(np.sum([np.asarray(c[i], np.float64) for c in cols], axis=0)) for i in range(1, 5)]
    mags = [float(np.sum([np.max(np.abs(c[i])) for c in cols])) for i in range(1, 5)]
    for a in [ll] + sums:
        a.setflags(write=False)
    return ll, sums, mags


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))


def _check_stats(got, want, what):
    """got = (ll (M,), Abar, Ubar, Hbar, Rbar) of the device; want = (ll (M,), [sums])."""
    ll, stats = got[0], got[1:]
    w_ll, w_stats = want
    assert ll.shape == w_ll.shape
    for j in range(w_ll.size):
        el = abs(ll[j] - w_ll[j]) / abs(w_ll[j])
        print(f"{what} column {j}: ll {el:.2e}")
        assert el <= TOL, (what, j, ll[j], w_ll[j])
    for name, a, b in zip(NAMES, stats, w_stats):
        e = _rel(a, b)
        print(f"{what} {name}: {e:.2e}")
        assert np.shape(a) == np.shape(b) and e <= TOL, (what, name, e)


@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-M%d" % s)
def test_against_the_oracle(kname, shape):
    from pssgp import _backend as Bk
    n, m = shape
    _, (form, P, H) = _model(kname)
    t, Y = _data(n, m)
    d = P.shape[0]
    got = Bk.gp_ll_grad_multi(form, P, H, R, t, Y)
    assert got[0].shape == (m,) and got[1].shape == (d, d) and got[2].shape == (d,) and got[3].shape == (d,)
    ll, sums, mags = _oracle(kname, n, m)
    # cancellation between the columns cannot hide an error: the sum is no smaller than 1/16 of its terms' magnitudes
    for name, s, mag in zip(NAMES, sums, mags):
        print(f"{kname} {shape} {name}: sum_c max|stat_c| / max|sum_c stat_c| = {mag / max(1e-300, float(np.max(np.abs(s)))):.2f}")
        assert mag <= 16.0 * float(np.max(np.abs(s))), (name, mag, float(np.max(np.abs(s))))
    _check_stats(got, (ll, sums), f"{kname} {shape}")


@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-M%d" % s)
def test_against_the_single_column_device_calls(kname, shape):
    from pssgp import _backend as Bk
    n, m = shape
    _, (form, P, H) = _model(kname)
    t, Y = _data(n, m)
    got = Bk.gp_ll_grad_multi(form, P, H, R, t, Y)
    packed = Bk.Series.pack(form, P, H)
    cols = []
    for j in range(m):
        ser = Bk.Series(t, np.ascontiguousarray(Y[:, j]))
        try:
            assert ser.has_gp_adj
            cols.append(ser.gp_ll_grad_adj(packed, R))
        finally:
            ser.close()
    sums = [np.sum([np.asarray(c[i], np.float64) for c in cols], axis=0) for i in range(1, 5)]
    _check_stats(got, (np.array([c[0] for c in cols]), sums), f"{kname} {shape} against the column calls")
    np.testing.assert_allclose(got[0], Bk.gp_ll_multi(form, P, H, R, t, Y), rtol=1e-11, atol=0.0)


class _Chunk:
    """pgps_set_chunk for the block, restored on every exit."""

    def __init__(self, steps):
        from pssgp import _backend as Bk
        self.ctx, self.steps = Bk.get_context(), steps

    def __enter__(self):
        self.ctx.set_chunk(self.steps)

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


@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
@pytest.mark.parametrize("straddle", [False, True], ids=["plain", "missing-run-across-workgroups"])
def test_several_workgroups_and_ragged_tail(kname, straddle):
    """Two steps per lane: 512 steps per workgroup, so the 1300 steps span three workgroups, the last one partly filled.
    `straddle`: rows 508..516 are missing -- a missing run on either side of the first workgroup boundary."""
    from pssgp import _backend as Bk
    n, m = 1300, 5
    extra = tuple(range(508, 517)) if straddle else ()
    _, (form, P, H) = _model(kname)
    t, Y = _data(n, m, extra_missing=extra)
    if straddle:
        assert np.all(np.isnan(Y[508:517]))
    with _Chunk(2):
        got = Bk.gp_ll_grad_multi(form, P, H, R, t, Y)
    ll, sums, _ = _oracle(kname, n, m, extra)
    _check_stats(got, (ll, sums), f"{kname} chunk 2 straddle={straddle}")


@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
@pytest.mark.parametrize("n,m,chunk", [(700, 9, 1), (700, 9, 3), (5000, 3, 0)], ids=lambda v: str(v))
def test_chunk_lengths_and_the_default_geometry(kname, n, m, chunk):
    from pssgp import _backend as Bk
    _, (form, P, H) = _model(kname)
    t, Y = _data(n, m)
    with _Chunk(chunk):
        got = Bk.gp_ll_grad_multi(form, P, H, R, t, Y)
    ll, sums, _ = _oracle(kname, n, m)
    _check_stats(got, (ll, sums), f"{kname} N {n} M {m} chunk {chunk}")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
def test_repeatable_whatever_the_rounds_and_columns_apart(kname):
    from pssgp import _backend as Bk
    n, m = 700, 9
    _, (form, P, H) = _model(kname)
    t, Y = _data(n, m)
    assert m > TILE[kname]                      # (more than one column group, so a small budget makes more than one round)
    first = Bk.gp_ll_grad_multi(form, P, H, R, t, Y)
    assert _same(first, Bk.gp_ll_grad_multi(form, P, H, R, t, Y)), "two calls differ"
    with _BatchScratch(4096):                   # (less than one group's scratch: one group per round)
        rounds = Bk.gp_ll_grad_multi(form, P, H, R, t, Y)
    assert _same(first, rounds), "the result depends on how the column groups are split into rounds"
    assert _same(first, Bk.gp_ll_grad_multi(form, P, H, R, t, Y))
    other = Y.copy()
    observed = ~np.isnan(Y[:, 0])
    keep = 4
    cols = [j for j in range(m) if j != keep]
    other[np.ix_(observed, cols)] = np.random.RandomState(1).randn(int(observed.sum()), m - 1)
    o = Bk.gp_ll_grad_multi(form, P, H, R, t, other)
    assert _bits(o[0][keep]) == _bits(first[0][keep]), "a column's log-likelihood depends on the other columns' data"
    assert not np.array_equal(o[0][cols], first[0][cols])


def test_abi_errors_and_the_dev_entry():
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    lib = ctx.lib
    n, m, d = 300, 5, 2
    _, (form, P, H) = _model("m32")
    lam, N1, N2 = form
    t, Y = _data(n, m)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)            # noqa: E731
    N1, N2, P, H = (np.ascontiguousarray(a, np.float64) for a in (N1, N2, P, H))
    nout = m + d * d + 2 * d + 1
    out = np.full(nout, np.nan)

    def host(M=m, dim=d, r=R, ys=Y):
        return lib.pgps_gp_ll_grad_multi_f64(ctx.handle, n, M, dim, lam, p(N1), p(N2), p(P), p(H), r, p(t), p(ys), 0.0, p(out))

    mixed = Y.copy()
    mixed[np.flatnonzero(~np.isnan(Y[:, 0]))[3], 2] = np.nan
    assert host(M=0) == -1                      # PGPS_E_INVALID
    assert host(dim=4) == -2                    # PGPS_E_UNSUPPORTED_DIM
    assert host(r=0.0) == -1
    assert host(ys=mixed) == -1
    # a valid call on the same context afterwards succeeds and is right
    assert host() == 0
    ll, sums, _ = _oracle("m32", n, m)
    split = lambda o: (o[:m], o[m:m + d * d].reshape(d, d), o[m + d * d:m + d * d + d], o[m + d * d + d:m + d * d + 2 * d],  # noqa: E731
                       o[m + d * d + 2 * d])
    _check_stats(split(out), (ll, sums), "after the refused calls")
    clean = out.copy()

    dev = {"t": ctx.malloc(t.nbytes), "y": ctx.malloc(Y.nbytes), "out": ctx.malloc(out.nbytes)}
    try:
        ctx.h2d(dev["t"], t), ctx.h2d(dev["y"], Y)
        rc = lib.pgps_gp_ll_grad_multi_dev_f64(ctx.handle, n, m, d, lam, p(N1), p(N2), p(P), p(H), R, ctypes.c_void_p(dev["t"]),
                                               ctypes.c_void_p(dev["y"]), 0.0, ctypes.c_void_p(dev["out"]))
        assert rc == 0
        ctx.synchronize()
        d_out = np.full(nout, np.nan)
        ctx.d2h(d_out, dev["out"])
        assert np.array_equal(_bits(d_out), _bits(clean)), "the device-pointer entry differs from the host-array entry"
    finally:
        for ptr in dev.values():
            ctx.free(ptr)


def _spy(monkeypatch):
    from pssgp import _backend as Bk
    calls = []
    real = Bk.gp_ll_grad_multi

    def spy(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(Bk, "gp_ll_grad_multi", spy)
    return calls


def _column_loop(kernel, t, Y, **kwargs):
    from pssgp.model import StateSpaceGP
    each = [StateSpaceGP((t[:, None], np.ascontiguousarray(Y[:, j:j + 1])), kernel(), R, parallel=True).log_likelihood_and_grad(**kwargs)
            for j in range(Y.shape[1])]
    return np.sum([e[0] for e in each]), np.sum([e[1] for e in each], axis=0)


def _check_model(model, want, **kwargs):
    ll, grad = model.log_likelihood_and_grad(**kwargs)
    np.testing.assert_allclose(ll, want[0], rtol=1e-11, atol=0.0)
    assert np.max(np.abs(grad - want[1])) <= TOL * np.max(np.abs(want[1])), (grad, want[1])
    return ll, grad


def test_model_takes_one_call(monkeypatch):
    from pssgp.kernels import RBF, Matern32
    from pssgp.model import StateSpaceGP
    n, m = 300, 5
    t, Y = _data(n, m)
    matern = lambda: Matern32(variance=1.3, lengthscales=0.7)          # noqa: E731
    calls = _spy(monkeypatch)
    kern = matern()
    model = StateSpaceGP((t, Y), kern, R, parallel=True)
    t_before, Y_before = model.data[0].copy(), model.data[1].copy()
    want = _column_loop(matern, t, Y)
    _, full = _check_model(model, want)
    assert len(calls) == 1, "the device route was not taken"
    _check_model(model, want)
    assert len(calls) == 2                      # exactly one call per log_likelihood_and_grad
    _check_model(model, want, method="adjoint")
    assert len(calls) == 3
    _check_model(model, _column_loop(matern, t, Y, method="dual"), method="dual")
    assert len(calls) == 3, "method='dual' must take the column loop"
    # wrt masks as on the single-column route
    _, part = model.log_likelihood_and_grad(wrt=[1])
    assert len(calls) == 4
    assert _bits(part[1]) == _bits(full[1]) and part[0] == 0.0 and part[2] == 0.0
    # the model's parameters and data are as they were
    assert float(kern.variance) == 1.3 and float(kern.lengthscales) == 0.7 and model.noise_variance == R
    assert np.array_equal(model.data[0], t_before) and np.array_equal(_bits(model.data[1]), _bits(Y_before))

    del calls[:]
    # a row that is NaN in one column only: the column loop, same values
    mixed = Y.copy()
    mixed[np.flatnonzero(~np.isnan(Y[:, 0]))[3], 1] = np.nan
    _check_model(StateSpaceGP((t, mixed), matern(), R, parallel=True), _column_loop(matern, t, mixed))
    # a kernel outside the Matern family: the column loop as well
    rbf = lambda: RBF(variance=1.2, lengthscales=0.8, order=4, balancing_iter=5)       # noqa: E731
    _check_model(StateSpaceGP((t, Y), rbf(), R, parallel=True), _column_loop(rbf, t, Y))
    # parallel=False has no gradient, on any route
    with pytest.raises(NotImplementedError):
        StateSpaceGP((t, Y), matern(), R, parallel=False).log_likelihood_and_grad()
    # one column never takes the new pass
    one = StateSpaceGP((t, np.ascontiguousarray(Y[:, :1])), matern(), R, parallel=True)
    _check_model(one, _column_loop(matern, t, Y[:, :1]))
    assert len(calls) == 0, "the column loop was not taken"
    # below the measured minimum of columns (StateSpaceGP._multi_grad_pays) the automatic choice is the loop; asked for by
    # name the pass runs
    two = StateSpaceGP((t, np.ascontiguousarray(Y[:, :2])), matern(), R, parallel=True)
    want = _column_loop(matern, t, Y[:, :2])
    _check_model(two, want)
    assert len(calls) == 0
    _check_model(two, want, method="adjoint")
    assert len(calls) == 1
