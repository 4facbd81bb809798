"""The column-tiled adjoint pass on the host (no GPU): the per-step arithmetic of the multi-output gradient kernels
(parallel-gps_amd/csrc/pgps_math.h: adj_step_m, adj_filtered_m, adj_element_m, adj_reverse_m -- what pgps_multi_grad.hip.h runs
per lane) is compiled with g++ and run as a whole sequential forward and reverse sweep (tests/cpu_math/multi_adj.cpp), with
the transition matrices and process noises of every step passed in from numpy.  Its statistics must equal the SUM over the
columns of the oracle's single-column reverse sweep (oracle/np_grad.py); the shared parts (E, L) of the tile's adjoint element
must be the single-column element's bit for bit, L counted once per existing column."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

from oracle import np_grad as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, MC, R = 61, 4, 0.1
TOL = 1e-12


def _has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return " fma " in f.read()
    except OSError:
        return False


FLAGS = [["-O2"]] + ([["-O2", "-mfma", "-ffp-contract=fast"]] if _has_fma() else [])


@pytest.fixture(scope="module", params=range(len(FLAGS)), ids=lambda i: " ".join(FLAGS[i]))
def harness(request, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("multi_adj") / "libmultiadj.so")
    subprocess.run(["g++"] + FLAGS[request.param] + ["-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "parallel-gps_amd", "csrc"),
                                                     os.path.join(ROOT, "tests", "cpu_math", "multi_adj.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    P = ctypes.c_void_p
    lib.multi_adj_sweep.argtypes = [ctypes.c_int, ctypes.c_long, ctypes.c_int, P, P, P, P, P, ctypes.c_double, P, P, P, P]
    return lib


def _sde(d):
    from pssgp.kernels import Matern12, Matern32, Matern52
    sde = {1: Matern12, 2: Matern32, 3: Matern52}[d](variance=1.3, lengthscales=0.7).get_sde()
    return (np.ascontiguousarray(sde.F, np.float64), np.ascontiguousarray(sde.P0, np.float64),
            np.ascontiguousarray(np.asarray(sde.H, np.float64).reshape(-1)))


@functools.lru_cache(maxsize=None)
def _case(d, nc):
    """Times, Y (N, nc) with 15 % of the rows missing -- the first and the last among them --, the steps' F_k and Q_k, and the
    oracle's statistics of every column: computed once, shared by the flag sets."""
    rng = np.random.RandomState(10 * d + nc)
    t = 0.1 + np.sort(rng.rand(N)) * 2.0
    Y = np.sin(3.0 * t)[:, None] * rng.uniform(0.5, 2.0, (1, nc)) + 0.3 * rng.randn(N, nc)
    miss = np.zeros(N, bool)
    miss[[0, N - 1]] = True
    others = rng.permutation(np.arange(1, N - 1))[:int(round(0.15 * N)) - 2]
    miss[others] = True
    assert miss.sum() == int(round(0.15 * N))
    Y[miss] = np.nan
    F, Pinf, h = _sde(d)
    dts = np.diff(np.concatenate([[0.0], t]))
    Fs = np.stack([sla.expm(dt * F) for dt in dts])
    Qs = np.stack([Pinf - Fk @ Pinf @ Fk.T for Fk in Fs])
    Qs = 0.5 * (Qs + np.swapaxes(Qs, 1, 2))
    cols = [G.ll_grad_stats(F, Pinf, h, R, t, Y[:, c]) for c in range(nc)]
    arrays = (np.ascontiguousarray(Y), np.ascontiguousarray(Fs), np.ascontiguousarray(Qs), np.ascontiguousarray(dts))
    for a in arrays:
        a.setflags(write=False)
    return arrays, (F, Pinf, h), cols


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("nc", [MC, MC - 1, 1], ids=lambda v: f"nc{v}")
def test_tile_sweep_equals_the_sum_of_the_columns(harness, d, nc):
    (Y, Fs, Qs, dts), (F, Pinf, h), cols = _case(d, nc)
    nst = d * d + 2 * d + 1
    stats, ll, chk = np.full(nst, np.nan), np.full(nc, np.nan), np.full(4, np.nan)
    p = lambda a: a.ctypes.data                                 # noqa: E731
    assert harness.multi_adj_sweep(d, N, nc, p(Fs), p(Qs), p(dts), p(Pinf), p(h), R, p(Y), p(stats), p(ll), p(chk)) == 0
    got = (stats[:d * d].reshape(d, d), stats[d * d:d * d + d], stats[d * d + d:d * d + 2 * d], stats[d * d + 2 * d:])
    for name, a, idx in zip(("Abar", "Ubar", "Hbar", "Rbar"), got, (1, 2, 3, 4)):
        want = np.sum([np.asarray(c[idx], np.float64) for c in cols], axis=0).reshape(a.shape)
        err = float(np.max(np.abs(a - want)) / np.max(np.abs(want)))
        print(f"d = {d} nc = {nc} {name}: {err:.2e}")
        assert err <= TOL, (name, err)
    for c in range(nc):
        assert abs(ll[c] - cols[c][0]) <= TOL * abs(cols[c][0]), c
    print(f"d = {d} nc = {nc}: shared parts that differ {chk[0]:.0f}, scan form a {chk[1]:.2e} B {chk[2]:.2e}, absent columns {chk[3]:.1e}")
    assert chk[0] == 0, "E or L of the tile's adjoint element is not the single-column element's (L times nc) bit for bit"
    # the scan form (suffix of the elements applied to (0, 0)) carries the same (a_c, B) as the sweep: both are O(N) chains of
    # d x d products in fp64
    assert chk[1] <= 1e-11 and chk[2] <= 1e-11
    assert chk[3] == 0.0, "an absent column did not stay at zero"


def test_automatic_route_bounds():
    """StateSpaceGP._multi_grad_pays: the measured bounds of the automatic route (its docstring has the numbers) -- from M = 3
    up to 2^16 steps, Matern-5/2 from M = 2 up to 2^17; never decided by anything but the kernel, N and M."""
    from pssgp.kernels import Matern12, Matern32, Matern52
    from pssgp.model import StateSpaceGP
    t, Y = np.linspace(0.1, 1.0, 8), np.zeros((8, 3))
    pays = {k.__name__: StateSpaceGP((t, Y), k(1.0, 1.0), 0.1, parallel=True)._multi_grad_pays for k in (Matern12, Matern32, Matern52)}
    for name in ("Matern12", "Matern32"):
        assert not pays[name](4096, 2) and pays[name](4096, 3) and pays[name](300, 5)
        assert pays[name](65536, 16) and not pays[name](65537, 16) and not pays[name](2 ** 20, 64)
    assert pays["Matern52"](4096, 2) and pays["Matern52"](131072, 16) and not pays["Matern52"](131073, 16)


def test_refusals_and_what_they_count():
    """The batched evaluations and the draws are single-output and take one shared noise variance.  A multi-output model is
    refused BEFORE the evaluation is counted (_n_eval decides when the series becomes resident); a single-output model with
    observation_variances is refused after it.  No library needed."""
    from pssgp.kernels import Matern32
    from pssgp.model import StateSpaceGP
    t, tq, thetas = np.linspace(0.1, 1.0, 8), np.linspace(0.2, 0.9, 3)[:, None], np.array([[1.0, 1.0, 0.1]])
    calls = {"predict_f_samples": lambda m: m.predict_f_samples(tq, num_samples=2, seed=1),
             "log_likelihood_batch": lambda m: m.log_likelihood_batch(thetas),
             "predict_f_batch": lambda m: m.predict_f_batch(tq, thetas),
             "log_likelihood_and_grad_batch": lambda m: m.log_likelihood_and_grad_batch(thetas)}
    multi = StateSpaceGP((t, np.zeros((8, 3))), Matern32(1.0, 1.0), 0.1, parallel=True)
    het = StateSpaceGP((t, np.zeros(8)), Matern32(1.0, 1.0), 0.1, parallel=True, observation_variances=np.full(8, 0.2))
    for name, call in calls.items():
        with pytest.raises(NotImplementedError) as e:
            call(multi)
        assert str(e.value) == f"{name} covers single-output models; this one has 3 output columns"
        assert getattr(multi, "_n_eval", 0) == 0
        before = getattr(het, "_n_eval", 0)
        with pytest.raises(NotImplementedError) as e:
            call(het)
        assert str(e.value) == (f"{name} is not available with observation_variances set (per-observation noise variances cover "
                                "maximum_log_likelihood_objective, predict_f and log_likelihood_and_grad)")
        assert het._n_eval == before + 1
