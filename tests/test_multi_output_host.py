"""Multi-output StateSpaceGP on the host (no GPU): Y (N, M) is M independent GPs that share the kernel, the noise and the
inputs.  With parallel=False the model runs its column loop -- M internal single-column models -- so it must equal M
one-column models bit for bit; the column-tiled ("multi right-hand-side") algebra the device route is built on
(parallel-gps_amd/csrc/pgps_math.h: filt_extend_m, filt_combine_m, filt_apply_m, smth_combine_m, smth_apply_m) is compiled
with g++ and checked against four runs of the single-column functions."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import np_oracle as O
from pssgp.kernels import RBF, Matern32, Matern52
from pssgp.model import StateSpaceGP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, M = 40, 9, 3

KERNELS = {
    "matern32": (lambda: Matern32(variance=1.0, lengthscales=0.5), ("matern32", 1.0, 0.5)),
    "matern52": (lambda: Matern52(variance=1.0, lengthscales=0.5), ("matern52", 1.0, 0.5)),
    "rbf4": (lambda: RBF(variance=1.0, lengthscales=0.5, order=4, balancing_iter=5), None),
}


@pytest.fixture(autouse=True)
def host_discretisation(monkeypatch):
    """StateSpaceGP's sequential path builds its LGSSM through _backend.discretise, which runs on the device even with
    parallel=False; these tests have no GPU, so that one call takes the model's own host discretisation (expm per step)."""
    from pssgp import _backend, model
    monkeypatch.setattr(_backend, "discretise", lambda F, Pinf, ts, t0=0.0, device=0: model._host_discretise(F, Pinf, ts, t0))


def _data(seed=3):
    rng = np.random.RandomState(seed)
    t = np.sort(rng.rand(N)) * 4.0
    Y = np.sin(3.0 * t)[:, None] * np.array([1.0, -0.5, 2.0])[None, :] + 0.3 * rng.randn(N, M)
    tq = np.sort(rng.rand(K)) * 4.4
    return t, Y, tq


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _columns_equal_single_models(kernel, t, Y, tq):
    multi = StateSpaceGP((t[:, None], Y), kernel(), 0.1, parallel=False)
    assert multi.num_latent_gps == Y.shape[1]
    mean, var = multi.predict_f(tq[:, None])
    lls = multi.log_likelihood_columns()
    assert mean.shape == (tq.size, Y.shape[1]) and var.shape == (tq.size, Y.shape[1]) and lls.shape == (Y.shape[1],)
    singles = [StateSpaceGP((t[:, None], Y[:, j:j + 1]), kernel(), 0.1, parallel=False) for j in range(Y.shape[1])]
    want_ll = []
    for j, s in enumerate(singles):
        m1, v1 = s.predict_f(tq[:, None])
        assert _same_bits(mean[:, j], m1[:, 0]) and _same_bits(var[:, j], v1[:, 0]), j
        want_ll.append(s.maximum_log_likelihood_objective())
        assert _same_bits(lls[j], want_ll[-1]), j
    assert _same_bits(multi.maximum_log_likelihood_objective(), np.sum(np.asarray(want_ll, dtype=lls.dtype)))
    return mean, var, lls


@pytest.mark.parametrize("kname", list(KERNELS))
def test_loop_equals_m_models(kname):
    kernel, spec = KERNELS[kname]
    t, Y, tq = _data()
    mean, var, lls = _columns_equal_single_models(kernel, t, Y, tq)
    if spec is None:
        return
    for j in range(M):
        ll, m_d, v_d = O.dense_gp(spec, t, Y[:, j], 0.1, tq)
        assert abs(lls[j] - ll) < 1e-6 * abs(ll)
        assert np.max(np.abs(mean[:, j] - m_d)) < 1e-6 and np.max(np.abs(var[:, j] - v_d)) < 1e-6


def test_mixed_nan_rows_take_the_loop_and_match():
    t, Y, tq = _data(seed=5)
    Y[4, 1] = np.nan                    # one column is NaN where the others are not
    Y[17, 1] = np.nan
    Y[9, :] = np.nan                    # ... and a row missing everywhere
    _, var, _ = _columns_equal_single_models(KERNELS["matern32"][0], t, Y, tq)
    assert not np.array_equal(var[:, 0], var[:, 1])     # (the columns no longer share their covariances)


def test_shapes_setter_and_single_output_methods():
    t, Y, tq = _data()
    model = StateSpaceGP((t[:, None], Y), Matern32(1.0, 0.5), 0.1, parallel=False)
    mean, var = model.predict_f(tq[:, None])
    assert mean.shape == (K, M) and var.shape == (K, M)
    mean_c, cov = model.predict_f(tq[:, None], full_cov=True)
    assert mean_c.shape == (K, M) and cov.shape == (M, K, K)
    assert _same_bits(mean_c, mean)
    for j in range(1, M):
        assert _same_bits(cov[j], cov[0])
    assert np.max(np.abs(np.diagonal(cov, axis1=1, axis2=2).T - var)) < 1e-12
    # M = 1 keeps its shapes
    one = StateSpaceGP((t[:, None], Y[:, :1]), Matern32(1.0, 0.5), 0.1, parallel=False)
    m1, v1 = one.predict_f(tq[:, None])
    assert one.num_latent_gps == 1 and m1.shape == (K, 1) and v1.shape == (K, 1)
    assert one.predict_f(tq[:, None], full_cov=True)[1].shape == (1, K, K)
    assert one.log_likelihood_columns().shape == (1,)
    # the number of columns is fixed at construction
    with pytest.raises(ValueError):
        model.data = (t[:, None], Y[:, :2])
    with pytest.raises(ValueError):
        one.data = (t[:, None], Y)
    model.data = (t[:, None], 2.0 * Y)
    assert np.allclose(model.predict_f(tq[:, None])[0], 2.0 * mean, rtol=1e-12, atol=0.0)      # (the column loop was rebuilt)
    # the batch / sample evaluations are single-output
    two = StateSpaceGP((t[:, None], Y[:, :2]), Matern32(1.0, 0.5), 0.1, parallel=True)
    thetas = np.ones((2, 3))
    for call in (lambda: two.predict_f_samples(tq[:, None], 2), lambda: two.predict_f_batch(tq[:, None], thetas),
                 lambda: two.log_likelihood_batch(thetas), lambda: two.log_likelihood_and_grad_batch(thetas)):
        with pytest.raises(NotImplementedError):
            call()


# ---- the multi right-hand-side algebra on the host ---------------------------------------------------------------------
def _has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return " fma " in f.read()
    except OSError:
        return False


FLAGS = [["-O2"]] + ([["-O2", "-mfma", "-ffp-contract=fast"]] if _has_fma() else [])


@pytest.fixture(scope="module", params=range(len(FLAGS)), ids=lambda i: " ".join(FLAGS[i]))
def harness(request, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("multi_rhs") / "libmultirhs.so")
    subprocess.run(["g++"] + FLAGS[request.param] + ["-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "parallel-gps_amd", "csrc"),
                                                     os.path.join(ROOT, "tests", "cpu_math", "multi_rhs.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.multi_rhs_check.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    return lib


OPS = {"extend_observed": 0, "extend_missing": 1, "filt_combine": 2, "filt_apply": 3, "smth_combine": 4, "smth_apply": 5}


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("op", list(OPS))
def test_multi_rhs_algebra_equals_four_single_runs(harness, d, op):
    n = 400
    stream = np.ascontiguousarray(np.random.default_rng(100 * d + OPS[op]).standard_normal((n, 256)))
    out = np.full(2, np.nan)
    assert harness.multi_rhs_check(d, OPS[op], stream.ctypes.data, n, out.ctypes.data) == 0
    print(f"d = {d} {op}: shared parts that differ {out[0]:.0f}, column parts rel. err {out[1]:.2e}")
    assert out[0] == 0, "a shared part (A, C, J / E, L / P) is not bit-identical to the single-column function's"
    assert out[1] <= 1e-14
