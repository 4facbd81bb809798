"""The joint posterior covariance between selected steps on the host (pgps_seq_ks_cov_*, sequential.ks_cov) and
StateSpaceGP(parallel=False).predict_f(X, full_cov=True): against dense conditioning of the joint
state-space prior, the oracle smoother and the dense GP (sample_law.py), against the law of the backward sampler's draws,
and against a numpy restatement of the recursion.  No GPU needed.  Errors are conftest.relerr, bounds TOL64 / TOL32."""
import functools

import numpy as np
import pytest

from conftest import relerr
from oracle import np_oracle as O
from sample_law import (MODELS, TOL32, TOL64, dense_f_posterior, diag_blocks, joint_state_posterior, law_case, project,
                        unit_vector_state_covariance)
from test_gpu_sample_law import REPEATED, TIES

N_LAW = 300


def np_cross_cov(ssm, fPs, sPs, sel):
    """Cov(x_i, x_j | ys) = E_i .. E_{j-1} sP_j (i < j) at the selected steps, (n d, n d): the gains
    E_k = fP_k F_{k+1}^T Pp_{k+1}^-1 of the smoothing elements multiplied out step by step"""
    _, Fs, Qs, _, _ = (np.asarray(a, np.float64) for a in ssm)
    sel = np.asarray(sel)
    n, d = len(sel), Fs.shape[1]
    out = np.zeros((n, d, n, d))
    for j in range(n):
        V = 0.5 * (sPs[sel[j]] + sPs[sel[j]].T)
        out[j, :, j, :] = V
        for i in range(j - 1, -1, -1):
            for k in range(sel[i + 1] - 1, sel[i] - 1, -1):
                F, P = Fs[k + 1], fPs[k]
                Pp = F @ P @ F.T + Qs[k + 1]
                V = np.linalg.solve(0.5 * (Pp + Pp.T), F @ P).T @ V
            out[i, :, j, :] = V
            out[j, :, i, :] = V.T
    return out.reshape(n * d, n * d)


def full(blocks):
    """(n, n, d, d) blocks -> (n d, n d)"""
    n, _, d, _ = blocks.shape
    return np.asarray(blocks, np.float64).transpose(0, 2, 1, 3).reshape(n * d, n * d)


def sub(want, sel, d):
    idx = (np.asarray(sel)[:, None] * d + np.arange(d)).reshape(-1)
    return want[np.ix_(idx, idx)]


@functools.lru_cache(maxsize=2)
def reference(name, ties=()):
    ssm, ts, ys, fms, fPs, spec = law_case(name, N_LAW, ties=ties)
    sms, sPs = O.kfs(ssm, ys)
    return ssm, ts, ys, fms, fPs, sPs, spec, joint_state_posterior(ssm, ys)


def selections(N, seed=3):
    rng = np.random.default_rng(seed)
    return {"random40": np.sort(rng.choice(N, 40, replace=False)), "adjacent": np.array([17, 18, 19, 140, 141]),
            "first_last_in": np.array([0, 5, 150, N - 1]), "first_last_out": np.array([1, 150, N - 2]),
            "single": np.array([123])}


def _ks_cov(ssm, fPs, sPs, sel, dtype, H=None):
    from pssgp.kalman.sequential import ks_cov
    out = ks_cov(tuple(np.asarray(a, dtype) for a in ssm), np.asarray(fPs, dtype), np.asarray(sPs, dtype), sel,
                 H=None if H is None else np.asarray(H, dtype).reshape(-1))
    assert out.dtype == dtype
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", MODELS)
def test_ks_cov_all_steps(name, dtype):
    """every step selected: the whole (N d, N d) joint against dense conditioning, its projection against the dense GP,
    its diagonal blocks against the oracle smoother; the projected output (H=) is the projection"""
    ssm, ts, ys, fms, fPs, sPs, spec, want = reference(name)
    N, d = fms.shape
    blocks = _ks_cov(ssm, fPs, sPs, np.arange(N), dtype)
    assert blocks.shape == (N, N, d, d)
    cov = full(blocks)
    errs = {"joint": relerr(cov, want), "blocks": relerr(diag_blocks(cov, N, d), sPs)}
    proj = _ks_cov(ssm, fPs, sPs, np.arange(N), dtype, H=ssm[3])
    assert proj.shape == (N, N)
    errs["projected"] = relerr(proj, project(want, ssm[3], N, d))
    if spec is not None:
        errs["dense"] = relerr(proj, dense_f_posterior(spec, ts, ys, 0.1))
    print(f"ks_cov {name} {np.dtype(dtype).name}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert np.array_equal(cov, cov.T) and np.array_equal(proj, proj.T)
    tol = TOL64 if dtype == np.float64 else TOL32
    for k, v in errs.items():
        assert v < tol, (name, k, v)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", MODELS)
def test_ks_cov_selections(name, dtype):
    ssm, ts, ys, fms, fPs, sPs, spec, want = reference(name)
    N, d = fms.shape
    tol = TOL64 if dtype == np.float64 else TOL32
    for label, sel in selections(N).items():
        e1 = relerr(full(_ks_cov(ssm, fPs, sPs, sel, dtype)), sub(want, sel, d))
        e2 = relerr(_ks_cov(ssm, fPs, sPs, sel, dtype, H=ssm[3]), project(sub(want, sel, d), ssm[3], len(sel), d))
        print(f"ks_cov {name} {np.dtype(dtype).name} {label}: states {e1:.2e} projected {e2:.2e}")
        assert max(e1, e2) < tol, (name, label, e1, e2)


@pytest.mark.parametrize("name", MODELS)
def test_ks_cov_tied_times(name):
    """a pair, a triple, a near-tie of 1e-9: the law against the dense reference; rows of exactly tied steps agree"""
    ssm, ts, ys, fms, fPs, sPs, spec, want = reference(name, TIES)
    N, d = fms.shape
    cov = full(_ks_cov(ssm, fPs, sPs, np.arange(N), np.float64))
    e = relerr(cov, want)
    gaps = []
    for k in REPEATED:
        assert ts[k + 1] == ts[k]
        gaps.append(float(np.max(np.abs(cov[k * d:(k + 1) * d] - cov[(k + 1) * d:(k + 2) * d])) / np.max(np.abs(cov))))
    sel = np.array([5, 9, 10, 21, 29, 30, 31, 200, 255, 256, 280])
    e_sel = relerr(full(_ks_cov(ssm, fPs, sPs, sel, np.float64)), sub(want, sel, d))
    print(f"ks_cov ties {name}: joint {e:.2e} selection {e_sel:.2e} tied rows {max(gaps):.2e}")
    assert max(e, e_sel, max(gaps)) < TOL64, (name, e, e_sel, gaps)


@pytest.mark.parametrize("name", MODELS)
def test_ks_cov_is_the_law_of_ks_sample(name):
    """the two features agree: A A^T of the sampler's unit-vector draws is ks_cov on all steps"""
    from pssgp.kalman.sequential import ks_sample
    ssm, ts, ys, fms, fPs, spec = law_case(name, 120)
    _, sPs = O.kfs(ssm, ys)
    AAt, _ = unit_vector_state_covariance(lambda s, m, P, z, h: ks_sample(s, m, P, z.shape[0], 0, z=z, H=h), ssm, fms, fPs,
                                          np.float64)
    e = relerr(full(_ks_cov(ssm, fPs, sPs, np.arange(120), np.float64)), AAt)
    print(f"ks_cov against ks_sample's law {name}: {e:.2e}")
    assert e < TOL64, (name, e)


@pytest.mark.parametrize("name", MODELS)
def test_ks_cov_is_the_numpy_recursion(name):
    ssm, ts, ys, fms, fPs, sPs, spec, want = reference(name)
    sel = selections(N_LAW)["random40"]
    e = relerr(full(_ks_cov(ssm, fPs, sPs, sel, np.float64)), np_cross_cov(ssm, fPs, sPs, sel))
    print(f"ks_cov against the numpy recursion {name}: {e:.2e}")
    assert e < TOL64, (name, e)


def test_invalid_selections_raise():
    from pssgp import _backend
    from pssgp.kalman.sequential import ks_cov
    ssm, ts, ys, fms, fPs, spec = law_case("matern_d2", 50)
    _, sPs = O.kfs(ssm, ys)
    for bad in ([3, 2], [4, 4], [-1, 3], [10, 50], []):
        with pytest.raises(ValueError):
            ks_cov(ssm, fPs, sPs, bad)
    # the C entry point itself
    lib = _backend.load_library()
    Fs, Qs = np.ascontiguousarray(ssm[1]), np.ascontiguousarray(ssm[2])
    out = np.empty((2, 2, 2, 2))
    p = _backend._ptr
    for bad in ([3, 2], [4, 4], [-1, 3], [10, 50]):
        sel = np.asarray(bad, np.int64)
        assert lib.pgps_seq_ks_cov_f64(50, 2, p(Fs), p(Qs), p(fPs), p(sPs), 2, p(sel), None, p(out)) == -1
    assert lib.pgps_seq_ks_cov_f64(50, 2, p(Fs), p(Qs), p(fPs), p(sPs), 0, p(np.zeros(1, np.int64)), None, p(out)) == -1
    assert lib.pgps_seq_ks_cov_f64(50, 40, p(Fs), p(Qs), p(fPs), p(sPs), 2, p(np.arange(2)), None, p(out)) == -2


# ------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------
def model_case(n=400, seed=11):
    rng = np.random.default_rng(seed)
    ts = np.cumsum(0.05 * rng.uniform(0.5, 1.5, n))
    ys = np.sin(2 * ts) + 0.3 * rng.standard_normal(n)
    xq = np.concatenate([rng.uniform(ts[0], ts[-1], 37), [ts[n // 3], ts[3 * n // 4] + 0.01, ts[3 * n // 4] + 0.01]])
    rng.shuffle(xq)
    return ts, ys, xq


def dense_posterior(spec, ts, ys, xq, noise):
    Kxx = O.dense_K(spec, ts, ts) + noise * np.eye(ts.size)
    Kqx = O.dense_K(spec, xq, ts)
    return Kqx @ np.linalg.solve(Kxx, ys), O.dense_K(spec, xq, xq) - Kqx @ np.linalg.solve(Kxx, Kqx.T)


def oracle_marginals(model, xq):
    """predict_f(xq) of the model by the oracle (sequential filter + smoother in numpy).  predict_f itself discretises on
    the device in both modes, so the host tests take the marginals from here; test_gpu_cov.py compares with predict_f"""
    ts, ys = model.data
    tq, inverse = np.unique(np.asarray(xq, np.float64), return_inverse=True)
    mean, var = O.ssgp_predict_f(model.kernel.get_sde(), np.asarray(ts, np.float64).reshape(-1),
                                 np.asarray(ys, np.float64).reshape(-1), float(model.noise_variance), tq, parallel=False)
    return mean[inverse], var[inverse]


def check_model_full_cov(model, xq, label, tol=TOL64, marginals=oracle_marginals):
    """shapes, exact symmetry, and the mean / the diagonal against the model's marginal predict_f"""
    K = xq.size
    mean, cov = model.predict_f(xq[:, None], full_cov=True)
    assert mean.shape == (K, 1) and cov.shape == (1, K, K), (mean.shape, cov.shape)
    assert np.array_equal(cov[0], cov[0].T)
    m0, v0 = marginals(model, xq)
    e_mean, e_diag = relerr(mean[:, 0], m0), relerr(np.diag(cov[0]), v0)
    print(f"predict_f full_cov {label}: mean {e_mean:.2e} diagonal {e_diag:.2e}")
    assert max(e_mean, e_diag) < tol, (label, e_mean, e_diag)
    return mean, cov


@pytest.mark.parametrize("name", ["matern12", "matern32", "matern52", "m32+m52"])
def test_predict_f_full_cov_host(kernel_zoo, name):
    """unsorted Xnew holding a training time and a duplicate, against the dense GP posterior"""
    from pssgp.model import StateSpaceGP
    _, make, spec, _ = next(z for z in kernel_zoo if z[0] == name)
    ts, ys, xq = model_case()
    model = StateSpaceGP((ts[:, None], ys[:, None]), make(), noise_variance=0.1, parallel=False)
    mean, cov = check_model_full_cov(model, xq, f"host {name}")
    want_mean, want_cov = dense_posterior(spec, ts, ys, xq, 0.1)
    e_m, e_c = relerr(mean[:, 0], want_mean), relerr(cov[0], want_cov)
    print(f"predict_f full_cov host {name} against the dense GP: mean {e_m:.2e} covariance {e_c:.2e}")
    assert max(e_m, e_c) < TOL64, (name, e_m, e_c)
    dup = np.flatnonzero(xq == ts[300] + 0.01)                  # (model_case: n = 400)
    assert dup.size == 2 and np.array_equal(cov[0][dup[0]], cov[0][dup[1]]) and np.array_equal(cov[0][:, dup[0]], cov[0][:, dup[1]])


def test_predict_f_full_cov_host_empty():
    from pssgp.kernels import Matern32
    from pssgp.model import StateSpaceGP
    ts, ys, xq = model_case(100)
    model = StateSpaceGP((ts[:, None], ys[:, None]), Matern32(1.0, 0.5), noise_variance=0.1, parallel=False)
    mean, cov = model.predict_f(np.zeros((0, 1)), full_cov=True)
    assert mean.shape == (0, 1) and cov.shape == (1, 0, 0)


def test_predict_f_full_cov_host_d8():
    """state dimensions above the device's lane-chunk limit run on the host"""
    from pssgp.kernels import RBF
    from pssgp.model import StateSpaceGP
    ts, ys, xq = model_case(200)
    kern = RBF(variance=1., lengthscales=0.5, order=8, balancing_iter=10)
    assert np.asarray(kern.get_sde().F).shape[0] == 8
    model = StateSpaceGP((ts[:, None], ys[:, None]), kern, noise_variance=0.1, parallel=False)
    check_model_full_cov(model, xq, "host rbf8")


def test_predict_f_full_cov_host_float32_model():
    from pssgp import config
    from pssgp.kernels import Matern32
    from pssgp.model import StateSpaceGP
    ts, ys, xq = model_case()
    want = StateSpaceGP((ts[:, None], ys[:, None]), Matern32(1.0, 0.5), noise_variance=0.1,
                        parallel=False).predict_f(xq[:, None], full_cov=True)
    config.set_default_float(np.float32)
    try:
        model = StateSpaceGP((ts[:, None].astype(np.float32), ys[:, None].astype(np.float32)), Matern32(1.0, 0.5),
                             noise_variance=0.1, parallel=False)
        mean, cov = check_model_full_cov(model, xq.astype(np.float32), "host float32 model", tol=TOL32)
    finally:
        config.set_default_float(np.float64)
    assert mean.dtype == np.float32 and cov.dtype == np.float32
    e_m, e_c = relerr(mean, want[0]), relerr(cov, want[1])
    print(f"predict_f full_cov float32 model against fp64: mean {e_m:.2e} covariance {e_c:.2e}")
    assert max(e_m, e_c) < TOL32
