"""The law of the host twin's joint posterior draws (pgps_seq_ks_sample_*), exactly: the covariance A A^T taken from
unit-vector draws against dense conditioning of the joint state-space prior, the oracle smoother and the dense GP
(sample_law.py).  No GPU needed."""
import numpy as np
import pytest

from oracle import np_oracle as O
from sample_law import (MODELS, TOL32, TOL64, joint_state_posterior, law_case, law_errors, unit_vector_state_covariance)


def _ks(s, m, P, z, h):
    from pssgp.kalman.sequential import ks_sample
    return ks_sample(s, m, P, z.shape[0], 0, z=z, H=h)


def test_joint_state_posterior_is_the_smoother_and_the_dense_gp():
    """the reference against two independent ones: its diagonal blocks are the oracle smoother's covariances, its
    H-projection the dense GP posterior"""
    from conftest import relerr
    from sample_law import dense_f_posterior, diag_blocks, project
    for name in ("matern_d3", "m32*m52", "rbf6"):
        ssm, ts, ys, _, _, spec = law_case(name, 120)
        want = joint_state_posterior(ssm, ys)
        N, d = ssm[1].shape[:2]
        assert relerr(diag_blocks(want, N, d), O.kfs(ssm, ys)[1]) < 1e-11, name
        if spec is not None:
            assert relerr(project(want, ssm[3], N, d), dense_f_posterior(spec, ts, ys, 0.1)) < 1e-11, name


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", MODELS)
def test_ks_sample_law(name, dtype):
    """300 steps, the eight models, fp64 and float32 (Fs, Qs and the oracle's fp64 filtered moments rounded to float32).
    With the unpivoted factor three cases failed here: rbf6 1.7e-1 in fp64 and 8.6e-1 in float32, and the d = 6 Matern
    model 2.1e-2 in float32; now 9.2e-15, 7.3e-6 and 2.2e-6 (worst of all: d = 5 float32, 6.4e-5 joint, 1.2e-4 dense)."""
    ssm, ts, ys, fms, fPs, spec = law_case(name, 300)
    cov, mean0 = unit_vector_state_covariance(_ks, ssm, fms, fPs, dtype)
    errs = law_errors(cov, mean0, ssm, ts, ys, spec)
    print(f"ks_sample law {name} {np.dtype(dtype).name}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    tol = TOL64 if dtype == np.float64 else TOL32
    for k, v in errs.items():
        assert v < tol, (name, k, v)


@pytest.mark.parametrize("name", MODELS)
def test_ks_sample_law_projected(name):
    """the projected output (H=) carries the H-projection of the same law"""
    from conftest import relerr
    from sample_law import project
    ssm, ts, ys, fms, fPs, spec = law_case(name, 120)
    N, d = fms.shape
    cov, mean0 = unit_vector_state_covariance(_ks, ssm, fms, fPs, np.float64, H=ssm[3])
    want = joint_state_posterior(ssm, ys)
    assert relerr(cov, project(want, ssm[3], N, d)) < TOL64, name
    assert relerr(mean0, O.kfs(ssm, ys)[0] @ np.asarray(ssm[3]).reshape(d)) < TOL64, name


@pytest.mark.parametrize("name", ["matern32", "rbf6"])
def test_monte_carlo_window_reference_has_converged(name):
    """the reference of test_gpu_sample_law.py::test_predict_f_samples_monte_carlo_pairs: the dense GP posterior of a
    cluster given the training points within 40 lengthscales does not move when the window is halved"""
    from conftest import relerr
    from sample_law import mc_setup, window_posterior
    _, spec, ell, ts, _, xq, noise = mc_setup(name)
    for c in range(4):
        q = slice(4 * c, 4 * c + 4)
        assert np.ptp(xq[q]) <= ell
        assert relerr(window_posterior(spec, ts, xq[q], noise, 20 * ell), window_posterior(spec, ts, xq[q], noise, 40 * ell)) < 1e-6


def test_monte_carlo_dense_reference_describes_the_rbf6_model():
    """the dense squared-exponential GP is a reference for draws of the order-6 state-space model only where the two
    agree well inside the Monte Carlo resolution: at the case's noise variance every within-cluster entry of the model's
    own posterior covariance (sde_K, the model's stationary covariance function) is within one standard error of the
    sample covariance -- a sixth of the test's bound -- of the dense one.  At noise 0.1 it is 1.9 of the whole bound."""
    from sample_law import mc_setup, sde_K, window_posterior
    kern, spec, ell, ts, _, xq, noise = mc_setup("rbf6")
    sde = kern.get_sde()
    S = 16384

    def ratio(q, r):
        dense = window_posterior(spec, ts, q, r, 20 * ell)
        own = window_posterior(lambda a, b: sde_K(sde, a, b), ts, q, r, 20 * ell)
        bound = 6 * np.sqrt((np.outer(np.diag(dense), np.diag(dense)) + dense ** 2) / (S - 1))
        return float(np.max(np.abs(own - dense) / bound))
    for c in range(4):
        assert ratio(xq[4 * c:4 * c + 4], noise) < 1.0 / 6.0
    assert ratio(xq[:4], 0.1) > 1.0


def test_rbf6_own_covariance_reference():
    """sde_K is the covariance function of the rbf6 state-space model (against scipy's expm), its windowed posterior has
    converged at 20 lengthscales, and it is the law the state-space model conditions to (joint_state_posterior on a short
    series) -- which the squared-exponential kernel is not"""
    import scipy.linalg as sla
    from conftest import relerr
    from sample_law import dense_f_posterior, law_series, mc_setup, project, sde_K, window_posterior
    kern, _, ell, ts, _, xq, _ = mc_setup("rbf6")
    sde = kern.get_sde()
    P0, F, _, H, _ = (np.asarray(a, np.float64) for a in sde)
    h = H.reshape(-1)
    taus = np.array([0.0, 0.003, 0.1, 0.7, 3.0, 15.0])
    assert relerr(sde_K(sde, taus, [0.0])[:, 0], [h @ sla.expm(F * t) @ P0 @ h for t in taus]) < 1e-13

    def K(a, b):
        return sde_K(sde, a, b)
    q = xq[:4]
    assert relerr(window_posterior(K, ts, q, 0.1, 10 * ell), window_posterior(K, ts, q, 0.1, 20 * ell)) < 1e-6
    t, y = law_series(120)
    ssm = O.get_ssm(sde, t, 0.1)
    got = project(joint_state_posterior(ssm, y), h, 120, 6)
    obs = ~np.isnan(y)
    Kqx = K(t, t[obs])
    want = K(t, t) - Kqx @ np.linalg.solve(K(t[obs], t[obs]) + 0.1 * np.eye(int(obs.sum())), Kqx.T)
    assert relerr(got, want) < 1e-9
    assert relerr(got, dense_f_posterior(("rbf", 1.0, 0.5), t, y, 0.1)) > 1e-3
