"""Joint posterior draws on the host: the draw definition, the backward-sampling twin
(pgps_seq_ks_sample_*) and StateSpaceGP(parallel=False).predict_f_samples, against numpy restatements and the dense GP.
No GPU needed."""
import math

import numpy as np
import pytest

from conftest import relerr
from oracle import np_oracle as O

M32 = 0xFFFFFFFF


def philox(ctr, key):
    """Philox4x32-10 (Random123): ctr four 32-bit words, key two."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def u53(a, b):
    return (((a << 21) | (b >> 11)) + 0.5) * 2.0 ** -53


def box_muller(w, f32=False):
    u, v = u53(w[0], w[1]), u53(w[2], w[3])
    if f32:
        u, v = np.float32(u), np.float32(v)
        r = np.sqrt(np.float32(-2) * np.log(u))
        a = np.float32(2 * math.pi) * v
        return float(r * np.cos(a)), float(r * np.sin(a))
    r = math.sqrt(-2.0 * math.log(u))
    return r * math.cos(2 * math.pi * v), r * math.sin(2 * math.pi * v)


def draws(seed, N, d, S, s0=0, f32=False):
    """the library's z (S, N, d), restated"""
    z = np.empty((S, N, d))
    for s in range(S):
        for k in range(N):
            for j in range((d + 1) // 2):
                a, b = box_muller(philox((k & M32, k >> 32, s0 + s, j), (seed & M32, seed >> 32)), f32)
                z[s, k, 2 * j] = a
                if 2 * j + 1 < d:
                    z[s, k, 2 * j + 1] = b
    return z


def psd_chol(M, scale):
    """semidefinite Cholesky factor with diagonal pivoting: the largest remaining diagonal entry is the pivot (lowest index
    on ties); stops when it is not above (d + 3) eps scale, the remaining columns zero.  C C^T = M, C not triangular."""
    d = M.shape[0]
    A = np.array(M, dtype=np.float64)
    C = np.zeros_like(A)
    tau = (d + 3) * 2.0 ** -52 * scale
    for j in range(d):
        p = int(np.argmax(np.diag(A)))
        if not A[p, p] > tau:
            break
        C[:, j] = A[:, p] * (1.0 / math.sqrt(A[p, p]))
        A -= np.outer(C[:, j], C[:, j])
        A[p, p] = 0.0
    return C


def np_backward_sample(ssm, fms, fPs, z):
    """section 1 of the definition in numpy: x_{N-1} = fm + C(fP) z, x_k = E_k x_{k+1} + g_k + C(L_k) z_k"""
    _, Fs, Qs, *_ = ssm
    S, N, d = z.shape
    x = np.empty((S, N, d))
    P = 0.5 * (fPs[-1] + fPs[-1].T)
    x[:, -1] = fms[-1] + z[:, -1] @ psd_chol(P, np.max(np.diag(P))).T
    for k in range(N - 2, -1, -1):
        F, Q, m, P = Fs[k + 1], Qs[k + 1], fms[k], 0.5 * (fPs[k] + fPs[k].T)
        Pp = F @ P @ F.T + Q
        E = np.linalg.solve(0.5 * (Pp + Pp.T), F @ P).T
        g = m - E @ (F @ m)
        EFP = E @ F @ P
        L = P - 0.5 * (EFP + EFP.T)
        x[:, k] = x[:, k + 1] @ E.T + g + z[:, k] @ psd_chol(L, np.max(np.diag(P))).T
    return x


def lib():
    from pssgp import _backend
    return _backend.load_library()


def merged_series(kernel, n=30, k=10, seed=0, noise=0.1):
    """~n training times, k query times (one duplicated, one equal to a training time), merged as predict_f does"""
    from pssgp.model import _merge_sorted
    rng = np.random.default_rng(seed)
    ts = np.cumsum(rng.uniform(0.05, 0.2, n))
    ys = np.sin(2 * ts) + 0.3 * rng.standard_normal(n)
    tq = np.sort(np.concatenate([rng.uniform(ts[0], ts[-1], k - 2), [ts[7]]]))
    tq = np.sort(np.concatenate([tq, [tq[3]]]))
    all_ts, all_ys, flags = _merge_sorted(ts, tq, (ys, np.full(tq.shape, np.nan)),
                                          (np.zeros(n, bool), np.ones(tq.shape, bool)))
    sde = kernel.get_sde()
    ssm = O.get_ssm(sde, all_ts, noise)
    return ts, ys, tq, all_ts, all_ys, flags, ssm


def test_philox_known_answers_and_library_word():
    assert philox((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert philox((M32,) * 4, (M32, M32)) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert philox((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    # the library's first pair under seed 0 is Box-Muller of the first vector's words
    from pssgp.kalman.sequential import sample_normals
    z = sample_normals(1, 2, 1, 0)
    assert np.max(np.abs(z[0, 0] - np.array(box_muller((0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8))))) < 1e-14


@pytest.mark.parametrize("d", [1, 2, 3, 5])
def test_normals_match_restatement(d):
    from pssgp.kalman.sequential import sample_normals
    seed = 0x1234_5678_9abc_def0
    want = draws(seed, 7, d, 3, s0=5)
    got = sample_normals(7, d, 3, seed, first_sample=5)
    assert np.max(np.abs(got - want)) < 1e-14
    got32 = sample_normals(7, d, 3, seed, first_sample=5, dtype=np.float32)
    assert got32.dtype == np.float32
    assert np.max(np.abs(got32 - draws(seed, 7, d, 3, s0=5, f32=True))) < 2e-6
    assert np.max(np.abs(got32 - want)) < 2e-5
    assert np.all(np.isfinite(got))


def test_ks_sample_zero_draws_are_smoothed_means(kernel_zoo):
    from pssgp.kalman.sequential import ks_sample
    for name, make, _, _ in kernel_zoo:
        *_, all_ys, flags, ssm = merged_series(make())
        fms, fPs = O.kf(ssm, all_ys)
        sms, _ = O.kfs(ssm, all_ys)
        N, d = fms.shape
        x = ks_sample(ssm, fms, fPs, 2, seed=3, z=np.zeros((2, N, d)))
        assert x.shape == (2, N, d)
        assert relerr(x[0], sms) < 1e-12, name
        assert relerr(x[1], sms) < 1e-12, name


def ss_joint_posterior(ssm, all_ys, flags):
    """dense conditioning of the joint state-space prior: Cov(f) over the merged steps, conditioned on the training rows"""
    P0, Fs, Qs, H, R = ssm
    N, d = Fs.shape[0], Fs.shape[1]
    h = H.reshape(d)
    Sig = np.zeros((N * d, N * d))
    P = P0
    for k in range(N):
        P = Fs[k] @ P @ Fs[k].T + Qs[k]
        Sig[k * d:(k + 1) * d, k * d:(k + 1) * d] = P
        for j in range(k - 1, -1, -1):              # Cov(x_k, x_j) = F_k Cov(x_{k-1}, x_j)
            Sig[k * d:(k + 1) * d, j * d:(j + 1) * d] = Fs[k] @ Sig[(k - 1) * d:k * d, j * d:(j + 1) * d]
            Sig[j * d:(j + 1) * d, k * d:(k + 1) * d] = Sig[k * d:(k + 1) * d, j * d:(j + 1) * d].T
    Hb = np.kron(np.eye(N), h[None, :])
    Kf = Hb @ Sig @ Hb.T
    tr, q = ~flags, flags
    A = Kf[np.ix_(tr, tr)] + float(np.asarray(R).reshape(())) * np.eye(int(tr.sum()))
    return Kf[np.ix_(q, q)] - Kf[np.ix_(q, tr)] @ np.linalg.solve(A, Kf[np.ix_(tr, q)])


def unit_vector_covariance(ssm, all_ys, flags, sampler):
    fms, fPs = O.kf(ssm, all_ys)
    N, d = fms.shape
    h = np.asarray(ssm[3]).reshape(d)
    Z = np.eye(N * d).reshape(N * d, N, d)
    out = sampler(ssm, fms, fPs, Z, h)
    out0 = sampler(ssm, fms, fPs, np.zeros((1, N, d)), h)
    A = (out - out0)[:, flags].T
    return A @ A.T, out0[0]


@pytest.mark.parametrize("name", ["matern12", "matern32", "matern52", "rbf6", "periodic2", "m32+m52", "m32*m52"])
def test_joint_covariance_from_unit_vectors(kernel_zoo, name):
    from pssgp.kalman.sequential import ks_sample
    _, make, spec, tol = next(z for z in kernel_zoo if z[0] == name)
    ts, ys, tq, _, all_ys, flags, ssm = merged_series(make())
    cov, mean0 = unit_vector_covariance(ssm, all_ys, flags,
                                        lambda s, m, P, z, h: ks_sample(s, m, P, z.shape[0], 0, z=z, H=h))
    assert np.all(np.isfinite(cov))
    if spec is not None:
        Kxx = O.dense_K(spec, ts, ts) + 0.1 * np.eye(ts.size)
        Kqx = O.dense_K(spec, tq, ts)
        want = O.dense_K(spec, tq, tq) - Kqx @ np.linalg.solve(Kxx, Kqx.T)
        assert relerr(cov, want) < (1e-8 if name.startswith("matern") else tol), name
    else:
        # rbf6: L_k is ill-conditioned (eigenvalues from 1e-16 to 1e-1 of the filtered covariance's scale); the pivoted
        # factor holds it to rounding (3.7e-14 measured; the unpivoted one gave 3.4e-9 here and 3.4e-1 on longer series:
        # test_sample_law.py)
        want = ss_joint_posterior(ssm, all_ys, flags)
        assert relerr(cov, want) < (4e-13 if name == "rbf6" else 1e-8), name
    # the zero draw is the smoothed mean (duplicate query and a query at a training time included)
    sms, _ = O.kfs(ssm, all_ys)
    assert relerr(mean0[flags], (sms @ np.asarray(ssm[3]).reshape(-1))[flags]) < 1e-12


def spaced_series(kernel, n=30, noise=0.1, seed=0):
    """training times with gaps of 0.5 .. 1.5 x 0.05, queries half-way between some of them, one at a training time and one
    duplicated: no near-coincident pair.  Between close but distinct times L_k is nearly singular, and the square root of
    its smallest pivots amplifies rounding differences between two implementations; tied and nearly tied
    times are test_gpu_sample_law.py's."""
    from pssgp.model import _merge_sorted
    rng = np.random.default_rng(seed)
    ts = np.cumsum(0.05 * rng.uniform(0.5, 1.5, n))
    ys = np.sin(2 * ts) + 0.3 * rng.standard_normal(n)
    tq = np.sort(np.concatenate([0.5 * (ts[3:-1:4] + ts[4::4]), [ts[9], ts[9]]]))
    all_ts, all_ys, flags = _merge_sorted(ts, tq, (ys, np.full(tq.shape, np.nan)),
                                          (np.zeros(n, bool), np.ones(tq.shape, bool)))
    return ts, ys, tq, all_ts, all_ys, flags, O.get_ssm(kernel.get_sde(), all_ts, noise)


def test_ks_sample_matches_numpy_restatement():
    from pssgp.kernels import Matern52
    from pssgp.kalman.sequential import ks_sample
    *_, all_ys, flags, ssm = spaced_series(Matern52(variance=1.3, lengthscales=0.4))
    fms, fPs = O.kf(ssm, all_ys)
    N, d = fms.shape
    z = draws(77, N, d, 4, s0=2)
    want = np_backward_sample(ssm, fms, fPs, z)
    assert relerr(ks_sample(ssm, fms, fPs, 4, 77, first_sample=2), want) < 1e-9
    assert relerr(ks_sample(ssm, fms, fPs, 4, 0, z=z), want) < 1e-9
    # the same draws in float32: rounding of P - E F P in float32 is amplified by the factor's small pivots (DESIGN.md 4o;
    # 1.7e-4 measured with the pivoted factor)
    x32 = ks_sample(tuple(np.asarray(a, np.float32) for a in ssm), fms.astype(np.float32), fPs.astype(np.float32), 4, 77,
                    first_sample=2)
    assert x32.dtype == np.float32 and relerr(x32, want) < 2e-3


def test_sampler_rejects_bad_arguments():
    import ctypes
    L = lib()
    z = np.empty(4)
    assert L.pgps_seq_sample_normals_f64(0, 1, 1, 0, 0, z.ctypes.data_as(ctypes.c_void_p)) == -1
    assert L.pgps_seq_sample_normals_f64(2, 1, 0, 0, 0, z.ctypes.data_as(ctypes.c_void_p)) == -1
    assert L.pgps_seq_ks_sample_f64(3, 40, None, None, None, None, 1, 0, 0, None, None, None) == -1
