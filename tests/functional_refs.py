"""Plain helpers of the functionals tests (test_functionals_host.py, test_gpu_functionals.py): kernels, series, the sequential
oracle's  C sm, C sP C^T  at the query rows, and the dense-GP laws of additive components and of derivatives."""
import math

import numpy as np

from oracle import np_oracle as O
from tests.conftest import make_times


def kernels():
    """The general-LTI kernels of tests/test_gpu_lti.py that the functionals tests use, plus the plain Matern ones and an RBF
    of order 16 (d = 16: every lane of a row live)."""
    from pssgp.kernels import Matern32, Matern52, RBF, Periodic, SquaredExponential
    return {
        "m32": lambda: Matern32(variance=1., lengthscales=0.5),                                              # d = 2
        "m52": lambda: Matern52(variance=1., lengthscales=0.5),                                              # d = 3
        "m32+m52": lambda: Matern32(variance=1., lengthscales=0.5) + Matern52(variance=1., lengthscales=0.5),  # d = 5
        "c5_qp_m52": lambda: Periodic(SquaredExponential(1., 1.), period=1., order=1) * Matern32(1., 1.) +
        Matern52(1., 1.),                                                                                     # d = 11
        "rbf15": lambda: RBF(variance=1., lengthscales=0.5, order=15, balancing_iter=10),                     # d = 15
        # (lengthscale 1.5, as test_gpu_lti.py's rbf20: at 0.5 the ORACLE is no reference at this order -- run on the case below
        # with its matrix-fraction Q and with sym(Pinf - F Pinf F^T) it differs from itself by 2e-4 max |ref| in H sm and 6e-3
        # in H F^2 sm, at 1.5 by 9e-10 and 4e-9: cond Pinf grows with order / lengthscale)
        "rbf16": lambda: RBF(variance=1., lengthscales=1.5, order=16, balancing_iter=10),                     # d = 16
        "co2_d18": lambda: Periodic(SquaredExponential(1., 1.), period=1., order=3) * Matern32(0.5, 5.) +
        Matern32(1., 2.),                                                                                     # d = 18
        "periodic10": lambda: Periodic(SquaredExponential(1., 0.8), period=1.5, order=10),                    # d = 22
    }


def series(n, seed):
    rng = np.random.default_rng(seed)
    t = make_times(n, seed=seed)
    y = np.sin(t) + 0.5 * np.cos(2.3 * t) + 0.3 * rng.standard_normal(n)
    return t, y


def powers_of_F(sde, n):
    """[H; H F; ...; H F^n] (n + 1, d) of the model -- rows whether or not f is that smooth: the smoother's algebra does not
    care."""
    F = np.asarray(sde.F, np.float64)
    rows = [np.asarray(sde.H, np.float64).reshape(-1)]
    for _ in range(n):
        rows.append(rows[-1] @ F)
    return np.stack(rows)


def oracle_lin(sde, C, R, t, y, tq):
    """(mean (K, J), cov (K, J, J), ll): the sequential filter + smoother of the oracle on the merged series (the C oracle above
    10^4 steps), then C sm and C sP C^T at the query rows."""
    C = np.asarray(C, np.float64)
    all_t, all_y, flags = O.merge_sorted(t, tq, (y, np.full(tq.shape, np.nan)),
                                         (np.zeros(t.shape, bool), np.ones(tq.shape, bool)))
    ssm = O.get_ssm(sde, all_t, R)
    if all_t.shape[0] > 10000:
        from oracle import c_oracle
        _, _, sms, sPs, ll = c_oracle.kfs(ssm, all_y)
    else:
        fms, fPs, ll, mps, Pps = O.kf(ssm, all_y, True, True)
        sms, sPs = O.ks(ssm, fms, fPs, mps, Pps)
    return sms[flags] @ C.T, np.einsum("ia,nab,jb->nij", C, sPs[flags], C), ll


def assert_close(got, want, tol, what=""):
    err = float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) if np.size(want) else 0.0
    bound = tol * max(1.0, float(np.max(np.abs(want)))) if np.size(want) else tol
    print(f"{what}: max |got - want| = {err:.3e}, bound {bound:.3e}")
    assert err < bound, (what, err, bound)


# -- dense GP laws -----------------------------------------------------------------------------------------------------------
def dense_components(specs, t, y, R, tq):
    """The posterior of the parts f_j of f = sum_j f_j, f_j ~ GP(0, k_j) independent, y = f(t) + noise:
    mean_j = K_j(X*, X) K_y^-1 y,  cov_ij = delta_ij K_j(x*, x*) - K_i(x*, X) K_y^-1 K_j(X, x*).  (mean (K, J), cov (K, J, J))."""
    t, y, tq = (np.asarray(a, np.float64).reshape(-1) for a in (t, y, tq))
    Ky = O.dense_K(("sum", list(specs)), t, t) + R * np.eye(t.size)
    Ks = [O.dense_K(s, tq, t) for s in specs]
    sol = [np.linalg.solve(Ky, k.T) for k in Ks]                    # K_y^-1 K_j(X, x*)
    alpha = np.linalg.solve(Ky, y)
    J = len(specs)
    mean = np.stack([k @ alpha for k in Ks], axis=1)
    cov = np.empty((tq.size, J, J))
    for i in range(J):
        for j in range(J):
            cov[:, i, j] = -np.sum(Ks[i] * sol[j].T, axis=1)
        cov[:, i, i] += np.diag(O.dense_K(specs[i], tq, tq))
    return mean, cov


def matern_dk(nu2, variance, ell, tau, order_s, order_t):
    """d^a/ds^a d^b/dt^b k(s - t) at tau = s - t for Matern-nu2/2 (nu2 = 3 or 5), in closed form.  With k(tau) = g(|tau|):
    d/ds = d/dtau, d/dt = -d/dtau, so the mixed derivative is (-1)^b k^(a+b)(tau)."""
    n = order_s + order_t
    return (-1.0) ** order_t * _matern_kn(nu2, variance, ell, np.asarray(tau, np.float64), n)


def _matern_kn(nu2, variance, ell, tau, n):
    """The n-th derivative of k with respect to tau (n <= 2 for Matern-3/2, n <= 4 for Matern-5/2)."""
    lam = math.sqrt(nu2) / ell
    r = np.abs(tau)
    s = np.sign(tau)
    e = np.exp(-lam * r)
    if nu2 == 3:
        # k = v (1 + lam r) e
        table = {0: (1 + lam * r) * e,
                 1: -s * lam ** 2 * r * e,
                 2: lam ** 2 * (lam * r - 1) * e}
    elif nu2 == 5:
        # k = v (1 + lam r + lam^2 r^2 / 3) e
        table = {0: (1 + lam * r + lam ** 2 * r ** 2 / 3) * e,
                 1: -s * (lam ** 2 * r / 3) * (1 + lam * r) * e,
                 2: (lam ** 2 / 3) * (lam ** 2 * r ** 2 - lam * r - 1) * e,
                 3: s * (lam ** 4 / 3) * r * (3 - lam * r) * e,
                 4: (lam ** 4 / 3) * (lam ** 2 * r ** 2 - 5 * lam * r + 3) * e}
    else:
        raise ValueError(nu2)
    return variance * table[n]


def dense_derivative(nu2, variance, ell, t, y, R, tq, order):
    """The posterior of f^(order) at tq for f ~ GP(0, Matern-nu2/2), y = f(t) + noise:
    mean = d^n_s k(x*, X) K_y^-1 y,  var = d^n_s d^n_t k(x*, x*) - d^n_s k(x*, X) K_y^-1 d^n_t k(X, x*).  (mean (K,), var (K,))."""
    t, y, tq = (np.asarray(a, np.float64).reshape(-1) for a in (t, y, tq))
    spec = ("matern32" if nu2 == 3 else "matern52", variance, ell)
    Ky = O.dense_K(spec, t, t) + R * np.eye(t.size)
    Ks = matern_dk(nu2, variance, ell, tq[:, None] - t[None, :], order, 0)          # Cov(f^(n)(x*), f(X))
    prior = float(matern_dk(nu2, variance, ell, 0.0, order, order))
    return Ks @ np.linalg.solve(Ky, y), prior - np.sum(Ks * np.linalg.solve(Ky, Ks.T).T, axis=1)
