"""The host halves of log_likelihood_and_grad_batch and of the lock-step HMC driver, without a device: the batched
contraction of a single Matern kernel's adjoints (StateSpaceGP._matern_grad_contract) against difference quotients of the
oracle's filter and against oracle/np_grad.py::contract; the lock-step HMC core on a callable; split-R-hat; the method's
argument contract.  The device half is tests/test_gpu_grad_batch.py."""
import numpy as np
import pytest

from oracle import np_grad as G
from tests.conftest import make_times

# (variance, lengthscale, R): the settings tests/test_gpu_adjoint.py holds the single call to
SETTINGS = np.array([(1.3, 0.7, 0.2), (0.9, 0.45, 0.12), (2.2, 1.1, 0.12), (1.1, 0.8, 0.25), (1.2, 0.6, 0.15)])


def _series(n, seed):
    rng = np.random.default_rng(seed)
    t = make_times(n, seed=seed)
    y = np.sin(t) + 0.5 * np.cos(2.3 * t) + 0.3 * rng.standard_normal(n)
    y[rng.uniform(size=n) < 0.15] = np.nan
    return t, y


def _matern(kname, s2=1.0, ell=1.0):
    from pssgp.kernels import Matern12, Matern32, Matern52
    return {"m12": Matern12, "m32": Matern32, "m52": Matern52}[kname](s2, ell)


def _stats_row(stats):
    ll, Abar, Ubar, Hbar, Rbar = stats
    return np.concatenate([[ll], np.asarray(Abar).reshape(-1), Ubar, Hbar, [Rbar]])


@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
def test_batched_contraction_of_the_matern_adjoints(kname):
    """stats from the oracle's reverse sweep at five settings -> the helper's (B, 3) gradients: equal to central differences
    of the oracle's filter (step 1e-6, 1e-4 max(1, |g|)) and to np_grad.contract on the kernel's sde_with_grads (1e-9)."""
    from pssgp.kernels.sde_grads import sde_with_grads
    from pssgp.model import StateSpaceGP
    t, y = _series(60, seed=7)
    k = _matern(kname)
    gp = StateSpaceGP((t[:, None], y[:, None]), k, noise_variance=0.1, parallel=False)
    params = gp.trainable_parameters()
    names = [n for _, n in params]
    assert names == ["variance", "lengthscales", "noise_variance"]
    table = gp._matern_table(SETTINGS, params)
    assert table is not None

    def ll_at(s2, ell, R):
        sde = _matern(kname, s2, ell).get_sde()
        return G.ll_only(sde.F, sde.P0, sde.H, R, t, y)

    stats, want = [], []
    for s2, ell, R in SETTINGS:
        kk = _matern(kname, s2, ell)
        sde, grads = sde_with_grads(kk)
        ref = G.ll_grad_stats(sde.F, sde.P0, sde.H, R, t, y)
        stats.append(_stats_row(ref))
        want.append(G.contract(ref, sde.H, grads))
    stats, want = np.stack(stats), np.stack(want)
    got = StateSpaceGP._matern_grad_contract(stats, table, names, SETTINGS[:, 1], SETTINGS[:, 0])
    assert got.shape == (5, 3)
    assert np.max(np.abs(got - want)) <= 1e-9 * max(1.0, float(np.max(np.abs(want))))
    h = 1e-6
    for b, row in enumerate(SETTINGS):
        for j in range(3):
            up, dn = row.copy(), row.copy()
            up[j] += h
            dn[j] -= h
            fd = (ll_at(*up) - ll_at(*dn)) / (2 * h)
            assert abs(got[b, j] - fd) <= 1e-4 * max(1.0, abs(fd)), (b, j, got[b, j], fd)
    # the columns follow `names`
    perm = ["noise_variance", "variance", "lengthscales"]
    got_p = StateSpaceGP._matern_grad_contract(stats, table, perm, SETTINGS[:, 1], SETTINGS[:, 0])
    assert np.array_equal(got_p, got[:, [2, 0, 1]])


def _normal_target(U):
    U = np.asarray(U, np.float64)
    return -0.5 * np.sum(U * U, axis=1), -U


def _run_core(target, U0, seeds, **kw):
    from pssgp.experiments.toy import hmc_chains_core
    rngs = [np.random.RandomState(s) for s in seeds]
    return hmc_chains_core(target, U0, n_samples=40, n_burnin=15, step_sizes=0.3, n_leapfrogs=4, rngs=rngs, **kw)


def test_lock_step_chains_are_independent_bit_for_bit():
    """Chain c of a C = 4 run on a 3-dimensional standard normal == the C = 1 run with chain c's seed and start, bitwise
    (samples, acceptance counts, last point, adapted step size)."""
    seeds = [11, 12, 13, 14]
    U0 = np.random.default_rng(0).standard_normal((4, 3))
    out, acc, U, eps = _run_core(_normal_target, U0, seeds)
    assert out.shape == (4, 40, 3) and np.all(np.isfinite(out))
    assert acc.min() > 0                                        # (the chains move)
    for c in range(4):
        o1, a1, u1, e1 = _run_core(_normal_target, U0[c:c + 1], seeds[c:c + 1])
        assert np.array_equal(o1[0], out[c]) and a1[0] == acc[c] and np.array_equal(u1[0], U[c]) and e1[0] == eps[c]


def test_a_chain_with_a_non_finite_target_rejects_alone():
    seeds = [21, 22, 23, 24]
    U0 = np.random.default_rng(1).standard_normal((4, 3))

    def broken(U):
        lp, g = _normal_target(U)
        lp, g = lp.copy(), g.copy()
        lp[2], g[2] = np.nan, np.nan
        return lp, g

    out, acc, U, _ = _run_core(_normal_target, U0, seeds)
    outb, accb, Ub, _ = _run_core(broken, U0, seeds)
    for c in (0, 1, 3):
        assert np.array_equal(outb[c], out[c]) and accb[c] == acc[c] and np.array_equal(Ub[c], U[c])
    assert accb[2] == 0 and np.array_equal(outb[2], np.broadcast_to(U0[2], (40, 3)))     # chain 2 never left its start


def _split_rhat_direct(x):
    C, n, P = x.shape
    h = n // 2
    seqs = [x[c, :h] for c in range(C)] + [x[c, n - h:] for c in range(C)]
    m = len(seqs)
    out = np.zeros(P)
    for p in range(P):
        means = np.array([s[:, p].mean() for s in seqs])
        W = np.mean([np.sum((s[:, p] - s[:, p].mean()) ** 2) / (h - 1) for s in seqs])
        Bv = h / (m - 1) * np.sum((means - means.mean()) ** 2)
        out[p] = np.sqrt(((h - 1) / h * W + Bv / h) / W)
    return out


def test_split_rhat():
    from pssgp.experiments.toy import split_rhat
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 101, 2)) * np.array([1.0, 3.0]) + rng.standard_normal((3, 1, 2))
    assert np.allclose(split_rhat(x), _split_rhat_direct(x), rtol=1e-12, atol=0)
    iid = np.random.default_rng(6).standard_normal((4, 2000, 3))
    assert np.all(np.abs(split_rhat(iid) - 1.0) <= 0.02)
    shifted = iid.copy()
    shifted[1] += 3.0
    assert np.all(split_rhat(shifted) > 1.5)


def test_method_contract():
    from pssgp.kernels import Matern32
    from pssgp.model import StateSpaceGP
    t, y = _series(30, seed=2)
    m = StateSpaceGP((t[:, None], y[:, None]), Matern32(1.0, 0.5), noise_variance=0.1, parallel=False)
    with pytest.raises(NotImplementedError):
        m.log_likelihood_and_grad_batch(SETTINGS)
    m = StateSpaceGP((t[:, None], y[:, None]), Matern32(1.0, 0.5), noise_variance=0.1, parallel=True)
    with pytest.raises(ValueError):
        m.log_likelihood_and_grad_batch(np.ones((4, 2)))
    with pytest.raises(ValueError):
        m.log_likelihood_and_grad_batch(np.ones((4, 4)))
    assert (m.kernel.variance, m.kernel.lengthscales, m.noise_variance) == (1.0, 0.5, 0.1)


def test_parameters_are_restored_when_a_row_raises():
    """A row that fails AFTER rows have been assigned -- inside the preparation of the general path, and inside the loop --
    leaves the model's parameters as they were (the failure is injected: neither path reaches the device before it)."""
    from pssgp.kernels import Matern32, Matern52
    from pssgp.model import StateSpaceGP
    t, y = _series(40, seed=3)
    rng = np.random.default_rng(0)

    def settings(m, B):
        x0 = np.array([getattr(o, a) for o, a in m.trainable_parameters()], np.float64)
        return x0, x0[None, :] * rng.uniform(0.8, 1.25, size=(B, x0.size))

    # the general path: the third row's preparation raises
    m = StateSpaceGP((t[:, None], y[:, None]), Matern32(1.3, 0.7) + Matern52(0.6, 1.1), noise_variance=0.15, parallel=True)
    x0, thetas = settings(m, 4)
    real, calls = m._adjoint_prepared, []

    def failing():
        calls.append([getattr(o, a) for o, a in m.trainable_parameters()])
        if len(calls) == 3:
            raise RuntimeError("third row")
        return real()

    m._adjoint_prepared = failing
    with pytest.raises(RuntimeError, match="third row"):
        m.log_likelihood_and_grad_batch(thetas)
    assert len(calls) == 3 and np.array_equal(calls[2], thetas[2])         # (row 2 WAS assigned when it failed)
    assert np.array_equal([getattr(o, a) for o, a in m.trainable_parameters()], x0)

    # the loop: the second row's gradient raises
    m = StateSpaceGP((t[:, None], y[:, None]), Matern32(1.0, 0.5), noise_variance=0.1, parallel=True)
    m._GRAD_BATCH_FROM = 10 ** 9            # (no batched launches for this model: the loop)
    x0, thetas = settings(m, 3)
    seen = []

    def grad(wrt=None, method=None):
        seen.append([getattr(o, a) for o, a in m.trainable_parameters()])
        if len(seen) == 2:
            raise RuntimeError("second row")
        return 0.0, np.zeros(3)

    m.log_likelihood_and_grad = grad
    with pytest.raises(RuntimeError, match="second row"):
        m.log_likelihood_and_grad_batch(thetas)
    assert len(seen) == 2 and np.array_equal(seen[1], thetas[1])
    assert np.array_equal([getattr(o, a) for o, a in m.trainable_parameters()], x0)
