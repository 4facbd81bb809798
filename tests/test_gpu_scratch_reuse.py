"""One context, one call after the other, each laying the context's scratch out afresh (parallel-gps_amd/csrc/pgps_scratch.h: every
launch function carves its parts from one carver and resolves them against the base the commit hands back): a fused predict_f,
a batched predict_f in three groups, the multi-output adjoint pass in two rounds, the general-LTI adjoint pass, the fused
predict_f again on a series that makes the workspace grow and move, the batch again, and the array-path filter + smoother.
Every result must equal, bit for bit, the same call on a context created fresh for it and set to the same budget: results are
deterministic for a fixed geometry, so a difference means a part was resolved against a stale base, or two parts overlap."""
import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

R = 0.1
N, K, B, M = 700, 90, 5, 5


def _data(n, k, seed):
    rng = np.random.RandomState(seed)
    t = 0.2 + np.sort(rng.rand(n)) * (n / 80.0)
    y = np.sin(3.0 * t) + 0.3 * rng.randn(n)
    y[rng.rand(n) < 0.1] = np.nan
    tq = np.sort(rng.rand(k)) * (n / 80.0) * 1.1
    return t, y, tq


def _fused(cls, v=1.3, l=0.7):
    from pssgp import _backend as Bk
    sde = cls(variance=v, lengthscales=l).get_sde()
    return sde, (Bk.nilpotent_form(sde.F), np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1))


def _predict_batch_scratch_per_model(n_merged, d, batch):
    """Bytes of scratch one model of the batched fused predict takes (launch_gp_predict_batch, fp64, the three-launch form):
    256 lanes per workgroup, steps per lane by the rule of the batched fused launches, every part rounded to 256 bytes."""
    up = lambda x: (x + 255) // 256 * 256                                       # noqa: E731
    lc = 16
    while lc > 4 and batch * -(-n_merged // (256 * lc)) < 1024:
        lc //= 2
    if n_merged < 256 * 4:
        lc = max(1, -(-n_merged // 256))
    nb = -(-n_merged // (256 * lc))
    nl = 256 * nb
    nfilt, nsmth = d * d + 2 * d + d * (d + 1), d * d + d + d * (d + 1) // 2
    return (up(nb * nfilt * 8) + up(nl * nfilt * 8) + up(nb * nsmth * 8) + up(nl * nsmth * 8) + up(nb * 8) + up(n_merged * d * 8)
            + up(n_merged * d * d * 8))


def _steps():
    """[(name, budget, call)]: `call()` runs on whatever context the module-level entry points find."""
    from oracle import np_oracle as O
    from pssgp import _backend as Bk
    from pssgp.kernels import Matern32, Matern52
    t, y, tq = _data(N, K, 1)
    t_long, y_long, _ = _data(6000, K, 2)
    sde52, (form52, P52, H52) = _fused(Matern52)
    sde32, (form32, P32, H32) = _fused(Matern32)
    thetas = np.exp(np.random.RandomState(3).uniform(-1.0, 1.0, (B, 3)))
    models = []
    for v, l, r in thetas:
        _, (f, P, H) = _fused(Matern52, v, l)
        models.append((f, P, H, r))
    per_model = _predict_batch_scratch_per_model(N + K, 3, B)
    batch_budget = 5 * per_model // 2
    assert 2 * per_model <= batch_budget < 3 * per_model and -(-B // 2) == 3     # groups of 2, 2, 1
    rng = np.random.RandomState(4)
    Y = np.sin(3.0 * t)[:, None] * rng.uniform(0.5, 2.0, (1, M)) + 0.3 * rng.randn(N, M)
    Y[np.isnan(y)] = np.nan
    # d = 5: Matern-3/2 + Matern-5/2 as one LTI model
    F5 = sla.block_diag(np.asarray(sde32.F, np.float64), np.asarray(sde52.F, np.float64))
    P5 = sla.block_diag(P32, P52)
    H5 = np.concatenate([H32, H52])
    t5, y5, _ = _data(1500, 1, 5)
    ssm = tuple(np.asarray(a, np.float64) for a in O.get_ssm(sde32, t, R))
    y_arr = np.where(np.isnan(y), 0.0, y)

    def flat(res):
        return [np.asarray(a, np.float64) for a in res]

    predict = lambda: flat(Bk.gp_predict(form52, P52, H52, R, t, y, tq))                        # noqa: E731
    batch = lambda: flat(Bk.gp_predict_batch(models, t, y, tq)[:3])                              # noqa: E731
    return [
        ("a: fused predict_f", 0, predict),
        ("b: predict_f_batch in three groups", batch_budget, batch),
        # d = 2 runs tiles of four columns: two column groups, the second holds one column; 4096 bytes hold no group
        ("c: multi-output ll + grad in two rounds", 4096, lambda: flat(Bk.gp_ll_grad_multi(form32, P32, H32, R, t, Y))),
        ("d: general-LTI ll + grad", 0, lambda: flat(Bk.lti_ll_grad(F5, P5, H5, R, t5, y5))),
        ("e: fused predict_f, longer series", 0, lambda: flat(Bk.gp_predict(form52, P52, H52, R, t_long, y_long, tq))),
        ("f: predict_f_batch again", batch_budget, batch),
        ("g: pkfs on arrays", 0, lambda: flat(Bk.pkfs(ssm, y_arr, return_filtered=True, return_loglikelihood=True))),
    ]


def test_one_context_equals_fresh_contexts():
    from pssgp import _backend as Bk
    steps = _steps()
    default = Bk.get_context()
    reused, fresh = Bk.Context(0), None
    got, bad = [], []
    try:
        Bk._contexts[0] = reused                    # the module-level entry points run on it
        for name, budget, call in steps:
            try:
                reused.set_batch_scratch(budget)
                got.append(call())
            finally:
                reused.set_batch_scratch(0)
            assert reused.status() == 0, name
        for (name, budget, call), res in zip(steps, got):
            fresh = Bk.Context(0)
            Bk._contexts[0] = fresh
            try:
                fresh.set_batch_scratch(budget)
                want = call()
            finally:
                fresh.set_batch_scratch(0)
                Bk._contexts[0] = reused
                fresh.close()
                fresh = None
            assert len(res) == len(want), name
            for i, (a, b) in enumerate(zip(res, want)):
                assert np.all(np.isfinite(b)), (name, i)
                same = a.shape == b.shape and np.array_equal(a, b)
                print(f"{name} output {i}: {'equal' if same else 'DIFFERENT'}")
                if not same:
                    bad.append((name, i, float(np.max(np.abs(a - b))) if a.shape == b.shape else "shape"))
    finally:
        Bk._contexts[0] = default
        reused.set_batch_scratch(0)
        reused.close()
        if fresh is not None:
            fresh.close()
    assert not bad, bad
