"""The joint posterior covariance on the device (pgps_pks_cov_*, pgps_lti_predict_cov_f64) and
StateSpaceGP(parallel=True).predict_f(X, full_cov=True): against dense conditioning of the joint state-space prior, the oracle
smoother and the dense GP (sample_law.py) across the block scan, the spine fold, ragged chunks, tied times, both precisions
and both float32 policies; against the host twin at scale; the model-level call pinned to pks_cov; and the sample
covariance of predict_f_samples' draws against the law.  Errors are conftest.relerr, bounds TOL64 / TOL32."""
import functools

import numpy as np
import pytest

from conftest import relerr
from oracle import np_oracle as O
from sample_law import MODELS, TOL32, TOL64, dense_f_posterior, diag_blocks, joint_state_posterior, law_case, mc_setup, project
from test_cov_host import check_model_full_cov, dense_posterior, full, model_case, selections, sub
from test_gpu_sample_law import GEOMETRIES, MODES, REPEATED, TIES, ctx

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def reference(name, N, ties=()):
    ssm, ts, ys, fms, fPs, spec = law_case(name, N, ties=ties)
    _, sPs = O.kfs(ssm, ys)
    return ssm, ts, ys, fms, fPs, sPs, spec, joint_state_posterior(ssm, ys)


def device_selections(N):
    """test_cov_host's selections, a segment boundary on the workgroup boundary 255 | 256 of one step per lane, and one
    segment that spans all three workgroups"""
    sels = dict(selections(N))
    if N > 512:
        sels["boundary_255_256"] = np.array([100, 255, 256, 300, 511, 512, N - 1])
        sels["span_all"] = np.array([3, N - 3])
    return sels


def pks_cov(ssm, fPs, sPs, sel, mode, chunk=0, H=None):
    from pssgp import _backend
    dtype, policy = MODES[mode]
    c = ctx()
    try:
        c.set_chunk(chunk)
        if policy is not None:
            c.set_f32_policy(policy)
        out = _backend.pks_cov(tuple(np.asarray(a, dtype) for a in ssm), np.asarray(fPs, dtype), np.asarray(sPs, dtype), sel,
                               H=None if H is None else np.asarray(H, dtype).reshape(-1))
    finally:
        c.set_chunk(0)
        c.set_f32_policy(0)
    assert out.dtype == dtype
    return out


def run_cov(name, mode, chunk, N, ties=()):
    ssm, ts, ys, fms, fPs, sPs, spec, want = reference(name, N, ties)
    d = fms.shape[1]
    tol = TOL64 if MODES[mode][0] == np.float64 else TOL32
    label = f"pks_cov {name} {mode} chunk {chunk} N {N}{' ties' if ties else ''}"
    cov = full(pks_cov(ssm, fPs, sPs, np.arange(N), mode, chunk))
    proj = pks_cov(ssm, fPs, sPs, np.arange(N), mode, chunk, H=ssm[3])
    errs = {"joint": relerr(cov, want), "blocks": relerr(diag_blocks(cov, N, d), sPs),
            "projected": relerr(proj, project(want, ssm[3], N, d))}
    if spec is not None:
        errs["dense"] = relerr(proj, dense_f_posterior(spec, ts, ys, 0.1))
    print(f"{label} all steps: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert np.array_equal(cov, cov.T) and np.array_equal(proj, proj.T), label
    for k, v in errs.items():
        assert v < tol, (label, k, v)
    for sname, sel in device_selections(N).items():
        e1 = relerr(full(pks_cov(ssm, fPs, sPs, sel, mode, chunk)), sub(want, sel, d))
        e2 = relerr(pks_cov(ssm, fPs, sPs, sel, mode, chunk, H=ssm[3]), project(sub(want, sel, d), ssm[3], len(sel), d))
        print(f"{label} {sname}: states {e1:.2e} projected {e2:.2e}")
        assert max(e1, e2) < tol, (label, sname, e1, e2)
    return cov


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geometry", ["default_300", "chunk1_553"])
@pytest.mark.parametrize("name", MODELS)
def test_pks_cov(name, geometry, mode):
    """all steps and the selections, with and without H, over one workgroup and over three (ragged last one)"""
    chunk, N = GEOMETRIES[geometry]
    run_cov(name, mode, chunk, N)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["matern_d1", "matern_d2"])
def test_pks_cov_four_steps_per_lane(name, mode):
    chunk, N = GEOMETRIES["chunk4_2053"]
    run_cov(name, mode, chunk, N)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", MODELS)
def test_pks_cov_tied_times(name, mode):
    """a pair, a triple, a pair across the workgroup boundary and a near-tie of 1e-9; rows of exactly tied steps agree"""
    chunk, N = GEOMETRIES["chunk1_553"]
    cov = run_cov(name, mode, chunk, N, ties=TIES)
    ssm, ts, ys, fms, fPs, sPs, spec, want = reference(name, N, TIES)
    d = fms.shape[1]
    tol = TOL64 if MODES[mode][0] == np.float64 else TOL32
    for k in REPEATED:
        assert ts[k + 1] == ts[k]
        gap = float(np.max(np.abs(cov[k * d:(k + 1) * d] - cov[(k + 1) * d:(k + 2) * d])) / np.max(np.abs(cov)))
        print(f"pks_cov tied rows {name} {mode} step {k}: {gap:.2e}")
        assert gap < tol, (name, mode, k, gap)


@pytest.mark.parametrize("name", ["matern_d3", "rbf6"])
def test_pks_cov_float32_promoted(name):
    """pgps_set_f32_policy(2): the float32 call runs in fp64 arithmetic on widened inputs, rounds, and says so"""
    from pssgp import _backend
    chunk, N = GEOMETRIES["chunk1_553"]
    ssm, ts, ys, fms, fPs, sPs, spec, want = reference(name, N, ())
    d = fms.shape[1]
    sel = device_selections(N)["random40"]
    c = ctx()
    c.status()
    try:
        c.set_f32_policy(2)
        args = (tuple(np.asarray(a, np.float32) for a in ssm), fPs.astype(np.float32), sPs.astype(np.float32))
        got = _backend.pks_cov(*args, np.arange(N))
        got_h = _backend.pks_cov(*args, sel, H=np.asarray(ssm[3], np.float32).reshape(-1))
        promoted = c.status() & 4
    finally:
        c.set_f32_policy(0)
    assert got.dtype == np.float32 and got_h.dtype == np.float32 and promoted
    e1, e2 = relerr(full(got), want), relerr(got_h, project(sub(want, sel, d), ssm[3], len(sel), d))
    print(f"pks_cov {name} float32 promoted: joint {e1:.2e} projected selection {e2:.2e}")
    assert np.array_equal(full(got), full(got).T) and max(e1, e2) < TOL32


@pytest.mark.parametrize("name", ["matern_d2", "matern_d5", "rbf6"])
def test_pks_cov_repeats_symmetry_and_geometry(name):
    """one call repeated gives the same bits; the output is symmetric bit for bit; another launch geometry agrees to
    rounding"""
    chunk, N = GEOMETRIES["chunk1_553"]
    ssm, ts, ys, fms, fPs, sPs, spec, want = reference(name, N, ())
    sel = device_selections(N)["random40"]
    for H in (None, ssm[3]):
        for s in (np.arange(N), sel):
            a = pks_cov(ssm, fPs, sPs, s, "f64", chunk, H=H)
            b = pks_cov(ssm, fPs, sPs, s, "f64", chunk, H=H)
            assert np.array_equal(a, b)
            m = a if H is not None else full(a)
            assert np.array_equal(m, m.T)
            e = max(relerr(pks_cov(ssm, fPs, sPs, s, "f64", c2, H=H), a) for c2 in (0, 2, 3))
            print(f"pks_cov {name} {'projected' if H is not None else 'states'} n {len(s)}: other geometries {e:.2e}")
            assert e < TOL64, (name, e)


def test_pks_cov_rejects_bad_arguments():
    from ctypes import c_int, c_long
    from pssgp import _backend
    from pssgp._backend import PgpsError, _ptr
    ssm, ts, ys, fms, fPs, spec = law_case("matern_d2", 50)
    _, sPs = O.kfs(ssm, ys)
    Fs, Qs = np.ascontiguousarray(ssm[1]), np.ascontiguousarray(ssm[2])
    out = np.empty((2, 2, 2, 2))
    c = ctx()

    def call(N, d, n, sel):
        sel = np.asarray(sel, np.int64)
        c.call("pgps_pks_cov_f64", c_long(N), c_int(d), _ptr(Fs), _ptr(Qs), _ptr(fPs), _ptr(sPs), c_long(n), _ptr(sel), None,
               _ptr(out))
    for bad in ([3, 2], [4, 4], [-1, 3], [10, 50]):
        with pytest.raises(PgpsError) as e:
            call(50, 2, 2, bad)
        assert e.value.code == -1, bad
    with pytest.raises(PgpsError) as e:
        call(50, 2, 0, [0])
    assert e.value.code == -1
    with pytest.raises(PgpsError) as e:
        call(50, 8, 2, [0, 1])
    assert e.value.code == -2
    with pytest.raises(ValueError):
        _backend.pks_cov(ssm, fPs, sPs, [5, 5])
    call(50, 2, 2, [7, 30])                                    # (and the context still works)
    one = _backend.pks_cov(ssm, fPs, sPs, [17])
    assert one.shape == (1, 1, 2, 2) and relerr(one[0, 0], sPs[17]) < TOL64


def test_pks_cov_output_too_large_is_an_allocation_error():
    """2^18 selected steps: a (2^18, 2^18) fp64 output is 512 GiB, more than the device has"""
    from ctypes import c_int, c_long
    from pssgp._backend import PgpsError, _ptr
    N = 2 ** 18
    a = np.ones((N, 1, 1))
    sel = np.arange(N, dtype=np.int64)
    out = np.empty(16)
    with pytest.raises(PgpsError) as e:
        ctx().call("pgps_pks_cov_f64", c_long(N), c_int(1), _ptr(a), _ptr(a), _ptr(a), _ptr(a), c_long(N), _ptr(sel), None,
                   _ptr(out))
    assert e.value.code == -4
    ssm, ts, ys, fms, fPs, spec = law_case("matern_d1", 50)
    from pssgp import _backend
    assert _backend.pks_cov(ssm, fPs, O.kfs(ssm, ys)[1], [3, 9]).shape == (2, 2, 1, 1)


@pytest.mark.parametrize("name", ["matern_d2", "matern_d6"])
def test_pks_cov_at_scale_is_the_host_twin(name):
    """2^17 + 3 steps, 2048 selected: 32 row tiles of the fill, hundreds of workgroups of the scan, segments from 1 step to
    hundreds.  The device's own discretisation, filter and smoother give the inputs; the host twin (pinned in
    test_cov_host.py) the reference"""
    from pssgp import _backend
    from pssgp.kalman.sequential import ks_cov
    from sample_law import law_model, law_series
    N, n = 2 ** 17 + 3, 2048
    kern, _ = law_model(name)
    ts, ys = law_series(N)
    sde = kern.get_sde()
    P0, h = np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1)
    Fs, Qs = _backend.discretise(sde.F, P0, ts)
    ssm = (P0, Fs, Qs, h[None, :], np.full((1, 1), 0.1))
    sms, sPs, fms, fPs = _backend.pkfs(ssm, ys, return_filtered=True)
    rng = np.random.default_rng(5)
    sel = np.sort(rng.choice(N, n, replace=False))
    sel = np.union1d(sel, sel[100] + np.arange(4))[:n]          # (four adjacent steps too; n selected steps exactly)
    assert sel.size == n
    got = _backend.pks_cov(ssm, fPs, sPs, sel, H=h)
    want = ks_cov(ssm, fPs, sPs, sel, H=h)
    e1 = relerr(got, want)
    few = sel[::7]                                              # states: 293 selected steps, five row tiles
    got_s = _backend.pks_cov(ssm, fPs, sPs, few)
    e2 = relerr(got_s, ks_cov(ssm, fPs, sPs, few))
    print(f"pks_cov at scale {name}: N {N} n {len(sel)} projected {e1:.2e}; n {len(few)} states {e2:.2e}")
    assert np.array_equal(got, got.T) and np.array_equal(full(got_s), full(got_s).T)
    assert max(e1, e2) < TOL64, (name, e1, e2)


@pytest.mark.parametrize("name", ["matern12", "matern32", "matern52", "rbf6", "periodic2", "m32+m52", "m32*m52"])
def test_lti_predict_cov_is_pks_cov_on_the_merged_series(kernel_zoo, name):
    """merge, qslot, the device's filter + smoother feeding the two passes: against pks_cov fed discretise, pkf, pks on
    the merged series"""
    from pssgp import _backend
    from pssgp.model import _merge_sorted
    _, make, _, _ = next(z for z in kernel_zoo if z[0] == name)
    ts, ys, xq = model_case(700)
    tq = np.unique(xq)
    sde = make().get_sde()
    all_ts, all_ys, flags = _merge_sorted(ts, tq, (ys, np.full(tq.shape, np.nan)), (np.zeros(ts.size, bool), np.ones(tq.shape, bool)))
    P0, h = np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1)
    Fs, Qs = _backend.discretise(sde.F, P0, all_ts)
    ssm = (P0, Fs, Qs, h[None, :], np.full((1, 1), 0.1))
    fms, fPs, ll_want = _backend.pkf(ssm, all_ys, return_loglikelihood=True)
    sms, sPs = _backend.pks(ssm, fms, fPs)
    rows = np.flatnonzero(flags)
    want = _backend.pks_cov(ssm, fPs, sPs, rows, H=h)
    mean, cov, ll = _backend.lti_predict_cov(sde.F, sde.P0, sde.H, 0.1, ts, ys, tq)
    e_c, e_m, e_l = relerr(cov, want), relerr(mean, sms[rows] @ h), abs(ll - float(ll_want)) / abs(float(ll_want))
    print(f"lti_predict_cov pin {name}: covariance {e_c:.2e} mean {e_m:.2e} ll {e_l:.2e}")
    assert np.array_equal(cov, cov.T)
    assert max(e_c, e_m, e_l) < TOL64, (name, e_c, e_m, e_l)


def predict_f_marginals(model, xq):
    """predict_f itself, on the sorted distinct query times (its device paths take sorted queries)"""
    tq, inverse = np.unique(xq, return_inverse=True)
    m, v = model.predict_f(tq[:, None])
    return m[inverse, 0], v[inverse, 0]


@pytest.mark.parametrize("name", ["matern12", "matern32", "matern52", "m32+m52"])
def test_predict_f_full_cov_device(kernel_zoo, name):
    """parallel=True against parallel=False, against predict_f's own marginals and against the dense GP: unsorted Xnew
    holding a training time and a duplicate; the pass's log-likelihood is the objective"""
    from pssgp import _backend
    from pssgp.model import StateSpaceGP
    _, make, spec, _ = next(z for z in kernel_zoo if z[0] == name)
    ts, ys, xq = model_case()
    dev = StateSpaceGP((ts[:, None], ys[:, None]), make(), noise_variance=0.1, parallel=True)
    host = StateSpaceGP((ts[:, None], ys[:, None]), make(), noise_variance=0.1, parallel=False)
    mean, cov = check_model_full_cov(dev, xq, f"device {name}", marginals=predict_f_marginals)
    check_model_full_cov(host, xq, f"host {name} (device marginals)", marginals=predict_f_marginals)
    mean_h, cov_h = host.predict_f(xq[:, None], full_cov=True)
    want_mean, want_cov = dense_posterior(spec, ts, ys, xq, 0.1)
    sde = dev.kernel.get_sde()
    ll = _backend.lti_predict_cov(sde.F, sde.P0, sde.H, 0.1, ts, ys, np.unique(xq))[2]
    errs = {"host mean": relerr(mean, mean_h), "host cov": relerr(cov, cov_h), "dense mean": relerr(mean[:, 0], want_mean),
            "dense cov": relerr(cov[0], want_cov),
            "ll": abs(ll - float(dev.maximum_log_likelihood_objective())) / abs(ll)}
    print(f"predict_f full_cov device {name}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < TOL64, (name, k, v)
    dup = np.flatnonzero(xq == ts[300] + 0.01)
    assert dup.size == 2 and np.array_equal(cov[0][dup[0]], cov[0][dup[1]]) and np.array_equal(cov[0][:, dup[0]], cov[0][:, dup[1]])
    m0, c0 = dev.predict_f(np.zeros((0, 1)), full_cov=True)
    assert m0.shape == (0, 1) and c0.shape == (1, 0, 0)
    a, b = dev.predict_f(np.sort(xq)[:, None]), dev.predict_f(np.sort(xq)[:, None], full_cov=False)
    assert a[1].shape == (xq.size, 1) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_predict_f_full_cov_device_float32_model():
    from pssgp import config
    from pssgp.kernels import Matern32
    from pssgp.model import StateSpaceGP
    ts, ys, xq = model_case()
    want = StateSpaceGP((ts[:, None], ys[:, None]), Matern32(1.0, 0.5), noise_variance=0.1,
                        parallel=True).predict_f(xq[:, None], full_cov=True)
    config.set_default_float(np.float32)
    try:
        model = StateSpaceGP((ts[:, None].astype(np.float32), ys[:, None].astype(np.float32)), Matern32(1.0, 0.5),
                             noise_variance=0.1, parallel=True)
        mean, cov = model.predict_f(xq[:, None].astype(np.float32), full_cov=True)
    finally:
        config.set_default_float(np.float64)
    assert mean.dtype == np.float32 and cov.dtype == np.float32 and cov.shape == (1, xq.size, xq.size)
    e_m, e_c = relerr(mean, want[0]), relerr(cov, want[1])
    print(f"predict_f full_cov device float32 model against fp64: mean {e_m:.2e} covariance {e_c:.2e}")
    assert max(e_m, e_c) < TOL32


def test_draws_have_the_full_cov_law_at_scale():
    """mc_setup("matern32"): 2^16 training points, 16 queries in 4 clusters, 16 384 draws of predict_f_samples.  EVERY entry
    of the sample covariance (136 distinct ones) within 6 standard errors of predict_f(full_cov=True), standard error
    sqrt((c_ii c_jj + c_ij^2) / S) -- the variance of a Gaussian sample covariance, derived, not tuned; 136 entries at 6
    sigma leave a chance of 3e-7 of a false alarm."""
    from pssgp.model import StateSpaceGP
    kern, spec, ell, ts, ys, xq, noise = mc_setup("matern32")
    S = 16384
    m = StateSpaceGP((ts[:, None], ys[:, None]), kern, noise_variance=noise, parallel=True)
    f = np.concatenate([m.predict_f_samples(xq[:, None], num_samples=S // 16, seed=5 + b)[..., 0] for b in range(16)])
    assert f.shape == (S, 16)
    mean, cov = m.predict_f(xq[:, None], full_cov=True)
    c = cov[0]
    got = np.cov(f, rowvar=False, ddof=1)
    se = np.sqrt((np.outer(np.diag(c), np.diag(c)) + c ** 2) / S)
    z = np.abs(got - c) / se
    zm = np.abs(f.mean(axis=0) - mean[:, 0]) / np.sqrt(np.diag(c) / S)
    print(f"draws against the law: worst |sample cov - cov| / se {z.max():.2f} (bound 6), worst mean {zm.max():.2f}; "
          f"far-cluster covariance {np.max(np.abs(c[:4, 4:])):.2e}")
    assert np.all(z <= 6.0), z.max()
    assert np.all(zm <= 6.0), zm.max()


def test_d8_on_the_device_is_unsupported():
    from pssgp.kernels import RBF
    from pssgp.model import StateSpaceGP
    from pssgp._backend import PgpsError
    ts, ys, xq = model_case(200)
    kern = RBF(variance=1., lengthscales=0.5, order=8, balancing_iter=10)
    model = StateSpaceGP((ts[:, None], ys[:, None]), kern, noise_variance=0.1, parallel=True)
    with pytest.raises(PgpsError) as e:
        model.predict_f(xq[:, None], full_cov=True)
    assert e.value.code == -2
