"""GPU tests of the whitening flavour of the multi-column Kalman pass and of the Gram kernels (k_gpm_whiten, k_gram_partial,
k_gram_finalize; csrc/pgps_whiten.hip.h), and of the mean-function evaluations of StateSpaceGP on the fused route.

The series, the chunks and their geometry table are test_gpu_multi_geometries.py's: N = 4696 rows at spacing 0.05, rows 2040..2055
and 4090..4100 missing (a missing run across a workgroup boundary at every chunk), pgps_set_chunk 1, 4 and 16 read back and held
to that file's table, and the library's own choice.  Every checked call follows the same call on other data (_fresh), so nothing
an earlier call left in scratch -- W itself is scratch in a Gram call, and is not zeroed -- can pass for a result.

Reference: the numpy multi-column filter of multi_refs.ss_multi (one covariance, a (d, M) matrix of means, O.get_ssm's Fs, Qs),
here keeping its standardised innovations r / sqrt(S); not the code under test.  Tolerance 1e-9: max norm relative to the largest
entry for W, |G_ij - ref| / sqrt(G_ii G_jj) for a Gram matrix.  Kernels: variance 1, lengthscale 0.5; R = 0.1."""
import functools
import math

import numpy as np
import pytest

from het_refs import R, matern, queries, sde_of
from multi_refs import multi_series
from oracle import np_oracle as O
from test_gpu_multi_geometries import (FE, KNAMES, LANES, MISSING, N, SPACING, TILE, _align256, _BatchScratch, _bits, _case,
                                       _Chunk, _CountReduce, _form, _fresh, _geometry)
from tests.conftest import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-9
CHUNKS = [1, 4, 16, 0]
SLAB = 1024                     # kGramSlab: rows of W per workgroup of k_gram_partial (tiles of 128 rows)
LOG2PI = math.log(2.0 * math.pi)


def _np_whiten(sde, t, Y):
    """(W (n, M), logdet, n_obs): ss_multi's forward loop, keeping r / sqrt(S); 0.0 at the rows that are not observed."""
    t, Y = np.asarray(t, np.float64).reshape(-1), np.asarray(Y, np.float64)
    seen = ~np.isnan(Y[:, 0])
    P0, Fs, Qs, H, _ = O.get_ssm(sde, t, R)
    h = H.reshape(-1)
    m, P = np.zeros((h.size, Y.shape[1])), P0.copy()
    W, logdet = np.zeros(Y.shape), 0.0
    for k in range(t.size):
        m = Fs[k] @ m
        P = Fs[k] @ P @ Fs[k].T + Qs[k]
        P = 0.5 * (P + P.T)
        if seen[k]:
            S = float(h @ P @ h) + R
            r = Y[k] - h @ m
            W[k] = r / math.sqrt(S)
            logdet += math.log(S)
            u = P @ h
            m = m + np.outer(u, r / S)
            P = P - np.outer(u, u) / S
            P = 0.5 * (P + P.T)
    return W, logdet, int(seen.sum())


@functools.lru_cache(maxsize=None)
def _ref(kname, m, n=N):
    """The reference (W, logdet, n_obs) on the first n rows of the m-column case: computed once, read-only."""
    t, Y, _ = _case(m)
    W, logdet, n_obs = _np_whiten(sde_of(kname), t[:n], Y[:n])
    W.setflags(write=False)
    return W, logdet, n_obs


def _gram_err(G, G_ref):
    dg = np.sqrt(np.diag(G_ref))
    return float(np.max(np.abs(G - G_ref) / np.outer(dg, dg)))


def _whiten_budget(kname, nb):
    """launch_gp_whiten without a Gram matrix: ldpart (2 x nb) is shared; a group holds its spine and its lane prefixes.  The
    budget that holds exactly two of the three column groups (test_gpu_multi_geometries._two_group_budget)."""
    group = nb * FE[kname] + LANES * nb * FE[kname]
    return _align256(8 * 2 * nb) + (5 * 8 * group) // 2


# ---- 1. the whitened columns at every geometry, and in rounds -----------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_whiten_against_the_reference(kname, chunk):
    """M = 2 x tile + 1 = 17 / 9 / 5 columns: three column groups, the last one holding one column (M odd: scalar stores).
    Then once more under a budget that holds two groups: rounds of two and one with their own c_base -- same bits."""
    from pssgp import _backend as Bk
    m = 2 * TILE[kname] + 1
    form, P, H = _form(kname)
    t, Y, _ = _case(m)
    W_ref, logdet_ref, n_ref = _ref(kname, m)
    nb = _geometry(chunk, N)[1] if chunk else None
    W, logdet, n_obs = _fresh(Bk.gp_whiten_multi, form, P, H, t, Y, chunk=chunk)
    ll = _fresh(Bk.gp_ll_multi, form, P, H, t, Y, chunk=chunk)
    assert W.shape == (N, m) and np.all(np.isfinite(W))
    e = relerr(W, W_ref)
    implied = -2.0 * ll - n_obs * LOG2PI - np.sum(W * W, axis=0)             # logdet from every column's log-likelihood
    print(f"{kname} M {m} chunk {chunk}: W {e:.2e} logdet {logdet!r} reference {logdet_ref!r} implied by gp_ll_multi "
          f"{implied.min()!r} .. {implied.max()!r}")
    assert e <= TOL
    missing = np.isnan(Y[:, 0])
    assert np.all(_bits(W[missing]) == 0), "a row that is not observed must hold exact zeros"
    assert n_obs == n_ref == int((~missing).sum())
    np.testing.assert_allclose(implied, logdet, rtol=1e-11, atol=0.0)
    assert abs(logdet - logdet_ref) <= TOL * abs(logdet_ref)
    if chunk:
        two = _whiten_budget(kname, nb)
        with _CountReduce() as count:
            Bk.gp_whiten_multi(form, P, H, R, t, 1.0 - Y)                   # (as _fresh, outside the count)
            count.launches()
            with _Chunk(chunk), _BatchScratch(two):
                W2, logdet2, n2 = Bk.gp_whiten_multi(form, P, H, R, t, Y)
            rounds = count.launches()
        print(f"{kname} M {m} chunk {chunk}: two-group budget {two} bytes, {rounds} k_gpm_reduce launches")
        assert rounds == 2
        assert np.array_equal(_bits(W), _bits(W2)) and _bits(logdet) == _bits(logdet2) and n2 == n_obs, "W depends on the rounds"


@pytest.mark.parametrize("kname", KNAMES)
def test_whiten_vector_stores(kname):
    """M = 2 x tile + 2 is even: the two full groups take the 16-byte loads of V and stores of W, the last group (two columns)
    the scalar ones; a column does not depend on what the other groups hold."""
    from pssgp import _backend as Bk
    m, full = 2 * TILE[kname] + 2, 2 * TILE[kname]
    form, P, H = _form(kname)
    t, Y, _ = _case(m)
    W, logdet, n_obs = _fresh(Bk.gp_whiten_multi, form, P, H, t, Y, chunk=4)
    part = _fresh(Bk.gp_whiten_multi, form, P, H, t, np.ascontiguousarray(Y[:, :full]), chunk=4)
    assert relerr(W, _ref(kname, m)[0]) <= TOL
    assert np.array_equal(_bits(W[:, :full]), _bits(part[0])) and _bits(logdet) == _bits(part[1]) and n_obs == part[2]


# ---- 2. the Gram matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("m", [1, 5, 16])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_gram_against_the_reference(kname, m, chunk):
    """1, 5 and 16 columns (one block of G, two with the second partial, all ten); 4696 rows are four whole slabs of 1024 rows and
    a last one of 600 = four tiles of 128 rows and one of 88."""
    from pssgp import _backend as Bk
    form, P, H = _form(kname)
    t, Y, _ = _case(m)
    W_ref, logdet_ref, n_ref = _ref(kname, m)
    if chunk:
        _geometry(chunk, N)
    G, logdet, n_obs = _fresh(Bk.gp_gram_multi, form, P, H, t, Y, chunk=chunk)
    again = _fresh(Bk.gp_gram_multi, form, P, H, t, Y, chunk=chunk)
    with _Chunk(chunk):
        twice = [Bk.gp_gram_multi(form, P, H, R, t, Y) for _ in range(2)]
    e = _gram_err(G, W_ref.T @ W_ref)
    print(f"{kname} M {m} chunk {chunk}: G {e:.2e} logdet {logdet!r} against {logdet_ref!r}")
    assert G.shape == (m, m) and np.all(np.isfinite(G)) and e <= TOL
    assert np.array_equal(_bits(G), _bits(G.T)), "G is not symmetric bit for bit"
    for other in [again] + twice:
        assert np.array_equal(_bits(G), _bits(other[0])) and _bits(logdet) == _bits(other[1]) and n_obs == other[2], "two calls differ"
    assert n_obs == n_ref and abs(logdet - logdet_ref) <= TOL * abs(logdet_ref)
    Wd, logdet_w, _ = _fresh(Bk.gp_whiten_multi, form, P, H, t, Y, chunk=chunk)
    assert _bits(logdet_w) == _bits(logdet)
    assert _gram_err(G, Wd.T @ Wd) <= 1e-12                              # the device's own W, summed in another order


@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("n", [257, 1189])
def test_gram_ragged_slabs(kname, n):
    """Row counts that end inside a slab and inside a tile: 257 = two tiles of 128 rows and one row (and one step in the second
    workgroup of the scan at one step per lane); 1189 = a whole slab of 1024 rows, then a slab of one whole tile and 37 rows --
    neither a multiple of the slab (1024) nor of 256."""
    from pssgp import _backend as Bk
    assert n % SLAB and n % 256
    m = 16
    form, P, H = _form(kname)
    t, Y, _ = _case(m)
    t, Y = t[:n], np.ascontiguousarray(Y[:n])
    W_ref = _ref(kname, m, n)[0]
    for chunk in (1, 0):
        G, logdet, n_obs = _fresh(Bk.gp_gram_multi, form, P, H, t, Y, chunk=chunk)
        e = _gram_err(G, W_ref.T @ W_ref)
        print(f"{kname} N {n} chunk {chunk}: G {e:.2e}")
        assert e <= TOL and np.array_equal(_bits(G), _bits(G.T)) and n_obs == _ref(kname, m, n)[2]


def test_gram_refuses_more_than_16_columns():
    from pssgp import _backend as Bk
    form, P, H = _form("m32")
    t, Y, _ = _case(17)
    with pytest.raises(Bk.PgpsError) as err:
        Bk.gp_gram_multi(form, P, H, R, t, Y)
    assert err.value.code == -1                                         # PGPS_E_INVALID
    mixed = np.array(_case(5)[1])
    mixed[7, 2] = np.nan
    for call in (Bk.gp_gram_multi, Bk.gp_whiten_multi):
        with pytest.raises(Bk.PgpsError):
            call(form, P, H, R, t, mixed)                               # a row observed in some columns only


@pytest.mark.parametrize("kname", KNAMES)
def test_ll_multi_keeps_its_bits(kname):
    """The unflavoured Kalman pass is untouched by the whitening flavour: pgps_gp_ll_multi_f64 before and after whitening and Gram
    calls on other data returns the bits recorded at the start."""
    from pssgp import _backend as Bk
    m = 2 * TILE[kname] + 1
    form, P, H = _form(kname)
    t, Y, _ = _case(m)
    recorded = Bk.gp_ll_multi(form, P, H, R, t, Y)
    Bk.gp_whiten_multi(form, P, H, R, t, 1.0 - Y)
    after_whiten = Bk.gp_ll_multi(form, P, H, R, t, Y)
    Bk.gp_gram_multi(form, P, H, R, t, np.ascontiguousarray(1.0 - Y[:, :5]))
    after_gram = Bk.gp_ll_multi(form, P, H, R, t, Y)
    assert np.array_equal(_bits(recorded), _bits(after_whiten)) and np.array_equal(_bits(recorded), _bits(after_gram))


# ---- 3. the model ----------------------------------------------------------------------------------------------------------
def _fourier(p, lo, hi):
    """p basis functions on [lo, hi]: 1, then sin / cos pairs of whole periods.  They are orthogonal on the interval and a
    stationary kernel's K_y^-1 is nearly diagonal in them, so A = Phi^T K_y^-1 Phi is well conditioned: the coefficients carry
    cond(A) times the rounding of G, and the 1e-9 of these tests is a statement about G only while cond(A) stays small
    (asserted below 1e6, as in test_mean_function_host.py)."""
    def fn(t):
        u = (t - lo) / (hi - lo)
        cols = [np.ones_like(u)]
        for j in range(1, p):
            w = 2.0 * math.pi * ((j + 1) // 2)
            cols.append(np.sin(w * u) if j % 2 else np.cos(w * u))
        return np.stack(cols, axis=1)
    return fn


@functools.lru_cache(maxsize=None)
def _trend_series():
    t, Y = multi_series(N, 1, SPACING, extra_missing=MISSING)
    u = (t - t[0]) / (t[-1] - t[0])
    y = Y[:, 0] + 3.0 + 2.0 * u - 1.5 * u * u
    tq = queries(t, 50)
    for a in (t, y, tq):
        a.setflags(write=False)
    return t, y, tq


def _mean_function(name, t):
    from pssgp.mean_functions import Basis, Polynomial
    if name == "poly2":
        return Polynomial(2, center=0.5 * (t[0] + t[-1]), scale=0.5 * (t[-1] - t[0]))
    p = int(name[1:])
    return Basis(_fourier(p, t[0], t[-1]), p)


def _models(kname, name):
    from pssgp.model import StateSpaceGP
    t, y, tq = _trend_series()
    out = []
    for parallel in (True, False):
        mf = _mean_function(name, t)
        mf.beta = 0.1 * np.cos(np.arange(mf.beta.shape[0]))
        out.append(StateSpaceGP((t[:, None], y[:, None]), matern(kname), noise_variance=R, parallel=parallel, mean_function=mf))
    return out + [tq]


@pytest.mark.parametrize("kname", ["m32", "m52"])
@pytest.mark.parametrize("name", ["poly2", "p15"])
def test_model_against_its_host_twin(kname, name, monkeypatch):
    """parallel=True (one covariance pass and one Gram pass on the device, 1 + p = 3 and 16 columns; predict_f_gls through
    gp_predict_multi) against the parallel=False model (the sequential filter's innovations, the column loop) at 1e-9."""
    from pssgp import _backend as Bk
    dev, host, tq = _models(kname, name)
    calls = []
    real = Bk.gp_gram_multi
    monkeypatch.setattr(Bk, "gp_gram_multi", lambda *a, **k: calls.append(1) or real(*a, **k))
    g, gh = dev.mean_gram(), host.mean_gram()
    assert calls == [1], "the fused route was not taken"
    e = _gram_err(g.G, gh.G)
    print(f"{kname} {name}: G {e:.2e} logdet {g.logdet!r} against {gh.logdet!r}")
    assert e <= TOL and g.n_obs == gh.n_obs and abs(g.logdet - gh.logdet) <= TOL * abs(gh.logdet)
    assert np.array_equal(_bits(g.G), _bits(g.G.T))
    (b, cov, prof), (bh, covh, profh) = dev.mean_coefficients(), host.mean_coefficients()
    assert np.linalg.cond(gh.A) < 1e6
    print(f"{kname} {name}: cond(A) {np.linalg.cond(gh.A):.1e} beta {relerr(b, bh):.2e} cov {relerr(cov, covh):.2e}")
    assert relerr(b, bh) <= TOL and relerr(cov, covh) <= TOL and abs(prof - profh) <= TOL * abs(profh)
    fd, fh = dev.log_marginal_likelihood_flat_mean(), host.log_marginal_likelihood_flat_mean()
    assert abs(fd - fh) <= TOL * abs(fh)
    (mean, var), (mean_h, var_h) = dev.predict_f_gls(tq[:, None]), host.predict_f_gls(tq[:, None])
    assert mean.shape == var.shape == (50, 1)
    print(f"{kname} {name}: predict_f_gls mean {relerr(mean, mean_h):.2e} var {relerr(var, var_h):.2e}")
    assert relerr(mean, mean_h) <= TOL and relerr(var, var_h) <= TOL
    # the gradient: the kernel's entries are the zero-mean model's on the residuals (the same arithmetic), the beta entries the
    # host twin's b - A beta
    p = dev.mean_function.beta.shape[0]
    ll, grad = dev.log_likelihood_and_grad()
    n0 = grad.shape[0] - p
    ll_h, grad_h = host.log_likelihood_and_grad(wrt=range(n0, n0 + p))
    t, y, _ = _trend_series()
    zero = type(dev)((t[:, None], (y - dev.mean_function(t))[:, None]), dev.kernel, noise_variance=R, parallel=True)
    ll_r, grad_r = zero.log_likelihood_and_grad()                       # (its first evaluation, as the residual model's above)
    assert _bits(ll) == _bits(ll_r) and np.array_equal(_bits(grad[:n0]), _bits(grad_r))
    print(f"{kname} {name}: ll {ll!r} against {ll_h!r}, d ll / d beta {relerr(grad[n0:], grad_h[n0:]):.2e}")
    assert abs(ll - ll_h) <= TOL * abs(ll_h) and relerr(grad[n0:], grad_h[n0:]) <= TOL
    _, only = dev.log_likelihood_and_grad(wrt=[0, n0 + 1])
    assert relerr(only[[0, n0 + 1]], grad[[0, n0 + 1]]) <= TOL and _bits(only[n0 + 1]) == _bits(grad[n0 + 1])
    assert np.count_nonzero(only) == 2
    # whiten on the fused route: W^T W is the Gram matrix
    W = dev.whiten(np.concatenate([_trend_series()[1][:, None], dev.mean_function.design(_trend_series()[0])], axis=1))
    assert _gram_err(W.T @ W, g.G) <= 1e-12 and np.all(_bits(W[np.isnan(_trend_series()[1])]) == 0)


def test_seventeen_columns_take_the_host_twin(monkeypatch):
    """1 + p = 17 exceeds the Gram kernel's 16 columns: mean_gram() of the parallel=True model is the host twin's, and agrees."""
    from pssgp import _backend as Bk
    dev, host, _ = _models("m32", "p16")

    def refuse(*a, **k):
        raise AssertionError("17 columns reached the device's Gram entry point")
    monkeypatch.setattr(Bk, "gp_gram_multi", refuse)
    g, gh = dev.mean_gram(), host.mean_gram()
    assert g.G.shape == (17, 17) and _gram_err(g.G, gh.G) <= TOL and g.n_obs == gh.n_obs
    assert relerr(dev.mean_coefficients()[0], host.mean_coefficients()[0]) <= TOL


def test_other_kernels_take_the_host_twin():
    """parallel=True on an RBF kernel: no fused route, so mean_gram() and whiten() are the host twin's (correct for any kernel),
    and the delegated evaluations are the zero-mean model's on the residuals."""
    from pssgp.kernels import RBF
    from pssgp.mean_functions import Linear
    from pssgp.model import StateSpaceGP
    t, y, tq = _trend_series()
    t, y = t[:300], y[:300]
    got = []
    for parallel in (True, False):
        mf = Linear()
        mf.beta = [1.0, 0.02]
        model = StateSpaceGP((t[:, None], y[:, None]), RBF(variance=1., lengthscales=0.5, order=4, balancing_iter=5), noise_variance=R,
                             parallel=parallel, mean_function=mf)
        got.append(model)
    dev, host = got
    assert dev._fused_route() is None
    g, gh = dev.mean_gram(), host.mean_gram()
    assert _gram_err(g.G, gh.G) <= TOL
    ll_whitened = -0.5 * (g.n_obs * LOG2PI + g.logdet + float(np.sum(dev.whiten(y - dev.mean_function(t)) ** 2)))
    ll = float(dev.maximum_log_likelihood_objective())
    ll_host = float(host.maximum_log_likelihood_objective())
    print(f"RBF: ll {ll!r} from the whitened residuals {ll_whitened!r} sequential {ll_host!r}")
    assert abs(ll - ll_whitened) <= TOL * abs(ll) and abs(ll - ll_host) <= TOL * abs(ll)
    zero = StateSpaceGP((t[:, None], (y - dev.mean_function(t))[:, None]), dev.kernel, noise_variance=R, parallel=True)
    assert _bits(zero.maximum_log_likelihood_objective()) == _bits(dev._residual_model().maximum_log_likelihood_objective())
    mean, var = dev.predict_f(tq[:20, None])                            # (the second evaluation of both zero-mean models)
    mean_z, var_z = zero.predict_f(tq[:20, None])
    assert np.array_equal(_bits(mean), _bits(mean_z + dev.mean_function(tq[:20])[:, None])) and np.array_equal(_bits(var), _bits(var_z))
