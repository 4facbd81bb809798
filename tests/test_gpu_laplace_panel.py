"""GPU tests of Laplace inference on a panel (pgps_gp_panel_laplace_*, LaplaceStateSpaceGPPanel(parallel=True); DESIGN.md
section 4ab): the mode search of every series inside one launch.  ctypes -> C ABI.  References (laplace_panel_refs.py; none is
the code under test): the single-series device route and the host twin at 1e-8 -- the move at which the searches stop, the
figure tests/test_gpu_laplace.py holds the device route to against its twin -- and the dense Laplace approximation of Rasmussen
& Williams at the Matern tolerance against the dense GP (1e-6).  Counts: halvings equal the host twin's; iterations equal it,
except where the twin's own move sequence has an entry within [tol / 2, 2 tol] (then +- 1).  Panels: the lengths of
test_gpu_panel.py (a one-row series, one lane, a full wave, 256 / 257 across the step-per-lane boundary, a ragged last wave),
every series with observations of its own seed; 2047 / 2048 rows (eight steps per lane, LDS-staged) in one test."""
import ctypes
import warnings

import numpy as np
import pytest

import laplace_panel_refs as PR
import laplace_refs as LR
from laplace_panel_refs import KNAMES, LENGTHS, LIKELIHOODS, MATERNS, PARS, TOL_SEARCH, err, likelihood, matern

pytestmark = pytest.mark.gpu

ROWS = ("f", "v", "zs", "ss")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _model(kname, variance=1.0, ell=0.5):
    """One entry of a panel call's model list: (form, Pinf, H, R)."""
    from pssgp import _backend as Bk
    from pssgp import kernels as Kn
    sde = getattr(Kn, MATERNS[kname][0])(variance=variance, lengthscales=ell).get_sde()
    return (Bk.nilpotent_form(sde.F), np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1), 0.0)


def _concat(cases):
    offs = np.concatenate([[0], np.cumsum([t.size for t, _ in cases])])
    return offs, np.concatenate([t for t, _ in cases]), np.concatenate([y for _, y in cases])


def _call(kname, lik, cases, pars=None, models=None, **kw):
    from pssgp import _backend as Bk
    offs, ts, ys = _concat(cases)
    out = Bk.gp_panel_laplace([_model(kname)] if models is None else models, LR.LIKS[lik], [PARS[lik]] if pars is None else pars,
                              offs, ts, ys, **kw)
    return offs, out


def _single(kname, lik, t, y, par=None, **kw):
    from pssgp.laplace import LaplaceStateSpaceGP
    return LaplaceStateSpaceGP((t[:, None], y[:, None]), matern(kname), likelihood(lik, par), parallel=True, **kw)


def _info(row):
    return {"iterations": int(row[3]), "halvings": int(row[4]), "converged": bool(row[5])}


class _Ctx:
    """pgps_set_chunk / pgps_set_batch_scratch for the block, restored on every exit."""

    def __init__(self, chunk=0, scratch=0):
        from pssgp import _backend as Bk
        self.ctx, self.chunk, self.scratch = Bk.get_context(), chunk, scratch

    def __enter__(self):
        self.ctx.set_chunk(self.chunk)
        self.ctx.set_batch_scratch(self.scratch)

    def __exit__(self, *exc):
        self.ctx.set_chunk(0)
        self.ctx.set_batch_scratch(0)


@pytest.mark.parametrize("lik", LIKELIHOODS)
@pytest.mark.parametrize("kname", KNAMES)
def test_against_the_references_and_the_single_series_route(kname, lik):
    cases = PR.panel(lik)
    offs, got = _call(kname, lik, cases)
    assert np.all(got["info"][:, 5] == 1.0), got["info"]
    for i, (t, y) in enumerate(cases):
        a, b = offs[i], offs[i + 1]
        nan = np.isnan(y)
        one = _single(kname, lik, t, y)
        fit = one.fit_mode()
        ev = got["info"][i, 0] + got["info"][i, 1] + LR.lik_constant(lik, y)
        e = [err(got["f"][a:b], fit["f"]), err(got["v"][a:b], fit["v"]), err(got["zs"][a:b], fit["z"]), err(got["ss"][a:b], fit["s"]),
             abs(ev - fit["log_evidence"]) / max(1.0, abs(fit["log_evidence"]))]
        ref = PR.dense(kname, lik, i)
        ed = [LR.rel(got["f"][a:b], ref["f_all"]), LR.rel(got["v"][a:b], ref["v_all"]),
              LR.rel(got["zs"][a:b][~nan], ref["z"]), LR.rel(got["ss"][a:b][~nan], ref["s"]),
              abs(ev - ref["evidence"]) / max(1.0, abs(ref["evidence"]))]
        _, twin_info, twin_moves = PR.twin(kname, lik, i)
        info = _info(got["info"][i])
        print(f"{kname} {lik} n {t.size}: single " + " ".join(f"{x:.1e}" for x in e) + " dense " + " ".join(f"{x:.1e}" for x in ed)
              + f" | {info} twin {twin_info['iterations']}/{twin_info['halvings']} single {one.fit_info['iterations']}/{one.fit_info['halvings']}")
        assert max(e) <= TOL_SEARCH, (i, e)
        assert max(ed) <= MATERNS[kname][2], (i, ed)
        assert PR.counts_agree(info, twin_info, twin_moves), (i, info, twin_info, twin_moves)
        assert np.array_equal(np.isnan(got["zs"][a:b]), nan) and np.all(got["ss"][a:b][nan] == 1.0)
        assert got["info"][i, 7] == float((~nan).sum())
        if lik == "poisson" and t.size > 2:
            assert info["halvings"] >= 1            # (the damped branch runs without special data)


@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_one_full_workgroup_and_the_limit(lik):
    from pssgp import _backend as Bk
    from pssgp.laplace_panel import LaplaceStateSpaceGPPanel
    kname = "m32"
    t9, y9 = PR.panel(lik, (2049,))[0]
    cases = PR.panel(lik, (2048, 2047))
    offs, got = _call(kname, lik, cases)
    assert np.all(got["info"][:, 5] == 1.0)
    for i, (t, y) in enumerate(cases):
        fit = _single(kname, lik, t, y).fit_mode()
        a, b = offs[i], offs[i + 1]
        e = [err(got["f"][a:b], fit["f"]), err(got["v"][a:b], fit["v"]), err(got["zs"][a:b], fit["z"]), err(got["ss"][a:b], fit["s"])]
        print(f"{lik} n {t.size}: " + " ".join(f"{x:.1e}" for x in e))
        assert max(e) <= TOL_SEARCH
    # one row more: refused at the ABI with the outputs untouched, spliced by the class
    ctx = Bk.get_context()
    table, d = Bk._gp_rows([_model(kname)])
    o2 = np.array([0, 2049], np.int64)
    f = np.full(2049, np.nan)
    info = np.full(8, np.nan)
    par = np.array([PARS[lik]])
    rc = ctx.lib.pgps_gp_panel_laplace_f64(ctx.handle, 1, Bk._ptr(o2), d, 1, Bk._ptr(table), LR.LIKS[lik], 1, Bk._ptr(par), Bk._ptr(t9),
                                           Bk._ptr(y9), 1e-8, 50, Bk._ptr(f), Bk._ptr(f), Bk._ptr(f), Bk._ptr(f), Bk._ptr(info))
    assert rc == -1 and np.all(np.isnan(f)) and np.all(np.isnan(info))
    short = PR.panel(lik)[3]
    p = LaplaceStateSpaceGPPanel([(t9, y9), short], matern(kname), likelihood(lik))
    assert p._long == [0] and p._short == [1]
    ev = p.log_evidences()
    for s, (t, y) in enumerate([(t9, y9), short]):
        want = float(_single(kname, lik, t, y).maximum_log_likelihood_objective())
        assert abs(ev[s] - want) <= TOL_SEARCH * max(1.0, abs(want))
    # pinned chunks on the 700-row series: unstaged (1, 3), staged full waves next to an unstaged ragged one (4), one lane
    # group of the workgroup only (8)
    t7, y7 = PR.panel(lik)[2]
    fit = _single(kname, lik, t7, y7).fit_mode()
    for chunk in (1, 3, 4, 8):
        with _Ctx(chunk=chunk):
            _, g = _call(kname, lik, [(t7, y7)])
        e = [err(g["f"], fit["f"]), err(g["v"], fit["v"]), err(g["zs"], fit["z"]), err(g["ss"], fit["s"])]
        print(f"{lik} chunk {chunk}: " + " ".join(f"{x:.1e}" for x in e))
        assert max(e) <= TOL_SEARCH and g["info"][0, 5] == 1.0


class _CountLaunches:
    """The context's launch counters; .launches() reads and resets: {slot name: launches}.  The search kernel and the
    gradient's input kernel go out on the slot of PGPS_K_SMOOTHER_APPLY (3), the adjoint passes on PGPS_K_FILTER_APPLY (1)."""

    def __init__(self):
        from pssgp import _backend as Bk
        self.ctx = Bk.get_context()
        self.search, self.adjoint = (self.ctx.lib.pgps_kernel_name(i).decode() for i in (3, 1))

    def __enter__(self):
        self.ctx.profile_enable((1 << 3) | (1 << 1))
        self.ctx.profile_read(reset=True)
        return self

    def launches(self):
        got = self.ctx.profile_read(reset=True)
        return int(got[self.search][1]), int(got[self.adjoint][1])

    def __exit__(self, *exc):
        self.ctx.profile_enable(0)
        self.ctx.profile_read(reset=True)


# budgets under which the panel of LENGTHS falls into groups of uneven size (its search needs 254, 512 and 891 KiB at d = 1, 2, 3;
# one series needs at most 60, 116 and 206 KiB)
UNEVEN = {"m12": 128 << 10, "m32": 300 << 10, "m52": 450 << 10}


@pytest.mark.parametrize("lik", LIKELIHOODS)
@pytest.mark.parametrize("kname", KNAMES)
def test_a_row_depends_on_nothing_but_its_series(kname, lik):
    from pssgp import _backend as Bk
    cases = PR.panel(lik)
    S = len(cases)
    pars = list(np.linspace(0.6, 2.4, S))                   # (one parameter per series: the exposures; Bernoulli reads none)

    def both(cs, ps):
        """The search and, from its modes, the gradient rows: (offs, search dict, gradient rows)."""
        o, out = _call(kname, lik, cs, pars=ps)
        _, ts, ys = _concat(cs)
        rows = Bk.gp_panel_laplace_grad([_model(kname)], LR.LIKS[lik], ps, o, ts, ys, out["f"], out["v"], out["zs"], out["ss"])
        return o, out, rows

    offs, base, base_rows = both(cases, pars)

    def same(got, order, what):
        o, out, rows = got
        for j, i in enumerate(order):
            for k in ROWS:
                assert np.array_equal(_bits(out[k][o[j]:o[j + 1]]), _bits(base[k][offs[i]:offs[i + 1]])), (what, k, i)
            assert np.array_equal(_bits(out["info"][j]), _bits(base["info"][i])), (what, "info", i)
            assert np.array_equal(_bits(rows[j]), _bits(base_rows[i])), (what, "gradient row", i)

    if lik == "poisson":                                    # (the exposures reach the results: a wrong row of pars would show)
        _, shared, _ = both(cases, [pars[0]])
        assert all(not np.array_equal(_bits(shared["info"][i]), _bits(base["info"][i])) for i in range(1, S))
    same(both(cases, pars), range(S), "repeated")
    perm = [2, 6, 0, 5, 3, 1, 4]                            # the 256-row series last: its look-ahead row lies past the allocation
    same(both([cases[i] for i in perm], [pars[i] for i in perm]), perm, "permuted")
    # a budget of one byte: no second series ever fits, every series is a group of its own -- S launches of the search, S of
    # the gradient's inputs and 3 S adjoint passes; and a budget that holds a few of the series: groups of uneven size
    with _Ctx(scratch=1), _CountLaunches() as count:
        got = both(cases, pars)
        n = count.launches()
    assert n == (2 * S, 3 * S), n
    same(got, range(S), "one series per group")
    with _Ctx(scratch=UNEVEN[kname]), _CountLaunches() as count:
        o, out = _call(kname, lik, cases, pars=pars)
        n_search = count.launches()[0]
        got = both(cases, pars)
        n = count.launches()
    print(f"{kname} {lik}: {n_search} launches of the search, {n[1] // 3} groups of the gradient under {UNEVEN[kname] >> 10} KiB")
    assert 1 < n_search < S and n[1] % 3 == 0 and n[1] > 3, (n_search, n)
    same(got, range(S), "a few series per group")
    # a neighbour's rows changed to large values move nothing
    loud = list(cases)
    t3, y3 = cases[3]
    y_big = np.where(np.isnan(y3), np.nan, 1.0 if lik == "bernoulli" else 1e3)
    loud[3] = (t3 + 1e3, y_big)
    o, out, rows = both(loud, pars)
    for i in [i for i in range(S) if i != 3]:
        for k in ROWS:
            assert np.array_equal(_bits(out[k][o[i]:o[i + 1]]), _bits(base[k][offs[i]:offs[i + 1]])), (k, i)
        assert np.array_equal(_bits(out["info"][i]), _bits(base["info"][i])) and np.array_equal(_bits(rows[i]), _bits(base_rows[i]))


def _damped_case():
    rng = np.random.default_rng(1)                  # (the case of test_damping_on_the_device: undamped Newton overflows)
    t = np.sort(rng.uniform(0.0, 10.0, 200))
    K = LR.matern_K("m32", 9.0, 1.0, t, t)
    y = rng.poisson(np.exp(np.linalg.cholesky(K + 1e-10 * np.eye(200)) @ rng.standard_normal(200))).astype(float)
    return t, y, K


def test_damping_inside_the_kernel():
    """The count series of test_damping_on_the_device (variance 9, exposure 1) between gentle ones: it alone halves beyond
    step 1 (the others take their one halving at step 1), and its mode and evidence are the dense search's."""
    from pssgp import _backend as Bk
    t, y, K = _damped_case()
    assert LR.dense_laplace(K, y, "poisson", 1.0, damp=False)["diverged"]
    ref = LR.dense_laplace(K, y, "poisson", 1.0)
    gentle = PR.panel("poisson")
    cases = [gentle[3], (t, y), gentle[4]]
    models = [_model("m32"), _model("m32", 9.0, 1.0), _model("m32")]
    offs, got = _call("m32", "poisson", cases, pars=[PARS["poisson"], 1.0, PARS["poisson"]], models=models)
    print(got["info"], ref["iterations"], ref["halvings"])
    assert np.all(got["info"][:, 5] == 1.0)
    assert got["info"][1, 4] == ref["halvings"] and got["info"][1, 4] > 1 and got["info"][0, 4] == 1 and got["info"][2, 4] == 1
    a, b = offs[1], offs[2]
    assert LR.rel(got["f"][a:b], ref["f"]) <= MATERNS["m32"][2]
    ev = got["info"][1, 0] + got["info"][1, 1] + LR.lik_constant("poisson", y)
    assert abs(ev - ref["evidence"]) <= MATERNS["m32"][2] * abs(ref["evidence"])


@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_the_iteration_cap(lik):
    from pssgp.laplace_panel import LaplaceStateSpaceGPPanel
    kname = "m32"
    cases = PR.panel(lik)
    p = LaplaceStateSpaceGPPanel(list(cases), matern(kname), likelihood(lik), max_iter=2)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fits = p.fit_modes()
    need_more = [i for i in range(len(cases)) if PR.twin(kname, lik, i)[1]["iterations"] > 2]
    assert need_more and [i for i, f in enumerate(p.fit_info) if not f["converged"]] == need_more
    assert len(caught) == 1 and f"{len(need_more)} of {len(cases)}" in str(caught[0].message)
    for i, (t, y) in enumerate(cases):
        one = _single(kname, lik, t, y, max_iter=2)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            want = one.fit_mode()
        e = [err(fits[i][k], want[k]) for k in ("f", "v", "z", "s")] + [abs(fits[i]["log_evidence"] - want["log_evidence"])
                                                                         / max(1.0, abs(want["log_evidence"]))]
        assert max(e) <= TOL_SEARCH, (i, e)
        assert p.fit_info[i]["iterations"] == one.fit_info["iterations"] and p.fit_info[i]["halvings"] == one.fit_info["halvings"]


def test_per_series_models_and_exposures():
    from pssgp.laplace_panel import LaplaceStateSpaceGPPanel
    from pssgp.kernels import Matern32
    cases = PR.panel("poisson")
    S = len(cases)
    rng = np.random.RandomState(3)
    thetas = np.column_stack([rng.uniform(0.5, 2.0, S), rng.uniform(0.3, 1.0, S)])
    expo = list(rng.uniform(0.5, 3.0, S))
    kern = Matern32(variance=1.0, lengthscales=0.5)
    p = LaplaceStateSpaceGPPanel(list(cases), kern, [likelihood("poisson", e) for e in expo])
    names = [n for _, n in p.trainable_parameters()]
    ev = p.log_evidences(thetas)
    assert (kern.variance, kern.lengthscales) == (1.0, 0.5) or np.allclose([float(kern.variance), float(kern.lengthscales)], [1.0, 0.5])
    for s, (t, y) in enumerate(cases):
        from pssgp.laplace import LaplaceStateSpaceGP
        k = Matern32(**{n: thetas[s, j] for j, n in enumerate(names)})
        want = float(LaplaceStateSpaceGP((t[:, None], y[:, None]), k, likelihood("poisson", expo[s])).maximum_log_likelihood_objective())
        assert abs(ev[s] - want) <= TOL_SEARCH * max(1.0, abs(want)), (s, ev[s], want)
    # swapping the settings of two series of equal data swaps their results
    twice = [cases[3], cases[3]]
    q = LaplaceStateSpaceGPPanel(twice, kern, [likelihood("poisson", expo[0]), likelihood("poisson", expo[1])])
    a = q.log_evidences(thetas[:2])
    q2 = LaplaceStateSpaceGPPanel(twice, kern, [likelihood("poisson", expo[1]), likelihood("poisson", expo[0])])
    b = q2.log_evidences(thetas[:2][::-1])
    assert a[0] != a[1] and np.array_equal(_bits(a), _bits(b[::-1]))


@pytest.mark.parametrize("lik", LIKELIHOODS)
@pytest.mark.parametrize("kname", KNAMES)
def test_gradient(kname, lik):
    from pssgp.laplace_panel import LaplaceStateSpaceGPPanel
    cases = PR.panel(lik)
    p = LaplaceStateSpaceGPPanel(list(cases), matern(kname), likelihood(lik))
    ev, grads = p.log_evidences_and_grads()
    total = np.zeros(grads.shape[1])
    for i, (t, y) in enumerate(cases):
        ref = PR.dense(kname, lik, i, grad=True)
        one_ev, one_g = _single(kname, lik, t, y).log_likelihood_and_grad()
        scale = max(1.0, float(np.max(np.abs(ref["gradient"]))))
        e_dense = float(np.max(np.abs(grads[i] - ref["gradient"]))) / scale
        e_one = float(np.max(np.abs(grads[i] - one_g))) / max(1.0, float(np.max(np.abs(one_g))))
        print(f"{kname} {lik} n {t.size}: grad vs dense {e_dense:.1e} vs single {e_one:.1e}")
        assert e_dense <= MATERNS[kname][2] and e_one <= TOL_SEARCH
        assert abs(ev[i] - float(one_ev)) <= TOL_SEARCH * max(1.0, abs(float(one_ev)))
        total += grads[i]
    ll, g = p.log_likelihood_and_grad()
    assert abs(float(ll) - float(np.sum(ev))) <= 1e-12 * abs(float(np.sum(ev)))
    assert float(np.max(np.abs(g - total))) <= 1e-10 * max(1.0, float(np.max(np.abs(total))))
    _, gm = p.log_likelihood_and_grad(wrt=[0])
    assert gm[0] == g[0] and np.all(gm[1:] == 0.0)


@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_predict(lik):
    from pssgp.laplace_panel import LaplaceStateSpaceGPPanel
    kname = "m52"
    cases = list(PR.panel(lik)) + [PR.panel(lik, (2040,))[0]]
    rng = np.random.RandomState(5)
    counts = [40, 3, 0, 9, 64, 1, 17, 20]                   # (series 2 has none; 2040 + 20 crosses the limit: it leaves the call)
    Xnews = []
    for (t, _), k in zip(cases, counts):
        x = rng.uniform(t[0] - 0.1, t[-1] + 0.1, k)
        Xnews.append(np.concatenate([x, x[:2]]) if k > 2 else x)    # (any order, repeats)
    p = LaplaceStateSpaceGPPanel(cases, matern(kname), likelihood(lik))
    pf, py = p.predict_f(Xnews), p.predict_y(Xnews)
    pd = p.predict_log_density([(x, np.ones(x.size)) for x in Xnews])
    for i, (t, y) in enumerate(cases):
        one = _single(kname, lik, t, y)
        if Xnews[i].size == 0:
            assert pf[i][0].shape == (0, 1) and pf[i][1].shape == (0, 1)
            continue
        wf, wy = one.predict_f(Xnews[i][:, None]), one.predict_y(Xnews[i][:, None])
        wd = one.predict_log_density((Xnews[i][:, None], np.ones((Xnews[i].size, 1))))
        e = [err(pf[i][0], wf[0]), err(pf[i][1], wf[1]), err(py[i][0], wy[0]), err(py[i][1], wy[1]), err(pd[i], wd)]
        print(f"{lik} n {t.size} k {Xnews[i].size}: " + " ".join(f"{x:.1e}" for x in e))
        assert max(e) <= TOL_SEARCH, (i, e)


def test_abi_errors_and_device_forms():
    from pssgp import _backend as Bk
    lik = "poisson"
    cases = PR.panel(lik)
    offs, ts, ys = _concat(cases)
    S, n = len(cases), int(offs[-1])
    ctx = Bk.get_context()
    table, d = Bk._gp_rows([_model("m32")])
    par = np.array([PARS[lik]])
    rows = [np.full(n, np.nan) for _ in range(4)]
    info = np.full((S, 8), np.nan)
    out = np.full((S, 2 + d * d + 2 * d), np.nan)
    P = Bk._ptr

    def fit(S_=S, offs_=offs, d_=d, nm=1, table_=table, lik_=LR.LIKS[lik], npars=1, par_=par, ts_=ts, tol=1e-8, max_iter=50, f=rows[0]):
        return ctx.lib.pgps_gp_panel_laplace_f64(ctx.handle, S_, P(offs_), d_, nm, P(table_), lik_, npars, P(par_), P(ts_), P(ys), tol,
                                                 max_iter, P(f), P(rows[1]), P(rows[2]), P(rows[3]), P(info))

    def grad(**kw):
        a = dict(S_=S, offs_=offs, d_=d, nm=1, lik_=LR.LIKS[lik], npars=1, par_=par)
        a.update(kw)
        return ctx.lib.pgps_gp_panel_laplace_grad_f64(ctx.handle, a["S_"], P(a["offs_"]), a["d_"], a["nm"], P(table), a["lik_"], a["npars"],
                                                      P(a["par_"]), P(ts), P(ys), P(rows[0]), P(rows[1]), P(rows[2]), P(rows[3]), P(out))

    bad_offs = offs.copy(); bad_offs[0] = 1
    empty = offs.copy(); empty[2] = empty[1]
    lam0 = table.copy(); lam0[0, 0] = 0.0
    invalid = [dict(S_=0), dict(offs_=bad_offs), dict(offs_=empty), dict(nm=2), dict(npars=2), dict(lik_=7), dict(par_=np.array([0.0])),
               dict(par_=np.array([np.inf])), dict(tol=-1.0), dict(tol=np.nan), dict(max_iter=0), dict(max_iter=1001), dict(table_=lam0),
               dict(ts_=None), dict(f=None)]
    for kw in invalid:
        assert fit(**kw) == -1, kw
    assert fit(d_=4) == -2 and fit(d_=0) == -2
    for kw in (dict(S_=0), dict(offs_=bad_offs), dict(nm=2), dict(npars=2), dict(lik_=7), dict(par_=np.array([-1.0]))):
        assert grad(**kw) == -1, kw
    assert grad(d_=4) == -2
    assert all(np.all(np.isnan(a)) for a in rows + [info, out])
    # the host forms, then the device forms on a PanelData: the same bits
    assert fit() == 0 and grad() == 0
    data = Bk.PanelData(offs, ts, ys)
    try:
        dev = Bk.panel.gp_panel_laplace_dev(data, [_model("m32")], LR.LIKS[lik], par, rows=True)
        dout = Bk.panel.gp_panel_laplace_grad_dev(data, [_model("m32")], LR.LIKS[lik], par)
    finally:
        data.close()
    for a, k in zip(rows, ROWS):
        assert np.array_equal(_bits(a), _bits(dev[k])), k
    assert np.array_equal(_bits(info), _bits(dev["info"])) and np.array_equal(_bits(out), _bits(dout))
