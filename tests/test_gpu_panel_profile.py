"""GPU tests of the panel's device solves and the profile gradient in one call (pgps_gp_panel_trend_solve_*,
pgps_gp_panel_profile_grad_*; k_panel_trend_solve, csrc/pgps_panel_trend.hip.h) and of
StateSpaceGPPanel.profile_log_likelihoods_and_grads on the device route.  ctypes -> C ABI.  Data and references:
panel_profile_refs.py / panel_trend_refs.py (a different seed per series; the numpy multi-column filter; numpy's dense solve of
the unit-diagonal system) -- none is the code under test.  Every case asserts panel_trend_refs.well_posed on the REFERENCE
record first (panel_profile_refs.ref_solution does).

Bounds.  The solve kernel on reference records: 64 p cond eps with cond taken from the reference -- the forward bound of a
Cholesky solve with the project's own constant (at most 1e-11 under cond <= 100) -- relative to max |beta|, to
sqrt(cov_ii cov_jj), and to the sums of magnitudes that enter profile and flat.  The chain on device records: 1e-9 on the profile
(the Gram tolerance of test_gpu_panel_trend.py) and 4 cond 1e-9 on beta (that file's bound).  Bits: exact."""
import ctypes

import numpy as np
import pytest

import panel_profile_refs as P
import panel_trend_refs as T
from het_refs import LOG2PI, R, rel
from panel_profile_refs import BASIS_C, LENGTHS
from test_gpu_panel import _BatchScratch, _kernel, _model, _same_bits
from test_gpu_multi_geometries import _Chunk

pytestmark = pytest.mark.gpu

TOL = 1e-9
HET = pytest.mark.parametrize("het", [False, True], ids=["scalar", "rs"])
S7 = len(LENGTHS)
E_INVALID = -1


def _records(kname, het, basis=None, C=None):
    """(records (7, C C + 2), [ref_solution of series i]) of the reference."""
    refs = [P.ref_solution(kname, i, het, basis, C) for i in range(S7)]
    return np.stack([r[0] for r in refs]), refs


def _solve(records, C):
    from pssgp import _backend as Bk
    return Bk.gp_panel_trend_solve(records, C)


# ---- 1. the solve kernel on reference records, through the host form ----------------------------------------------------------
@pytest.mark.parametrize("what", ["constant", "linear", "cubic", "wide8"])
@HET
def test_solve_against_the_reference(what, het):
    basis, C = (None, 8) if what == "wide8" else (what, BASIS_C[what])
    p = C - 1
    records, refs = _records("m32", het, basis, C)
    # the 7 records, then 300: the 7 repeated and permuted, so that a 256-lane workgroup boundary falls inside the panel
    pick = np.random.RandomState(3).permutation(np.arange(300) % S7)
    betas7, sol7 = _solve(records, C)
    betas300, sol300 = _solve(np.ascontiguousarray(records[pick]), C)
    assert betas7.shape == (S7, p) and sol7.shape == (S7, p * p + 4) and sol300.shape == (300, p * p + 4)
    for i, (rec, beta, cov, profile, flat, cond) in enumerate(refs):
        bound, s_prof, s_flat = P.solve_bounds(rec, C, cond)
        assert cond <= T.COND_MAX and bound <= 1e-11
        got_cov = sol7[i, :p * p].reshape(p, p)
        dg = np.sqrt(np.diag(cov))
        logdet_A = float(np.linalg.slogdet(np.asarray(rec[:C * C]).reshape(C, C)[1:, 1:])[1])
        e = [float(np.max(np.abs(betas7[i] - beta)) / np.max(np.abs(beta))), float(np.max(np.abs(got_cov - cov) / np.outer(dg, dg))),
             abs(sol7[i, p * p] - profile) / s_prof, abs(sol7[i, p * p + 1] - flat) / (s_flat + abs(logdet_A)),
             abs(sol7[i, p * p + 2] - logdet_A) / (s_flat + abs(logdet_A))]
        print(f"{what} rs {het} series {i}: cond {cond:.2f} bound {bound:.2e} beta {e[0]:.2e} cov {e[1]:.2e} profile {e[2]:.2e} "
              f"flat {e[3]:.2e} logdet_A {e[4]:.2e}")
        assert max(e) <= bound, (i, e, bound)
        assert sol7[i, p * p + 3] == 0.0
        _same_bits(got_cov, got_cov.T.copy(), ("cov is symmetric bit for bit", i))
        # alone, at every place among the 300, and on repetition
        b1, s1 = _solve(records[i:i + 1], C)
        _same_bits(b1[0], betas7[i], ("alone: betas", i))
        _same_bits(s1[0], sol7[i], ("alone: sol", i))
        for j in np.flatnonzero(pick == i):
            _same_bits(betas300[j], betas7[i], ("among 300: betas", i, j))
            _same_bits(sol300[j], sol7[i], ("among 300: sol", i, j))
    again = _solve(records, C)
    _same_bits(again[0], betas7, "repeated: betas")
    _same_bits(again[1], sol7, "repeated: sol")


@HET
def test_solve_with_one_column_has_nothing_to_solve(het):
    records, _ = _records("m32", het, None, 1)
    for recs in (records, np.ascontiguousarray(records[np.arange(300) % S7])):
        betas, sol = _solve(recs, 1)
        assert betas.shape == (recs.shape[0], 0) and sol.shape == (recs.shape[0], 4)
        want = -(recs[:, 2] * LOG2PI + recs[:, 1] + recs[:, 0]) / 2           # (left to right: n log 2 pi + logdet + G_00)
        _same_bits(sol[:, 0], want, "profile at C = 1")
        _same_bits(sol[:, 1], want, "flat = profile at C = 1")
        assert np.all(sol[:, 2] == 0.0) and np.all(sol[:, 3] == 0.0)


# ---- 2. status, on crafted records among good ones ----------------------------------------------------------------------------
def _with_A(rec, A):
    G = rec[:9].reshape(3, 3).copy()
    G[1:, 1:] = A
    return np.concatenate([G.reshape(-1), rec[9:]])


def test_status_of_crafted_records_among_good_ones():
    C, p = 3, 2
    records, _ = _records("m32", False, "linear")
    good_b, good_s = _solve(records, C)
    A0 = records[2, :9].reshape(3, 3)[1:, 1:]
    zero_diag, nan_entry = A0.copy(), A0.copy()
    zero_diag[1, 1] = 0.0
    nan_entry[0, 1] = np.nan                    # (in the upper triangle only)
    near = 1.0 - 1e-15
    assert 0.0 < 1.0 - near * near <= 64 * 2 * P.EPS          # pivot squared about 2e-15, under the threshold
    crafted = {1: (zero_diag, 1), 3: (nan_entry, 1), 4: (np.ones((2, 2)), 2), 6: (np.array([[1.0, near], [near, 1.0]]), 3)}
    recs = records.copy()
    for i, (A, _) in crafted.items():
        recs[i] = _with_A(records[i], A)
    betas, sol = _solve(recs, C)
    for i in range(S7):
        if i in crafted:
            assert sol[i, p * p + 3] == crafted[i][1], (i, sol[i, p * p + 3])
            assert np.all(np.isnan(betas[i])) and np.all(np.isnan(sol[i, :p * p + 3])), i
        else:
            _same_bits(betas[i], good_b[i], ("a neighbour's betas", i))
            _same_bits(sol[i], good_s[i], ("a neighbour's sol", i))


# ---- 3. the chain ---------------------------------------------------------------------------------------------------------------
def _concat(C, het, order=None, other=False):
    """(offs, ts, V, rs or None) of the panel's series in `order` with the C wide columns; other: other data of the same shape."""
    cases = T.panel(LENGTHS)
    idx = list(range(S7) if order is None else order)
    offs = np.concatenate([[0], np.cumsum([cases[i][0].size for i in idx])]).astype(np.int64)
    V = np.concatenate([T.wide_columns(cases[i][0], cases[i][1], C) for i in idx])
    if other:
        V = V.copy()
        V[:, 0] = 1.0 - V[:, 0]
    return offs, np.concatenate([cases[i][0] for i in idx]), np.ascontiguousarray(V), (np.concatenate([cases[i][2] for i in idx]) if het else None)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class _Device:
    """The panel on the device with buffers for everything the chain writes; .separate() runs the four _dev calls, .fused() the one."""

    def __init__(self, table, d, offs, ts, V, rs):
        from pssgp import _backend as Bk
        self.data = Bk.PanelData(offs, ts, V[:, 0], rs, V=V)
        self.table, self.d, self.nm = table, d, table.shape[0]
        S, C = self.data.S, self.data.C
        p = C - 1
        self.sizes = {"rec": S * (C * C + 2), "betas": S * p, "sol": S * (p * p + 4), "work": int(offs[-1]), "out": S * (2 + d * d + 2 * d)}
        self.buf = {k: self.data._buffer("t_" + k, 8 * max(1, n)) for k, n in self.sizes.items()}

    def _poison(self):
        for k, n in self.sizes.items():
            self.data.ctx.h2d(self.buf[k], np.full(max(1, n), -3.0))

    def _read(self, names):
        out = {}
        for k in names:
            out[k] = np.empty(self.sizes[k], np.float64)
            self.data.ctx.d2h(out[k], self.buf[k])
        return out

    def separate(self):
        dt, b, call = self.data, self.buf, self.data.ctx.call
        self._poison()
        head = (dt.S, _p(dt.offs), self.d, self.nm, _p(self.table))
        call("pgps_gp_panel_gram_dev_f64", *head, dt.C, dt.ts, dt.V, dt.rs, b["rec"])
        call("pgps_gp_panel_trend_solve_dev_f64", dt.S, dt.C, b["rec"], b["betas"], b["sol"])
        call("pgps_gp_panel_residual_dev_f64", dt.S, _p(dt.offs), dt.C, dt.V, b["betas"], b["work"])
        call("pgps_gp_panel_ll_grad_dev_f64", *head, dt.ts, b["work"], dt.rs, b["out"])
        return self._read(("betas", "sol", "work", "out"))

    def fused(self):
        dt, b = self.data, self.buf
        self._poison()
        dt.ctx.call("pgps_gp_panel_profile_grad_dev_f64", dt.S, _p(dt.offs), self.d, self.nm, _p(self.table), dt.C, dt.ts, dt.V, dt.rs,
                    b["betas"], b["sol"], b["work"], b["out"])
        return self._read(("betas", "sol", "work", "out"))

    def close(self):
        self.data.close()


def _host(table, d, offs, ts, V, rs):
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    S, C = offs.size - 1, V.shape[1]
    p = C - 1
    out = {"betas": np.full(S * p, -3.0), "sol": np.full(S * (p * p + 4), -3.0), "out": np.full(S * (2 + d * d + 2 * d), -3.0)}
    ctx.call("pgps_gp_panel_profile_grad_f64", S, _p(offs), d, table.shape[0], _p(table), C, _p(ts), _p(V), _p(rs), _p(out["betas"]),
             _p(out["sol"]), _p(out["out"]))
    return out


def _equal(got, want, what, names=("betas", "sol", "out")):
    for k in names:
        _same_bits(got[k], want[k], (what, k))


@pytest.mark.parametrize("kname", T.KNAMES)
@HET
@pytest.mark.parametrize("C", [2, 5])
def test_the_chain_has_the_bits_of_its_four_parts(kname, het, C):
    from pssgp import _backend as Bk
    table, d = Bk._gp_rows([_model(kname)])
    dev, other = _Device(table, d, *_concat(C, het)), _Device(table, d, *_concat(C, het, other=True))
    try:
        for chunk in (0, 4):
            for budget in (0, 1, 300 * 1024):           # the library's own; every series its own group; a few series per group
                with _Chunk(chunk), _BatchScratch(budget):
                    other.separate()
                    want = dev.separate()
                    other.fused()                       # (every checked call follows the same call on other data: scratch is not zeroed)
                    got = dev.fused()
                    assert not np.any(got["out"] == -3.0) and not np.any(got["sol"] == -3.0)
                    assert np.all(got["sol"].reshape(S7, -1)[:, -1] == 0.0)
                    _equal(got, want, (kname, het, C, chunk, budget), ("betas", "sol", "work", "out"))
                    if chunk == 0:
                        _host(table, d, *_concat(C, het, other=True))
                        _equal(_host(table, d, *_concat(C, het)), got, ("the host form", kname, het, C, budget))
    finally:
        dev.close()
        other.close()


@pytest.mark.parametrize("kname", T.KNAMES)
@HET
def test_a_row_of_the_chain_depends_on_nothing_but_its_series(kname, het):
    from pssgp import _backend as Bk
    C = 5
    table, d = Bk._gp_rows([_model(kname)])
    want = {k: v.reshape(S7, -1) for k, v in _host(table, d, *_concat(C, het)).items()}
    rev = list(range(S7 - 1, -1, -1))
    _host(table, d, *_concat(C, het, other=True))
    got = {k: v.reshape(S7, -1) for k, v in _host(table, d, *_concat(C, het, order=rev)).items()}
    for j, i in enumerate(rev):
        for k in want:
            _same_bits(got[k][j], want[k][i], ("reversed", k, i))
    rows = np.ascontiguousarray(np.repeat(table, S7, axis=0))
    _host(rows, d, *_concat(C, het, other=True))
    _equal(_host(rows, d, *_concat(C, het)), {k: v.reshape(-1) for k, v in want.items()}, "S equal rows of the model table")


# ---- 4. the chain against the references --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", T.KNAMES)
@HET
@pytest.mark.parametrize("basis", ["linear", "cubic"])
def test_the_chain_against_the_references(kname, het, basis):
    from pssgp import _backend as Bk
    C = BASIS_C[basis]
    p = C - 1
    refs = [P.ref_solution(kname, i, het, basis) for i in range(S7)]
    cases = T.panel(LENGTHS)
    offs = np.concatenate([[0], np.cumsum([c[0].size for c in cases])]).astype(np.int64)
    V = np.concatenate([P.columns_of(i, basis) for i in range(S7)])
    rs = np.concatenate([c[2] for c in cases]) if het else None
    table, d = Bk._gp_rows([_model(kname)])
    got = _host(table, d, offs, np.concatenate([c[0] for c in cases]), V, rs)
    betas, sol, out = got["betas"].reshape(S7, p), got["sol"].reshape(S7, -1), got["out"].reshape(S7, -1)
    for i, (_, beta, _, profile, _, cond) in enumerate(refs):
        bound = 4.0 * cond * TOL
        e = [abs(out[i, 0] - profile) / abs(profile), abs(sol[i, p * p] - profile) / abs(profile),
             float(np.max(np.abs(betas[i] - beta)) / np.max(np.abs(beta)))]
        print(f"{kname} rs {het} {basis} series {i}: out ll {e[0]:.2e} sol profile {e[1]:.2e} beta {e[2]:.2e} (bound {bound:.2e})")
        assert max(e[:2]) <= TOL and e[2] <= bound, (i, e)
        assert sol[i, -1] == 0.0


# ---- 5. the ABI's errors leave every output untouched ---------------------------------------------------------------------------
def test_abi_errors_leave_every_output_untouched():
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    lib = ctx.lib
    C = 3
    offs, ts, V, rs = _concat(C, True)
    table, d = Bk._gp_rows([_model("m32")])
    outs = [np.full(S7 * 8 * 8, -3.0) for _ in range(3)]           # betas, sol, out: larger than any case below
    dev = _Device(table, d, offs, ts, V, rs)
    try:
        dev._poison()
        b, dt = dev.buf, dev.data

        def host(offs_=offs, S_=S7, C_=C, V_=V, rs_=rs, table_=table, betas=outs[0], sol=outs[1], out=outs[2]):
            return lib.pgps_gp_panel_profile_grad_f64(ctx.handle, S_, _p(offs_), d, 1, _p(table_), C_, _p(ts), _p(V_), _p(rs_),
                                                      _p(betas), _p(sol), _p(out))

        def devf(offs_=offs, S_=S7, C_=C, rs_=dt.rs, table_=table, betas=b["betas"], sol=b["sol"], work=b["work"], out=b["out"]):
            return lib.pgps_gp_panel_profile_grad_dev_f64(ctx.handle, S_, _p(offs_), d, 1, _p(table_), C_, dt.ts, dt.V, rs_, betas, sol,
                                                          work, out)

        zero_R = table.copy()
        zero_R[0, -1] = 0.0
        big = np.zeros((2049, 9))
        long_offs = np.array([0, 2049], np.int64)
        invalid = {"C = 0": host(C_=0), "C = 9": host(C_=9, V_=big), "a 2049-row series": host(S_=1, offs_=long_offs, V_=big),
                   "null sol": host(sol=None), "null out": host(out=None), "null betas": host(betas=None),
                   "R = 0 without rs": host(table_=zero_R, rs_=None),
                   "C = 0 (dev)": devf(C_=0), "C = 9 (dev)": devf(C_=9), "a 2049-row series (dev)": devf(S_=1, offs_=long_offs),
                   "null sol (dev)": devf(sol=None), "null out (dev)": devf(out=None), "null ys_work (dev)": devf(work=None),
                   "null betas (dev)": devf(betas=None), "R = 0 without rs (dev)": devf(table_=zero_R, rs_=None),
                   "solve C = 0": lib.pgps_gp_panel_trend_solve_f64(ctx.handle, S7, 0, _p(V), _p(outs[0]), _p(outs[1])),
                   "solve C = 9": lib.pgps_gp_panel_trend_solve_f64(ctx.handle, S7, 9, _p(big), _p(outs[0]), _p(outs[1])),
                   "solve null sol": lib.pgps_gp_panel_trend_solve_f64(ctx.handle, S7, C, _p(V), _p(outs[0]), None),
                   "solve null betas": lib.pgps_gp_panel_trend_solve_f64(ctx.handle, S7, C, _p(V), None, _p(outs[1])),
                   "solve null sol (dev)": lib.pgps_gp_panel_trend_solve_dev_f64(ctx.handle, S7, C, b["rec"], b["betas"], None)}
        assert {k: v for k, v in invalid.items() if v != E_INVALID} == {}
        assert all(np.all(o == -3.0) for o in outs), "a refused call must not touch the outputs"
        for k, v in dev._read(("betas", "sol", "work", "out")).items():
            assert np.all(v == -3.0), ("a refused call must not touch the device outputs", k)
        assert ctx.status() == 0
        # the context still works: R = 0 is accepted with rs, and the plain call gives the _dev form's bits
        assert host(table_=zero_R) == 0 and host() == 0 and devf() == 0
        p = C - 1
        got = dev._read(("betas", "sol", "out"))
        _same_bits(outs[0][:S7 * p], got["betas"], "betas")
        _same_bits(outs[1][:S7 * (p * p + 4)], got["sol"], "sol")
        _same_bits(outs[2][:S7 * (2 + d * d + 2 * d)], got["out"], "out")
    finally:
        dev.close()


# ---- 6. the class on the device route ------------------------------------------------------------------------------------------
class _Spy:
    """Counts the calls of the _backend.panel wrappers the class takes (restored on exit)."""
    NAMES = ("gp_panel_gram_dev", "gp_panel_residual_dev", "gp_panel_ll_dev", "gp_panel_ll_grad_dev", "gp_panel_predict_dev",
             "gp_panel_loo_dev", "gp_panel_profile_grad_dev", "gp_panel_trend_solve")

    def __enter__(self):
        from pssgp import _backend as Bk
        self.calls, self._saved = [], []
        for name in self.NAMES:
            fn = getattr(Bk.panel, name)
            self._saved.append((name, fn))
            setattr(Bk.panel, name, self._wrap(name, fn))
        return self

    def _wrap(self, name, fn):
        def inner(*a, **kw):
            self.calls.append(name)
            return fn(*a, **kw)
        return inner

    def take(self):
        out, self.calls = self.calls, []
        return out

    def __exit__(self, *exc):
        from pssgp import _backend as Bk
        for name, fn in self._saved:
            setattr(Bk.panel, name, fn)


def _class_panel(kname, het, basis, lengths=LENGTHS, mean_function=None, series=None):
    from pssgp.panel import StateSpaceGPPanel
    cases = T.panel(lengths) if series is None else series
    return StateSpaceGPPanel([(t, y) for t, y, _ in cases], _kernel(kname), noise_variance=R, parallel=True,
                             observation_variances=[s for _, _, s in cases] if het else None,
                             mean_function=T.bases()[basis] if mean_function is None else mean_function)


def _reference_grad(kname, het, basis, i, theta, beta_ref, lengths=LENGTHS):
    """(ll, gradient) of the zero-mean model on the REFERENCE residuals y - Phi beta_ref of series i at `theta` (or the shared
    setting): oracle.np_grad with scalar noise, the single-series adjoint entry point with rs (np_grad has one R for all steps)."""
    from oracle import np_grad as G
    from pssgp.kernels.sde_grads import sde_with_grads
    from pssgp.model import StateSpaceGP
    t, y, s = T.panel(lengths)[i]
    Rv = R if theta is None else float(theta[2])
    res = y - T.design(basis, t) @ beta_ref
    if het:
        m = StateSpaceGP((t[:, None], res[:, None]), P.kernel_at(kname, theta), noise_variance=Rv, parallel=True, observation_variances=s)
        l1, g1 = m.log_likelihood_and_grad(method="adjoint")
        return float(l1), np.asarray(g1, np.float64)
    sde, kgrads = sde_with_grads(P.kernel_at(kname, theta))
    stats = G.ll_grad_stats(sde.F, sde.P0, sde.H, Rv, t[~np.isnan(res)], res[~np.isnan(res)])
    return float(stats[0]), np.asarray(G.contract(stats, sde.H, kgrads), np.float64)


@pytest.mark.parametrize("kname", T.KNAMES)
@HET
@pytest.mark.parametrize("basis", ["linear", "cubic"])
def test_the_class_on_the_device_route(kname, het, basis):
    panel = _class_panel(kname, het, basis)
    p = BASIS_C[basis] - 1
    before = np.arange(float(S7 * p)).reshape(S7, p)
    panel.betas = before
    setting = (float(panel.kernel.variance), float(panel.kernel.lengthscales), float(panel.noise_variance))
    thetas = P.theta_rows(S7)
    with _Spy() as spy:
        for own in (False, True):
            lls, grads = panel.profile_log_likelihoods_and_grads(thetas if own else None)
            assert spy.take() == ["gp_panel_profile_grad_dev"]
            assert lls.shape == (S7,) and grads.shape == (S7, 3)
            for i in range(S7):
                _, beta, _, profile, _, _ = P.ref_solution(kname, i, het, basis, None, own)
                w_ll, w_g = _reference_grad(kname, het, basis, i, thetas[i] if own else None, beta)
                spy.take()                              # (the reference's own device calls with rs are not the method's)
                e = [abs(lls[i] - profile) / abs(profile), abs(lls[i] - w_ll) / abs(w_ll), rel(grads[i], w_g)]
                print(f"{kname} rs {het} {basis} own thetas {own} series {i}: ll {e[0]:.2e} {e[1]:.2e} gradient {e[2]:.2e}")
                assert max(e) <= TOL, (own, i, e)
        total, grad = panel.profile_log_likelihoods_and_grads(reduce="sum")
        assert spy.take() == ["gp_panel_profile_grad_dev"]
        w_total, w_grad = panel.profile_log_likelihood_and_grad()
        assert spy.take() == ["gp_panel_gram_dev", "gp_panel_residual_dev", "gp_panel_ll_grad_dev"]
    assert isinstance(total, np.float64) and grad.shape == (3,)
    e = [abs(float(total) - float(w_total)) / abs(float(w_total)), rel(grad, w_grad)]
    print(f"{kname} rs {het} {basis}: reduce='sum' against profile_log_likelihood_and_grad {e[0]:.2e} {e[1]:.2e}")
    assert max(e) <= TOL, e
    assert np.array_equal(panel.betas, before)
    assert (float(panel.kernel.variance), float(panel.kernel.lengthscales), float(panel.noise_variance)) == setting


@HET
def test_a_long_series_is_spliced_and_nine_columns_take_the_loop(het):
    from pssgp.mean_functions import Basis
    lengths = (37, 3000, 300)
    panel = _class_panel("m32", het, "linear", lengths=lengths)
    with _Spy() as spy:
        lls, grads = panel.profile_log_likelihoods_and_grads()
        assert spy.take() == ["gp_panel_profile_grad_dev"] and panel._panel_data.S == 2
        total, grad = panel.profile_log_likelihoods_and_grads(reduce="sum")
        assert spy.take() == ["gp_panel_profile_grad_dev"]
    for i in range(3):
        G_ref = T.ref_gram("m32", lengths, i, het, "linear")
        T.well_posed(*G_ref, ("spliced", i))
        beta, _, profile = T.gls_from_gram(*G_ref)[:3]
        w_ll, w_g = _reference_grad("m32", het, "linear", i, None, beta, lengths)
        e = [abs(lls[i] - profile) / abs(profile), abs(lls[i] - w_ll) / abs(w_ll), rel(grads[i], w_g)]
        print(f"rs {het} lengths {lengths} series {i}: ll {e[0]:.2e} {e[1]:.2e} gradient {e[2]:.2e}")
        assert max(e) <= TOL, (i, e)
    assert abs(float(total) - np.sum(lls)) <= TOL * abs(np.sum(lls)) and rel(grad, np.sum(grads, axis=0)) <= TOL
    # C = 9: off the panel entry points -- the loop, and the spy sees no new wrapper
    cos8 = Basis(lambda t: np.stack([np.cos(j * np.pi * (t - 0.05)) for j in range(8)], axis=1), 8)
    wide = _class_panel("m32", het, None, lengths=(37, 300), mean_function=cos8)
    with _Spy() as spy:
        lls, grads = wide.profile_log_likelihoods_and_grads()
        assert spy.take() == [] and wide._panel_data.V is None
        total, grad = wide.profile_log_likelihoods_and_grads(reduce="sum")
        assert spy.take() == []
    profiles = wide.profile_log_likelihoods()
    assert np.max(np.abs(lls - profiles) / np.abs(profiles)) <= TOL
    assert abs(float(total) - np.sum(lls)) <= TOL * abs(np.sum(lls)) and rel(grad, np.sum(grads, axis=0)) <= TOL


@HET
def test_a_rank_deficient_series_is_named_on_the_device_route(het):
    """All observed rows of series 2 at ONE time under Linear: its two basis functions are collinear on the observed rows."""
    from pssgp.mean_functions import Linear
    cases = list(T.panel(LENGTHS))
    n = 40
    t = np.linspace(0.1, 0.9, n)
    t[10:16] = 0.4
    y = np.full(n, np.nan)
    y[10:16] = np.array([0.3, -0.1, 0.2, 0.05, -0.3, 0.1])
    cases[2] = (t, y, np.full(n, 0.02))
    panel = _class_panel("m32", het, None, mean_function=Linear(), series=cases)
    before = panel.betas.copy()
    setting = (float(panel.kernel.variance), float(panel.kernel.lengthscales), float(panel.noise_variance))
    with _Spy() as spy:
        for kw in ({}, {"reduce": "sum"}, {"thetas": P.theta_rows(S7)}):
            with pytest.raises(ValueError, match="series 2"):
                panel.profile_log_likelihoods_and_grads(**kw)
            assert spy.take() == ["gp_panel_profile_grad_dev"]
    assert np.array_equal(panel.betas, before)
    assert (float(panel.kernel.variance), float(panel.kernel.lengthscales), float(panel.noise_variance)) == setting
