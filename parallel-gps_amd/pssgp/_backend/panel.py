"""A panel: S independent series, each on its own clock and of its own length, evaluated in one launch per group
(pgps_gp_panel_*, include/pgps.h; fp64, Matern-family models, d <= 3).  Host-array calls, and PanelData: the concatenated
series kept on the device across calls, which the *_dev functions run on."""
import numpy as np

from .arrays import _prep, _ptr
from .batch import _gp_rows
from .context import get_context
from .library import _require

PANEL_MAX_STEPS = 2048          # PGPS_PANEL_MAX_STEPS: steps of one series, counted merged (n + k) in predict


def _panel_context(device):
    return _require(get_context(device), "pgps_gp_panel_ll_f64", "pgps_gp_panel_*")


def _offsets(offs, what="offs"):
    o = np.ascontiguousarray(offs, dtype=np.int64).reshape(-1)
    if o.shape[0] < 2 or o[0] != 0:
        raise ValueError(f"{what} must hold S + 1 >= 2 offsets starting at 0, got {o!r}")
    return o


def _table(models, S):
    """(table, d, nmodels) of `models` as _gp_rows takes them: one row (shared by all series) or S rows."""
    table, d = _gp_rows(models)
    if table.shape[0] not in (1, S):
        raise ValueError(f"a panel of {S} series takes 1 model (shared) or {S}, got {table.shape[0]}")
    return table, d, table.shape[0]


def _inputs(offs, ts, ys, rs):
    o = _offsets(offs)
    n = int(o[-1])
    ts_a, ys_a = _prep(ts, np.float64, (-1,)), _prep(ys, np.float64, (-1,))
    rs_a = None if rs is None else _prep(rs, np.float64, (-1,))
    for name, a in (("ts", ts_a), ("ys", ys_a), ("rs", rs_a)):
        if a is not None and a.shape[0] != n:
            raise ValueError(f"{name} has {a.shape[0]} rows, offs ends at {n}")
    return o, ts_a, ys_a, rs_a


PANEL_GRAM_COLUMNS_MAX = 8      # kPanelGramMax: columns C = 1 + p of pgps_gp_panel_gram_*


def _columns(V, n):
    V_a = np.ascontiguousarray(V, dtype=np.float64)
    if V_a.ndim != 2 or V_a.shape[0] != n or V_a.shape[1] < 1:
        raise ValueError(f"V must be ({n}, C) like the concatenated rows, got shape {V_a.shape}")
    return V_a


def gp_panel_ll(models, offs, ts, ys, rs=None, device=0):
    """Log-likelihoods (S,) of the S series cut out of the concatenated ts, ys (and rs: per-observation noise variances, or None)
    by `offs` (S + 1,); `models`: 1 or S entries as gp_ll_batch takes them, or their table (pgps_gp_panel_ll_f64)."""
    o, ts_a, ys_a, rs_a = _inputs(offs, ts, ys, rs)
    S = o.shape[0] - 1
    table, d, nm = _table(models, S)
    ll = np.empty(S, np.float64)
    _panel_context(device).call("pgps_gp_panel_ll_f64", S, _ptr(o), d, nm, _ptr(table), _ptr(ts_a), _ptr(ys_a), _ptr(rs_a), _ptr(ll))
    return ll


def gp_panel_ll_grad(models, offs, ts, ys, rs=None, device=0):
    """(S, 1 + d d + 2 d + 1): row s = [ll | Abar | Ubar | Hbar | Rbar] of series s (pgps_gp_panel_ll_grad_f64; split_grad_stats)."""
    o, ts_a, ys_a, rs_a = _inputs(offs, ts, ys, rs)
    S = o.shape[0] - 1
    table, d, nm = _table(models, S)
    out = np.empty((S, 2 + d * d + 2 * d), np.float64)
    _panel_context(device).call("pgps_gp_panel_ll_grad_f64", S, _ptr(o), d, nm, _ptr(table), _ptr(ts_a), _ptr(ys_a), _ptr(rs_a),
                                _ptr(out))
    return out


def gp_panel_predict(models, offs, qoffs, ts, ys, rs, tq, device=0):
    """predict_f of every series at its own (sorted) queries, rows qoffs[s] .. qoffs[s + 1] of tq (a series may have none):
    (mean, var (qoffs[S],), ll (S,)) (pgps_gp_panel_predict_f64)."""
    o, ts_a, ys_a, rs_a = _inputs(offs, ts, ys, rs)
    q = _offsets(qoffs, "qoffs")
    S = o.shape[0] - 1
    tq_a = _prep(tq, np.float64, (-1,))
    if q.shape[0] != S + 1 or tq_a.shape[0] != int(q[-1]):
        raise ValueError(f"qoffs must hold {S + 1} offsets ending at the {tq_a.shape[0]} rows of tq, got {q!r}")
    table, d, nm = _table(models, S)
    K = tq_a.shape[0]
    mean, var, ll = np.empty(K, np.float64), np.empty(K, np.float64), np.empty(S, np.float64)
    _panel_context(device).call("pgps_gp_panel_predict_f64", S, _ptr(o), _ptr(q), d, nm, _ptr(table), _ptr(ts_a), _ptr(ys_a),
                                _ptr(rs_a), _ptr(tq_a), _ptr(mean), _ptr(var), _ptr(ll))
    return mean, var, ll


class PanelData:
    """The concatenated series of a panel on the device: ts, ys (and rs) uploaded once, owned by this object and freed with
    it; the *_dev functions below run the device-pointer entry points on them.  Query grids and results travel per call
    through buffers that grow as needed and are owned here too."""

    def __init__(self, offs, ts, ys, rs=None, device=0, V=None):
        self.ctx = _panel_context(device)
        self.offs, ts_a, ys_a, rs_a = _inputs(offs, ts, ys, rs)
        self.S = self.offs.shape[0] - 1
        self.ys_host = ys_a             # (gp_panel_loo_dev forms the log densities from it)
        self._bufs = {}
        self._fixed = []
        self.V, self.C = None, 0        # the columns [y, Phi] of a panel with a mean function (gp_panel_gram_dev), resident too
        try:
            self.ts, self.ys = self._upload(ts_a), self._upload(ys_a)
            self.rs = None if rs_a is None else self._upload(rs_a)
            if V is not None:
                V_a = _columns(V, int(self.offs[-1]))
                self.V, self.C = self._upload(V_a), V_a.shape[1]
        except Exception:
            self.close()
            raise

    def residual_view(self):
        """A PanelData on the same ts / rs (borrowed: this object keeps owning them) whose ys is a buffer of this object that
        gp_panel_residual_dev fills: what the panel calls run on at given trend coefficients, with no row crossing the bus.
        It has no host copy of ys (the predictive checks' log densities need one)."""
        view = object.__new__(PanelData)
        view.ctx, view.offs, view.S = self.ctx, self.offs, self.S
        view.ts, view.rs, view.V, view.C = self.ts, self.rs, None, 0
        view.ys = self._buffer("residual", 8 * int(self.offs[-1]))
        view.ys_host = None
        view._bufs, view._fixed = self._bufs, []        # (its per-call buffers are this object's; close() frees nothing of its own)
        view.close = lambda: None
        return view

    def _upload(self, a):
        p = self.ctx.malloc(a.nbytes)
        self._fixed.append(p)
        self.ctx.h2d(p, a)
        return p

    def _buffer(self, name, nbytes):
        """A device buffer of at least nbytes under `name`, grown (never shrunk) across calls."""
        have = self._bufs.get(name)
        if have is None or have[1] < nbytes:
            if have is not None:
                self.ctx.free(have[0])
                del self._bufs[name]
            have = self._bufs[name] = (self.ctx.malloc(nbytes), nbytes)
        return have[0]

    def close(self):
        ctx = getattr(self, "ctx", None)
        if ctx is None or not getattr(ctx.handle, "value", None):
            return
        for p in self._fixed + [b[0] for b in self._bufs.values()]:
            ctx.free(p)
        self._fixed, self._bufs = [], {}

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass


def gp_panel_ll_dev(data, models):
    """gp_panel_ll on the resident series of `data` (pgps_gp_panel_ll_dev_f64): (S,)."""
    table, d, nm = _table(models, data.S)
    ll = np.empty(data.S, np.float64)
    with data.ctx.lock:
        dll = data._buffer("out", ll.nbytes)
        data.ctx.call("pgps_gp_panel_ll_dev_f64", data.S, _ptr(data.offs), d, nm, _ptr(table), data.ts, data.ys, data.rs, dll)
        data.ctx.d2h(ll, dll)
    return ll


def gp_panel_ll_grad_dev(data, models):
    """gp_panel_ll_grad on the resident series of `data` (pgps_gp_panel_ll_grad_dev_f64): (S, 1 + d d + 2 d + 1)."""
    table, d, nm = _table(models, data.S)
    out = np.empty((data.S, 2 + d * d + 2 * d), np.float64)
    with data.ctx.lock:
        dout = data._buffer("out", out.nbytes)
        data.ctx.call("pgps_gp_panel_ll_grad_dev_f64", data.S, _ptr(data.offs), d, nm, _ptr(table), data.ts, data.ys, data.rs, dout)
        data.ctx.d2h(out, dout)
    return out


def gp_panel_predict_dev(data, models, qoffs, tq):
    """gp_panel_predict on the resident series of `data` (pgps_gp_panel_predict_dev_f64): the queries go up, (mean, var
    (qoffs[S],), ll (S,)) come back."""
    q = _offsets(qoffs, "qoffs")
    tq_a = _prep(tq, np.float64, (-1,))
    if q.shape[0] != data.S + 1 or tq_a.shape[0] != int(q[-1]):
        raise ValueError(f"qoffs must hold {data.S + 1} offsets ending at the {tq_a.shape[0]} rows of tq, got {q!r}")
    table, d, nm = _table(models, data.S)
    K = tq_a.shape[0]
    res = np.empty(2 * K + data.S, np.float64)              # [mean | var | ll]: one copy back
    with data.ctx.lock:
        dtq = data._buffer("tq", tq_a.nbytes)
        dres = data._buffer("res", res.nbytes)
        data.ctx.h2d(dtq, tq_a)
        data.ctx.call("pgps_gp_panel_predict_dev_f64", data.S, _ptr(data.offs), _ptr(q), d, nm, _ptr(table), data.ts, data.ys,
                      data.rs, dtq, dres, dres + 8 * K, dres + 16 * K)
        data.ctx.d2h(res, dres)
    return res[:K], res[K:2 * K], res[2 * K:]


# -- mean functions of a panel (pgps_gp_panel_gram_*, pgps_gp_panel_residual_dev_f64) ---------------------
def _gram_context(ctx):
    return _require(ctx, "pgps_gp_panel_gram_f64", "pgps_gp_panel_gram_*")


def _split_gram(out, C):
    """(G (S, C, C), logdet (S,), n_obs (S,) int64) of the records [G | logdet | n_obs]."""
    S = out.shape[0]
    return (out[:, :C * C].reshape(S, C, C).copy(), out[:, C * C].copy(), np.rint(out[:, C * C + 1]).astype(np.int64))


def gp_panel_gram(models, offs, ts, V, rs=None, device=0):
    """(G (S, C, C), logdet (S,), n_obs (S,)) of the S series cut out of the concatenated ts, V (offs[S], C) by `offs`: G of
    series s is V_s^T K_y^-1 V_s with K_y = K + diag(R + rs) on its observed rows (column 0 of V is y, NaN = missing; a row is NaN
    in all columns or in none), logdet = log |K_y| (pgps_gp_panel_gram_f64; C <= PANEL_GRAM_COLUMNS_MAX)."""
    o = _offsets(offs)
    V_a = _columns(V, int(o[-1]))
    o, ts_a, _, rs_a = _inputs(o, ts, V_a[:, 0], rs)
    S, C = o.shape[0] - 1, V_a.shape[1]
    table, d, nm = _table(models, S)
    out = np.empty((S, C * C + 2), np.float64)
    _gram_context(get_context(device)).call("pgps_gp_panel_gram_f64", S, _ptr(o), d, nm, _ptr(table), C, _ptr(ts_a), _ptr(V_a),
                                            _ptr(rs_a), _ptr(out))
    return _split_gram(out, C)


def gp_panel_gram_dev(data, models):
    """gp_panel_gram on the resident ts, V (and rs) of `data` (pgps_gp_panel_gram_dev_f64): the S records come back in one copy."""
    if data.V is None:
        raise ValueError("this PanelData holds no columns V")
    _gram_context(data.ctx)
    table, d, nm = _table(models, data.S)
    C = data.C
    out = np.empty((data.S, C * C + 2), np.float64)
    with data.ctx.lock:
        dout = data._buffer("gram", out.nbytes)
        data.ctx.call("pgps_gp_panel_gram_dev_f64", data.S, _ptr(data.offs), d, nm, _ptr(table), C, data.ts, data.V, data.rs, dout)
        data.ctx.d2h(out, dout)
    return _split_gram(out, C)


def gp_panel_residual_dev(data, betas, into):
    """into.ys[k] = V[k, 0] - sum_j V[k, 1 + j] betas[s, j] over the rows of every series s of `data` (its resident V), on the
    device (pgps_gp_panel_residual_dev_f64): betas (S, C - 1) go up, nothing comes back.  `into`: a PanelData of the same
    offsets (data.residual_view(), or `data` itself: its ys is overwritten)."""
    if data.V is None:
        raise ValueError("this PanelData holds no columns V")
    _gram_context(data.ctx)
    if into.S != data.S or not np.array_equal(into.offs, data.offs):
        raise ValueError("`into` must hold the offsets of `data`")
    b = np.ascontiguousarray(betas, dtype=np.float64).reshape(data.S, -1)
    if b.shape[1] != data.C - 1:
        raise ValueError(f"betas must be ({data.S}, {data.C - 1}), got {np.shape(betas)}")
    with data.ctx.lock:
        db = data._buffer("betas", max(8, b.nbytes))
        if b.nbytes:
            data.ctx.h2d(db, b)
        data.ctx.call("pgps_gp_panel_residual_dev_f64", data.S, _ptr(data.offs), data.C, data.V, db, into.ys)
    return into


# -- the GLS solves on the device and the profile gradient in one call (pgps_gp_panel_trend_solve_*, pgps_gp_panel_profile_grad_*;
#    DESIGN.md section 4ae) -----------------------------------------------------------------------------------------------------
SOL_FIELDS = ("profile", "flat", "logdet_A", "status")     # what follows cov (p, p) in a row of sol


def _trend_context(ctx):
    return _require(ctx, "pgps_gp_panel_profile_grad_dev_f64", "pgps_gp_panel_profile_grad_*")


def split_sol(sol, p):
    """A dict of the rows of sol (S, p p + 4): "cov" (S, p, p), "profile", "flat", "logdet_A" (S,), "status" (S,) int64."""
    S = sol.shape[0]
    out = {"cov": sol[:, :p * p].reshape(S, p, p).copy()}
    for i, name in enumerate(SOL_FIELDS):
        out[name] = sol[:, p * p + i].copy()
    out["status"] = np.rint(out["status"]).astype(np.int64)
    return out


def gp_panel_trend_solve(records, C, device=0):
    """(betas_hat (S, C - 1), sol (S, (C - 1)^2 + 4)) of the Gram records (S, C C + 2) = [G | logdet | n_obs] as pgps_gp_panel_gram_*
    writes them: every series' GLS solve by one lane of one launch (pgps_gp_panel_trend_solve_f64).  A row of sol is
    [cov (p, p) | profile | flat | logdet_A | status] (split_sol); a series whose status is not 0 has NaN rows."""
    C = int(C)
    r = np.ascontiguousarray(records, dtype=np.float64)
    if not 1 <= C <= PANEL_GRAM_COLUMNS_MAX or r.ndim != 2 or r.shape[0] < 1 or r.shape[1] != C * C + 2:
        raise ValueError(f"records must be (S, C C + 2) with C = {C} in 1 .. {PANEL_GRAM_COLUMNS_MAX}, got shape {r.shape}")
    S, p = r.shape[0], C - 1
    betas, sol = np.empty((S, p), np.float64), np.empty((S, p * p + 4), np.float64)
    _trend_context(get_context(device)).call("pgps_gp_panel_trend_solve_f64", S, C, _ptr(r), _ptr(betas) if p else None, _ptr(sol))
    return betas, sol


def gp_panel_profile_grad_dev(data, models):
    """(rows (S, 1 + d d + 2 d + 1), betas_hat (S, C - 1), sol (S, (C - 1)^2 + 4)) on the resident ts, V (and rs) of `data`
    (pgps_gp_panel_profile_grad_dev_f64): Gram, solve, residuals and the adjoint pass queued back to back.  rows[s] is the record of
    gp_panel_ll_grad_dev on the residual series y_s - Phi_s betas_hat[s], which are left in the buffer of data.residual_view().
    The three outputs lie in ONE buffer of `data` and come back in ONE copy."""
    if data.V is None:
        raise ValueError("this PanelData holds no columns V")
    _trend_context(data.ctx)
    table, d, nm = _table(models, data.S)
    S, C = data.S, data.C
    p, nout = C - 1, 2 + d * d + 2 * d
    nb, ns = S * p, S * (p * p + 4)
    res = np.empty(nb + ns + S * nout, np.float64)              # [betas | sol | rows]
    with data.ctx.lock:
        work = data.residual_view().ys
        dres = data._buffer("profile", res.nbytes)
        data.ctx.call("pgps_gp_panel_profile_grad_dev_f64", S, _ptr(data.offs), d, nm, _ptr(table), C, data.ts, data.V, data.rs,
                      dres, dres + 8 * nb, work, dres + 8 * (nb + ns))
        data.ctx.d2h(res, dres)
    return res[nb + ns:].reshape(S, nout), res[:nb].reshape(S, p), res[nb:nb + ns].reshape(S, p * p + 4)


# -- predictive checks of every series (pgps_gp_panel_loo_*) ---------------------------------------------
_CHECK_ARRAYS = ("osa_mean", "osa_var", "loo_mean", "loo_var")


def _checks_result(want, arrays, sums, ys):
    """The dict of fused.gp_loo over the concatenated rows: the arrays asked for and their log densities (formed here from
    (ys, mean, var), NaN where ys is: the library stores none), "ll" and "loo_lpd" (S,)."""
    from .fused import normal_log_density
    out = {k: v for k, v in arrays.items() if v is not None}
    for name in ("osa", "loo"):
        if want[name]:
            out[f"{name}_log_density"] = normal_log_density(ys, out[f"{name}_mean"], out[f"{name}_var"])
    out["ll"], out["loo_lpd"] = sums[:, 0].copy(), sums[:, 1].copy()
    return out


def gp_panel_loo(models, offs, ts, ys, rs=None, osa=True, loo=True, device=0):
    """The predictive checks of every series of a panel in one launch per group (pgps_gp_panel_loo_f64), host arrays: the dict
    of gp_loo with arrays over the concatenated rows (offs[S],) and "ll", "loo_lpd" of shape (S,).  Series s is what gp_loo
    returns on series s alone, with the step's noise variance R + rs[k] where rs is given.  osa = loo = False: no per-row
    array is stored or copied back."""
    o, ts_a, ys_a, rs_a = _inputs(offs, ts, ys, rs)
    S = o.shape[0] - 1
    table, d, nm = _table(models, S)
    n = int(o[-1])
    want = {"osa": bool(osa), "loo": bool(loo)}
    arrays = {k: (np.empty(n, np.float64) if want[k[:3]] else None) for k in _CHECK_ARRAYS}
    sums = np.zeros((S, 2), np.float64)
    ctx = _require(get_context(device), "pgps_gp_panel_loo_f64", "pgps_gp_panel_loo_*")
    ctx.call("pgps_gp_panel_loo_f64", S, _ptr(o), d, nm, _ptr(table), _ptr(ts_a), _ptr(ys_a), _ptr(rs_a),
             *(_ptr(arrays[k]) for k in _CHECK_ARRAYS), _ptr(sums))
    return _checks_result(want, arrays, sums, ys_a)


def gp_panel_loo_dev(data, models, osa=True, loo=True):
    """gp_panel_loo on the resident series of `data` (pgps_gp_panel_loo_dev_f64): [sums | the arrays asked for] come back in
    one copy (none asked for: 2 S doubles); the log densities are formed from the host copy of ys that `data` keeps."""
    _require(data.ctx, "pgps_gp_panel_loo_dev_f64", "pgps_gp_panel_loo_*")
    table, d, nm = _table(models, data.S)
    n = int(data.offs[-1])
    want = {"osa": bool(osa), "loo": bool(loo)}
    names = [k for k in _CHECK_ARRAYS if want[k[:3]]]
    res = np.empty(2 * data.S + len(names) * n, np.float64)
    with data.ctx.lock:
        dres = data._buffer("checks", res.nbytes)
        ptrs = {k: dres + 8 * (2 * data.S + i * n) for i, k in enumerate(names)}
        data.ctx.call("pgps_gp_panel_loo_dev_f64", data.S, _ptr(data.offs), d, nm, _ptr(table), data.ts, data.ys, data.rs,
                      *(ptrs.get(k) for k in _CHECK_ARRAYS), dres)
        data.ctx.d2h(res, dres)
    sums = res[:2 * data.S].reshape(data.S, 2)
    arrays = {k: None for k in _CHECK_ARRAYS}
    for i, k in enumerate(names):
        arrays[k] = res[2 * data.S + i * n:2 * data.S + (i + 1) * n]
    return _checks_result(want, arrays, sums, data.ys_host)


# -- Laplace inference on a panel (pgps_gp_panel_laplace_*) ---------------------------------------------
PANEL_INFO = ("ll_sites", "correction", "psi", "iterations", "halvings", "converged", "max_move", "n_obs")
NEWTON_MAX_ITER_CAP = 1000      # kNewtonMaxIterCap of csrc/pgps_newton.h


def _laplace_context(device):
    return _require(get_context(device), "pgps_gp_panel_laplace_f64", "pgps_gp_panel_laplace_*")


def _pars(pars, S):
    p = np.ascontiguousarray(pars, dtype=np.float64).reshape(-1)
    if p.shape[0] not in (1, S):
        raise ValueError(f"a panel of {S} series takes 1 likelihood parameter (shared) or {S}, got {p.shape[0]}")
    return p


def gp_panel_laplace(models, lik, pars, offs, ts, ys, tol=1e-8, max_iter=50, device=0):
    """The mode search of every series of a panel in one launch per group (pgps_gp_panel_laplace_f64), host arrays: a dict
    with "f", "v", "zs", "ss" (offs[S],) -- the modes, their variances, the sites at them -- and "info" (S, 8) in the order
    of PANEL_INFO.  `models` as gp_panel_ll takes them (R is ignored); `pars`: 1 or S likelihood parameters."""
    o, ts_a, ys_a, _ = _inputs(offs, ts, ys, None)
    S = o.shape[0] - 1
    table, d, nm = _table(models, S)
    p = _pars(pars, S)
    n = int(o[-1])
    out = {k: np.empty(n, np.float64) for k in ("f", "v", "zs", "ss")}
    out["info"] = np.empty((S, len(PANEL_INFO)), np.float64)
    _laplace_context(device).call("pgps_gp_panel_laplace_f64", S, _ptr(o), d, nm, _ptr(table), int(lik), p.shape[0], _ptr(p),
                                  _ptr(ts_a), _ptr(ys_a), float(tol), int(max_iter),
                                  *(_ptr(out[k]) for k in ("f", "v", "zs", "ss", "info")))
    return out


def gp_panel_laplace_grad(models, lik, pars, offs, ts, ys, f, v, zs, ss, device=0):
    """(S, 1 + d d + 2 d + 1): row s = [c | Abar | Ubar | Hbar | Rbar], the adjoint statistics of the evidence of series s at the
    mode gp_panel_laplace returned (pgps_gp_panel_laplace_grad_f64; split_grad_stats).  c is the combination
    G(z + w) - G(w) + G(0), not the evidence."""
    o, ts_a, ys_a, _ = _inputs(offs, ts, ys, None)
    S = o.shape[0] - 1
    table, d, nm = _table(models, S)
    p = _pars(pars, S)
    rows = [_prep(a, np.float64, (-1,)) for a in (f, v, zs, ss)]
    if any(a.shape[0] != int(o[-1]) for a in rows):
        raise ValueError(f"f, v, zs, ss must have the panel's {int(o[-1])} rows")
    out = np.empty((S, 2 + d * d + 2 * d), np.float64)
    _laplace_context(device).call("pgps_gp_panel_laplace_grad_f64", S, _ptr(o), d, nm, _ptr(table), int(lik), p.shape[0],
                                  _ptr(p), _ptr(ts_a), _ptr(ys_a), *(_ptr(a) for a in rows), _ptr(out))
    return out


def _site_rows(data):
    """The device addresses of f, v, zs, ss of `data`: one buffer the panel keeps between the fit, the gradient and predict."""
    n = int(data.offs[-1])
    base = data._buffer("sites", 4 * 8 * n)
    return [base + 8 * n * i for i in range(4)]


def gp_panel_laplace_dev(data, models, lik, pars, tol=1e-8, max_iter=50, rows=False):
    """gp_panel_laplace on the resident series of `data` (pgps_gp_panel_laplace_dev_f64).  f, v, zs, ss stay on the device in
    `data` for gp_panel_laplace_grad_dev / gp_panel_laplace_predict_dev; info (S, 8) comes back, and with rows=True the
    dict of gp_panel_laplace."""
    _require(data.ctx, "pgps_gp_panel_laplace_dev_f64", "pgps_gp_panel_laplace_*")
    table, d, nm = _table(models, data.S)
    p = _pars(pars, data.S)
    info = np.empty((data.S, len(PANEL_INFO)), np.float64)
    n = int(data.offs[-1])
    with data.ctx.lock:
        f, v, zs, ss = _site_rows(data)
        dinfo = data._buffer("info", info.nbytes)
        data.ctx.call("pgps_gp_panel_laplace_dev_f64", data.S, _ptr(data.offs), d, nm, _ptr(table), int(lik), p.shape[0], _ptr(p),
                      data.ts, data.ys, float(tol), int(max_iter), f, v, zs, ss, dinfo)
        data.ctx.d2h(info, dinfo)
        if not rows:
            return info
        back = np.empty(4 * n, np.float64)
        data.ctx.d2h(back, f)
    return {"f": back[:n], "v": back[n:2 * n], "zs": back[2 * n:3 * n], "ss": back[3 * n:], "info": info}


def gp_panel_laplace_grad_dev(data, models, lik, pars):
    """gp_panel_laplace_grad on the modes gp_panel_laplace_dev left in `data` (pgps_gp_panel_laplace_grad_dev_f64)."""
    table, d, nm = _table(models, data.S)
    p = _pars(pars, data.S)
    out = np.empty((data.S, 2 + d * d + 2 * d), np.float64)
    with data.ctx.lock:
        f, v, zs, ss = _site_rows(data)
        dout = data._buffer("out", out.nbytes)
        data.ctx.call("pgps_gp_panel_laplace_grad_dev_f64", data.S, _ptr(data.offs), d, nm, _ptr(table), int(lik), p.shape[0],
                      _ptr(p), data.ts, data.ys, f, v, zs, ss, dout)
        data.ctx.d2h(out, dout)
    return out


def gp_panel_laplace_predict_dev(data, models, qoffs, tq):
    """The posterior of f under the approximation at every series' queries: pgps_gp_panel_predict_dev_f64 on the sites
    gp_panel_laplace_dev left in `data` (ys = zs, rs = ss; the table's R must be 0).  (mean, var (qoffs[S],))."""
    q = _offsets(qoffs, "qoffs")
    tq_a = _prep(tq, np.float64, (-1,))
    if q.shape[0] != data.S + 1 or tq_a.shape[0] != int(q[-1]):
        raise ValueError(f"qoffs must hold {data.S + 1} offsets ending at the {tq_a.shape[0]} rows of tq, got {q!r}")
    table, d, nm = _table(models, data.S)
    K = tq_a.shape[0]
    res = np.empty(2 * K, np.float64)
    with data.ctx.lock:
        _, _, zs, ss = _site_rows(data)
        dtq = data._buffer("tq", tq_a.nbytes)
        dres = data._buffer("res", res.nbytes)
        data.ctx.h2d(dtq, tq_a)
        data.ctx.call("pgps_gp_panel_predict_dev_f64", data.S, _ptr(data.offs), _ptr(q), d, nm, _ptr(table), data.ts, zs, ss, dtq,
                      dres, dres + 8 * K, None)
        data.ctx.d2h(res, dres)
    return res[:K], res[K:]


# -- the hyper-parameter fit of every series (pgps_gp_panel_fit_*) --------------------------------------
FIT_INFO = ("ll", "ll_start", "iterations", "evaluations", "status", "grad_norm", "n_obs", "reserved")
FIT_PARAMETERS = 3              # kFitP of csrc/pgps_fit.h: variance, lengthscales, noise_variance


def _fit_arguments(S, unit, theta0, lo, hi, free):
    """The host arrays of a fit call: the unit row (or None), theta0 / lo / hi (S, 3) and free (3,) int32."""
    out = []
    for name, a in (("theta0", theta0), ("lo", lo), ("hi", hi)):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (S, FIT_PARAMETERS):
            raise ValueError(f"{name} must be ({S}, {FIT_PARAMETERS}), got shape {a.shape}")
        out.append(a)
    f = np.ascontiguousarray(free, dtype=np.int32).reshape(-1)
    if f.shape[0] != FIT_PARAMETERS:
        raise ValueError(f"free must hold {FIT_PARAMETERS} flags, got {f.shape[0]}")
    u = None if unit is None else np.ascontiguousarray(unit, dtype=np.float64).reshape(-1)
    return [u] + out + [f]


def gp_panel_fit(d, unit, offs, ts, ys, rs, theta0, lo, hi, free, gtol=1e-6, max_iter=100, device=0):
    """The fit of every series of a panel in one launch per group (pgps_gp_panel_fit_f64), host arrays: (thetas (S, 3), info
    (S, 8) in the order of FIT_INFO).  d = 1, 2, 3: Matern-1/2, -3/2, -5/2; `unit`: one model row, the Matern-5/2 SDE at lam = 1
    and variance 1 (None at d < 3); theta0, lo, hi (S, 3) in theta = (variance, lengthscales, noise_variance); free (3,) flags."""
    o, ts_a, ys_a, rs_a = _inputs(offs, ts, ys, rs)
    S = o.shape[0] - 1
    u, t0, lo_a, hi_a, f = _fit_arguments(S, unit, theta0, lo, hi, free)
    thetas, info = np.empty((S, FIT_PARAMETERS), np.float64), np.empty((S, len(FIT_INFO)), np.float64)
    ctx = _require(get_context(device), "pgps_gp_panel_fit_f64", "pgps_gp_panel_fit_*")
    ctx.call("pgps_gp_panel_fit_f64", S, _ptr(o), int(d), _ptr(u), _ptr(ts_a), _ptr(ys_a), _ptr(rs_a), _ptr(t0), _ptr(lo_a),
             _ptr(hi_a), _ptr(f), float(gtol), int(max_iter), _ptr(thetas), _ptr(info))
    return thetas, info


def gp_panel_fit_dev(data, d, unit, theta0, lo, hi, free, gtol=1e-6, max_iter=100):
    """gp_panel_fit on the resident series of `data` (pgps_gp_panel_fit_dev_f64): [thetas | info] come back in one copy."""
    _require(data.ctx, "pgps_gp_panel_fit_dev_f64", "pgps_gp_panel_fit_*")
    S = data.S
    u, t0, lo_a, hi_a, f = _fit_arguments(S, unit, theta0, lo, hi, free)
    nt = S * FIT_PARAMETERS
    res = np.empty(nt + S * len(FIT_INFO), np.float64)
    with data.ctx.lock:
        dres = data._buffer("fit", res.nbytes)
        data.ctx.call("pgps_gp_panel_fit_dev_f64", S, _ptr(data.offs), int(d), _ptr(u), data.ts, data.ys, data.rs, _ptr(t0),
                      _ptr(lo_a), _ptr(hi_a), _ptr(f), float(gtol), int(max_iter), dres, dres + 8 * nt)
        data.ctx.d2h(res, dres)
    return res[:nt].reshape(S, FIT_PARAMETERS), res[nt:].reshape(S, len(FIT_INFO))
