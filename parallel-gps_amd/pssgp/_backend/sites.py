"""Laplace inference on the fused path (pgps_gp_newton_*, pgps_lik_sites_*): the host-array calls, and
the device buffers a mode search keeps between its Newton steps."""
import numpy as np

from .arrays import _prep, _ptr, _series_inputs
from .context import get_context
from .fused import _fused_model
from .library import _require, c_void_p

LIK_GAUSSIAN, LIK_BERNOULLI_LOGIT, LIK_POISSON_EXP = 0, 1, 2            # PGPS_LIK_*
LIK_W_MIN = 1e-10               # kLikWMin of csrc/pgps_lik.h: the floor of W = -d^2 log p / d f^2
NEWTON_SUMS = ("ll_sites", "lp", "f_alpha", "correction", "max_move", "n_obs")


def _site_context(device):
    return _require(get_context(device), "pgps_gp_newton_f64", "pgps_gp_newton_* / pgps_lik_sites_*")


def gp_newton(form, Pinf, H, lik, par, ts, ys, zs, ss, f_prev=None, t0=0.0, device=0):
    """One Newton step of the mode search on host arrays (pgps_gp_newton_f64): the smoothing pass over the sites (zs, ss),
    the likelihood `lik` (LIK_*) with parameter `par` at the new iterate.  Returns a dict: "f", "v", "alpha", "zs", "ss" (N,)
    and "sums" (6,) in the order of NEWTON_SUMS."""
    ts_a, ys_a, N = _series_inputs(ts, ys)
    zs_a, ss_a = _prep(zs, np.float64, (-1,)), _prep(ss, np.float64, (-1,))
    fp_a = None if f_prev is None else _prep(f_prev, np.float64, (-1,))
    for a in (zs_a, ss_a) + (() if fp_a is None else (fp_a,)):
        if a.shape[0] != N:
            raise ValueError(f"the sites and the previous iterate must have the series' {N} rows, got {a.shape[0]}")
    d, model = _fused_model(form, Pinf, H)
    out = {k: np.empty(N, np.float64) for k in ("f", "v", "alpha", "zs", "ss")}
    out["sums"] = np.zeros(6, np.float64)
    _site_context(device).call("pgps_gp_newton_f64", N, d, *model, int(lik), float(par), _ptr(ts_a), _ptr(ys_a), _ptr(zs_a),
                               _ptr(ss_a), _ptr(fp_a), float(t0), *(_ptr(out[k]) for k in ("f", "v", "alpha", "zs", "ss", "sums")))
    return out


def lik_sites(lik, par, ys, f_a, alpha_a, f_b=None, alpha_b=None, step=0.0, device=0):
    """The sites at f = f_a + step (f_b - f_a) (f_b None: f_a), alpha likewise (pgps_lik_sites_f64).  Returns a dict: "f",
    "alpha", "zs", "ss" (N,) and "sums" (3,) = (sum lp, sum f alpha, sum [lp - log N(zs | f, ss)])."""
    ys_a = _prep(ys, np.float64, (-1,))
    N = ys_a.shape[0]
    rows = [None if a is None else _prep(a, np.float64, (-1,)) for a in (f_a, alpha_a, f_b, alpha_b)]
    if any(a is not None and a.shape[0] != N for a in rows):
        raise ValueError(f"every array must have the observations' {N} rows")
    out = {k: np.empty(N, np.float64) for k in ("f", "alpha", "zs", "ss")}
    out["sums"] = np.zeros(3, np.float64)
    _site_context(device).call("pgps_lik_sites_f64", N, int(lik), float(par), _ptr(ys_a), *(_ptr(a) for a in rows), float(step),
                               *(_ptr(out[k]) for k in ("f", "alpha", "zs", "ss", "sums")))
    return out


class SiteBuffers:
    """The device side of one mode search: ts, ys and two sets of the five per-step arrays (f, alpha, v, zs, ss) -- the
    CURRENT iterate with the sites formed at it and the PROPOSAL a pass writes -- plus the pass's sums.  ts and ys are copied up
    once; a Newton step or a damped step brings back its sums alone.  Calls go through the _dev entry points under the
    context's lock.  close() (or the garbage collector) frees the memory."""

    _ARRAYS = ("f", "alpha", "v", "zs", "ss")

    def __init__(self, ts, ys, lik, par, t0=0.0, device=0):
        self.ctx = _site_context(device)
        ts_a, ys_a, self.N = _series_inputs(ts, ys)
        self.lik, self.par, self.t0 = int(lik), float(par), float(t0)
        n = self.N
        self._base = self.ctx.malloc(8 * (12 * n + 8))
        at = lambda i: c_void_p(self._base + 8 * n * i)
        self.ts, self.ys = at(0), at(1)
        self.cur = {k: at(2 + i) for i, k in enumerate(self._ARRAYS)}
        self.new = {k: at(7 + i) for i, k in enumerate(self._ARRAYS)}
        self._sums_d = at(12)
        self._sums = np.zeros(8, np.float64)
        self.ctx.h2d(self.ts.value, ts_a)
        self.ctx.h2d(self.ys.value, ys_a)

    def close(self):
        if getattr(self, "_base", None):
            self.ctx.free(self._base)
            self._base = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _sums_back(self, n):
        self.ctx.d2h(self._sums, self._sums_d.value)
        return self._sums[:n].copy()

    def start(self, f0=None):
        """The current iterate := f0 (zeros when None) with alpha = 0, and the sites at it.  Returns (sum lp, sum f alpha,
        correction)."""
        zeros = np.zeros(self.N, np.float64)
        self.ctx.h2d(self.cur["f"].value, zeros if f0 is None else _prep(f0, np.float64, (self.N,)))
        self.ctx.h2d(self.cur["alpha"].value, zeros)
        c = self.cur
        self.ctx.call("pgps_lik_sites_dev_f64", self.N, self.lik, self.par, self.ys, c["f"], c["alpha"], None, None, 0.0,
                      c["f"], c["alpha"], c["zs"], c["ss"], self._sums_d)
        return self._sums_back(3)

    def newton(self, model, d):
        """One pass over the current sites into the proposal's arrays; `model` = the (lam, N1, N2, Pinf, H) arguments of
        _fused_model.  Returns the six sums (NEWTON_SUMS)."""
        c, p = self.cur, self.new
        self.ctx.call("pgps_gp_newton_dev_f64", self.N, d, *model, self.lik, self.par, self.ts, self.ys, c["zs"], c["ss"], c["f"],
                      self.t0, p["f"], p["v"], p["alpha"], p["zs"], p["ss"], self._sums_d)
        return self._sums_back(6)

    def halve(self):
        """The proposal := the midpoint of the current iterate and the proposal, in (f, alpha), with the sites formed there
        (elementwise and in place: k halvings leave current + 2^-k (Newton point - current)).  Returns (sum lp, sum f alpha,
        correction)."""
        c, p = self.cur, self.new
        self.ctx.call("pgps_lik_sites_dev_f64", self.N, self.lik, self.par, self.ys, c["f"], c["alpha"], p["f"], p["alpha"],
                      0.5, p["f"], p["alpha"], p["zs"], p["ss"], self._sums_d)
        return self._sums_back(3)

    def accept(self):
        """The proposal becomes the current iterate."""
        self.cur, self.new = self.new, self.cur

    def fetch(self, name, proposal=False):
        """One per-step array of the current iterate (or of the proposal) as a host array (N,)."""
        out = np.empty(self.N, np.float64)
        self.ctx.d2h(out, (self.new if proposal else self.cur)[name].value)
        return out
