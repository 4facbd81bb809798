"""A series kept on the device across calls (pgps_series_*), and the packed models its calls take.  The calls here are the
host cost of every optimiser / sampler step: pointers are made once and reused, scalars go in as plain Python numbers."""
import ctypes

import numpy as np

from .. import _backend as _facade      # `check` is looked up there at every call: tests wrap it to record the routes
from .arrays import _prep, _ptr, _scalar_out, _series_inputs
from .batch import _gp_rows, _lti_table
from .context import get_context
from .library import _require, c_void_p
from .lti import LTI_DIM_MAX, LTI_DIM_MIN, split_grad_stats


class _Packed(tuple):
    """(lam, N1, N2, Pinf, H, d) of Series.pack with the arrays' ctypes pointers made once (`.ptrs`: four data_as() calls are
    3 us of a 36 us evaluation)."""

    def __new__(cls, items, ptrs=None):
        self = super().__new__(cls, items)
        self.ptrs = tuple(_ptr(a) for a in items[1:5]) if ptrs is None else ptrs
        return self


class PackBuffer:
    """One model's (N1, N2, Pinf, H) in a buffer that lives as long as the model: a new hyper-parameter setting copies 30
    doubles into it and reuses the four ctypes pointers (making them is ~10 us of a 40 us evaluation at a new setting).
    The tuple `pack()` returns is valid until the next `pack()`: the series calls are synchronous, nothing keeps an older one."""

    def __init__(self, d):
        self.d = d
        self.buf = np.zeros(3 * d * d + d, np.float64)
        dd = d * d
        self.views = (self.buf[0:dd].reshape(d, d), self.buf[dd:2 * dd].reshape(d, d), self.buf[2 * dd:3 * dd].reshape(d, d),
                      self.buf[3 * dd:3 * dd + d])
        base = self.buf.ctypes.data
        self.ptrs = (c_void_p(base), c_void_p(base + 8 * dd), c_void_p(base + 16 * dd), c_void_p(base + 24 * dd))

    def pack(self, form, Pinf, H):
        lam, N1, N2 = form
        v = self.views
        v[0][...] = N1
        v[1][...] = N2
        v[2][...] = Pinf
        v[3][...] = np.asarray(H).reshape(-1)
        return _Packed((float(lam), v[0], v[1], v[2], v[3], self.d), self.ptrs)


class Series:
    """A series kept on the device across calls (pgps_series_*, include/pgps.h): what an optimiser or sampler loop
    evaluates thousands of times is ONE (ts, ys) at changing hyper-parameters, and predict_f on a fixed grid.  The
    handle holds ts, ys and -- once set -- the query grid merged with them; a call sends the fused model's scalars and
    returns the log-likelihood (+ gradient), or the K posterior means and variances.  fp64, Matern-family models."""

    def __init__(self, ts, ys, t0=0.0, device=0):
        self.ctx = get_context(device)
        ts_a, ys_a, self.N = _series_inputs(ts, ys)
        lib = _require(self.ctx, "pgps_series_create_f64", "pgps_series_*").lib
        self.has_lti = hasattr(lib, "pgps_series_lti_ll_f64")
        self.has_lti_grad = hasattr(lib, "pgps_series_lti_ll_grad_f64")
        self.has_gp_adj = hasattr(lib, "pgps_series_gp_ll_grad_adj_f64")
        self.K = 0
        self._tq = None
        h = c_void_p()
        with self.ctx.lock:
            _facade.check(self.ctx, lib.pgps_series_create_f64(self.ctx.handle, self.N, _ptr(ts_a), _ptr(ys_a), float(t0), ctypes.byref(h)),
                          "pgps_series_create_f64")
        self.handle = h
        self._ll, self._llp = _scalar_out()
        self._gout = np.zeros(32, np.float64)
        self._goutp = _ptr(self._gout)
        self._lti_slots = {}

    def set_queries(self, tq):
        """The (sorted) query times of predict(); merged with the series on the device once."""
        tq_a = _prep(tq, np.float64, (-1,))
        if self._tq is not None and self._tq.shape == tq_a.shape and np.array_equal(self._tq, tq_a):
            return
        with self.ctx.lock:
            _facade.check(self.ctx, self.ctx.lib.pgps_series_set_queries_f64(self.handle, tq_a.shape[0], _ptr(tq_a)),
                          "pgps_series_set_queries_f64")
        self._tq, self.K = tq_a.copy(), tq_a.shape[0]
        self._mean, self._var = np.empty(self.K, np.float64), np.empty(self.K, np.float64)
        self._meanp, self._varp = _ptr(self._mean), _ptr(self._var)

    @staticmethod
    def pack(form, Pinf, H):
        """The fused model as the contiguous float64 arrays the calls take: (lam, N1, N2, Pinf, H, d)."""
        lam, N1, N2 = form
        d = N1.shape[0]
        c = lambda a, shape: a if (type(a) is np.ndarray and a.dtype == np.float64 and a.flags.c_contiguous and a.shape == shape) \
            else _prep(a, np.float64, shape)
        Hv = np.asarray(H, np.float64).reshape(-1)
        return _Packed((float(lam), c(N1, (d, d)), c(N2, (d, d)), c(Pinf, (d, d)), c(Hv, (d,)), d))

    def gp_ll(self, packed, R):
        lam, N1, N2, Pinf, H, d = packed
        p1, p2, p3, p4 = packed.ptrs if hasattr(packed, "ptrs") else (_ptr(N1), _ptr(N2), _ptr(Pinf), _ptr(H))
        with self.ctx.lock:
            _facade.check(self.ctx, self.ctx.lib.pgps_series_gp_ll_f64(self.handle, d, lam, p1, p2, p3, p4,
                                                                       float(R), self._llp), "pgps_series_gp_ll_f64")
        return self._ll.value

    # -- any kernel's LTI model (F, Pinf, H), fp64, 2 <= d <= 32: pgps_series_lti_* ------------------------------
    def _lti_slot(self, F, Pinf, H):
        """(d, pF, pPinf, pH, out, pout): the model copied into this handle's buffer for its state dimension -- the ctypes
        pointers of a dimension are made once (three data_as() calls and an output array per evaluation were ~10 us)."""
        F = np.asarray(F)
        d = F.shape[0]
        slot = self._lti_slots.get(d)
        if slot is None:
            if F.ndim != 2 or F.shape[1] != d or not (LTI_DIM_MIN <= d <= LTI_DIM_MAX):
                raise ValueError(f"the general-LTI device path covers state dimensions {LTI_DIM_MIN}..{LTI_DIM_MAX}, got {F.shape}")
            dd = d * d
            buf = np.zeros(2 * dd + d, np.float64)
            out = np.zeros(2 + dd + 2 * d, np.float64)
            base = buf.ctypes.data
            slot = self._lti_slots[d] = (buf, buf[0:dd].reshape(d, d), buf[dd:2 * dd].reshape(d, d), buf[2 * dd:2 * dd + d],
                                         c_void_p(base), c_void_p(base + 8 * dd), c_void_p(base + 16 * dd), out, _ptr(out))
        slot[1][...] = F
        slot[2][...] = Pinf
        slot[3][...] = np.asarray(H).reshape(-1)
        return d, slot[4], slot[5], slot[6], slot[7], slot[8]

    def lti_ll(self, F, Pinf, H, R):
        d, pF, pP, pH, _, _ = self._lti_slot(F, Pinf, H)
        with self.ctx.lock:
            _facade.check(self.ctx, self.ctx.lib.pgps_series_lti_ll_f64(self.handle, d, pF, pP, pH, float(R), self._llp),
                          "pgps_series_lti_ll_f64")
        return self._ll.value

    def lti_ll_grad(self, F, Pinf, H, R):
        """(ll, Abar, Ubar, Hbar, Rbar): the log-likelihood and the model's adjoints (pgps_series_lti_ll_grad_f64)."""
        d, pF, pP, pH, out, pout = self._lti_slot(F, Pinf, H)
        with self.ctx.lock:
            _facade.check(self.ctx, self.ctx.lib.pgps_series_lti_ll_grad_f64(self.handle, d, pF, pP, pH, float(R), pout),
                          "pgps_series_lti_ll_grad_f64")
        return split_grad_stats(out, d)

    def lti_predict(self, F, Pinf, H, R):
        """(mean (K,), var (K,), ll) at the query grid of set_queries()."""
        d, pF, pP, pH, _, _ = self._lti_slot(F, Pinf, H)
        with self.ctx.lock:
            _facade.check(self.ctx, self.ctx.lib.pgps_series_lti_predict_f64(self.handle, d, pF, pP, pH, float(R),
                                                                            self._meanp, self._varp, self._llp),
                          "pgps_series_lti_predict_f64")
        return self._mean.copy(), self._var.copy(), self._ll.value

    def _table_call(self, name, table, d, width):
        """One batched call of `name`: the (B, ...) model table in, a (B,) (width None) or (B, width) array out."""
        B = table.shape[0]
        out = np.empty(B if width is None else (B, width), np.float64)
        with self.ctx.lock:
            _facade.check(self.ctx, getattr(self.ctx.lib, name)(self.handle, B, d, _ptr(table), _ptr(out)), name)
        return out

    def lti_ll_batch(self, models):
        """B log-likelihoods: models = [(F, Pinf, H, R)] of one state dimension (2 <= d <= 16)."""
        table, d = _lti_table(models)
        return self._table_call("pgps_series_lti_ll_batch_f64", table, d, None)

    def gp_ll_grad(self, model, d, npar):
        with self.ctx.lock:
            _facade.check(self.ctx, self.ctx.lib.pgps_series_gp_ll_grad_f64(self.handle, d, npar, _ptr(model), _ptr(self._gout)),
                          "pgps_series_gp_ll_grad_f64")
        return float(self._gout[0]), self._gout[1:1 + npar].copy()

    def gp_ll_grad_adj(self, packed, R):
        """(ll, Abar, Ubar, Hbar, Rbar) of the fused (Matern-family) model by the adjoint pass on the lane-chunk kernels
        (pgps_series_gp_ll_grad_adj_f64): the same statistics as lti_ll_grad(), contracted by contract_grad_stats()."""
        lam, N1, N2, Pinf, H, d = packed
        with self.ctx.lock:
            _facade.check(self.ctx, self.ctx.lib.pgps_series_gp_ll_grad_adj_f64(self.handle, d, lam, _ptr(N1), _ptr(N2), _ptr(Pinf), _ptr(H),
                                                                                float(R), _ptr(self._gout)), "pgps_series_gp_ll_grad_adj_f64")
        return split_grad_stats(self._gout[:2 + d * d + 2 * d].copy(), d)

    def gp_ll_grad_adj_raw(self, packed, R):
        """The same call, results left in the handle's output buffer [ll | Abar | Ubar | Hbar | Rbar] (a view: valid until
        the next call) -- for callers that contract them in place."""
        lam, N1, N2, Pinf, H, d = packed
        p1, p2, p3, p4 = packed.ptrs if hasattr(packed, "ptrs") else (_ptr(N1), _ptr(N2), _ptr(Pinf), _ptr(H))
        with self.ctx.lock:
            _facade.check(self.ctx, self.ctx.lib.pgps_series_gp_ll_grad_adj_f64(self.handle, d, lam, p1, p2, p3, p4,
                                                                                float(R), self._goutp), "pgps_series_gp_ll_grad_adj_f64")
        return self._gout

    def gp_ll_grad_adj_batch(self, models):
        """B fused models in one set of launches (pgps_series_gp_ll_grad_adj_batch_f64): a (B, 1 + d d + 2 d + 1) array, row b
        = [ll | Abar | Ubar | Hbar | Rbar] of model b.  `models` as gp_ll_batch takes them, or a table."""
        packed, d = _gp_rows(models)
        return self._table_call("pgps_series_gp_ll_grad_adj_batch_f64", packed, d, 2 + d * d + 2 * d)

    def lti_ll_grad_batch(self, models):
        """The same for B general LTI models [(F, Pinf, H, R)] of one state dimension 2 .. 16, or their table
        (pgps_series_lti_ll_grad_batch_f64): the models side by side on the row-cooperative kernels."""
        table, d = _lti_table(models)
        return self._table_call("pgps_series_lti_ll_grad_batch_f64", table, d, 2 + d * d + 2 * d)

    def gp_predict(self, packed, R):
        """(mean (K,), var (K,), ll) at the query grid of set_queries()."""
        lam, N1, N2, Pinf, H, d = packed
        p1, p2, p3, p4 = packed.ptrs if hasattr(packed, "ptrs") else (_ptr(N1), _ptr(N2), _ptr(Pinf), _ptr(H))
        mean, var = np.empty(self.K, np.float64), np.empty(self.K, np.float64)
        with self.ctx.lock:
            _facade.check(self.ctx, self.ctx.lib.pgps_series_gp_predict_f64(self.handle, d, lam, p1, p2, p3,
                                                                            p4, float(R), _ptr(mean), _ptr(var), self._llp),
                          "pgps_series_gp_predict_f64")
        return mean, var, self._ll.value

    def _predict_batch(self, name, packed, d, mix):
        B = packed.shape[0]
        rows = 1 if mix is not None else B
        mean, var, ll = np.empty((rows, self.K), np.float64), np.empty((rows, self.K), np.float64), np.empty(B, np.float64)
        wv = None if mix is None else _prep(mix, np.float64, (B,))
        with self.ctx.lock:
            _facade.check(self.ctx, getattr(self.ctx.lib, name)(self.handle, B, d, _ptr(packed), _ptr(wv), _ptr(mean), _ptr(var), _ptr(ll)),
                          name)
        if mix is not None:
            return None, None, ll, (mean[0], var[0])
        return mean, var, ll, None

    def gp_predict_batch(self, models, mix=None):
        """B fused models at the query grid of set_queries() in one set of launches (pgps_series_gp_predict_batch_f64):
        (mean (B, K), var (B, K), ll (B,), None); with `mix` (B normalised weights) the (B, K) results stay on the device
        and (None, None, ll, (mixture mean (K,), mixture variance (K,))) comes back."""
        packed, d = _gp_rows(models)
        return self._predict_batch("pgps_series_gp_predict_batch_f64", packed, d, mix)

    def lti_predict_batch(self, models, mix=None):
        """The same for B general LTI models [(F, Pinf, H, R)] of one state dimension 2 .. 16
        (pgps_series_lti_predict_batch_f64): the models side by side on the row-cooperative kernels, one copy back."""
        table, d = _lti_table(models)
        return self._predict_batch("pgps_series_lti_predict_batch_f64", table, d, mix)

    def close(self):
        h, self.handle = getattr(self, "handle", None), None
        if h and self.ctx is not None and getattr(self.ctx.handle, "value", None):
            with self.ctx.lock:
                self.ctx.lib.pgps_series_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass
