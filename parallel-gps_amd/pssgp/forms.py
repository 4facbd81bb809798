"""The device forms of a kernel: what StateSpaceGP hands to the HIP entry points instead of (N, d, d) arrays.

`fused` = (sde-like, (lam, N1, N2)) where the SDE has the closed-form discretisation of the fused path (F = -lam I + N, N
nilpotent, d <= 3: the Matern family), `lti` = the SDE (F, P0, H) of the general-LTI path (2 <= d <= 32).  The pure parts are
functions (the stationarity residual, the Matern closed forms); what reads the model's memos is `ModelForms`, a mixin of
StateSpaceGP.
"""
from types import SimpleNamespace

import numpy as np

from . import _backend, config
from .kernels import RBF
from .kernels.base import Kernel, _tree_ids
from .kernels.sde_grads import leaf_parameters

_MATERN52_CHECKED = {}      # the same key -> the scaled unit form reproduced the kernel's own get_sde() (checked once per process)
_MATERN52_UNITS = {}        # (class, balancing sweeps, config sweeps) -> (Pinf, H, N, N^2 / 2) of the Matern-5/2 SDE at lam = 1, s2 = 1
_MATERN_DIMS = {"Matern12": 1, "Matern32": 2, "Matern52": 3}


def stationarity_residual(sde, F, P0):
    """(max |F P0 + P0 F^T + L Q L^T|, its bound 1e-8 max(1, max |L Q L^T|)): the device discretisation forms
    Q_k = P0 - F_k P0 F_k^T, which needs P0 stationary -- a model whose residual exceeds the bound stays on the host."""
    L = np.asarray(sde.L, np.float64)
    LQL = L @ np.atleast_2d(np.asarray(sde.Q, np.float64)) @ L.T
    return np.max(np.abs(F @ P0 + P0 @ F.T + LQL)), 1e-8 * max(1.0, float(np.max(np.abs(LQL))))


def matern_closed_forms(name, s2, ell, unit=None):
    """(lam, N1, N2, Pinf, H) of a single Matern kernel at variance s2 and lengthscale ell, lam = sqrt(2 nu) / l, as rows of
    entries (None: a zero matrix).  s2, ell are scalars (one setting) or (B,) arrays (the rows of a batch: every entry is
    then a scalar or a (B,) array).
      Matern-1/2:  F = -lam, Pinf = s2, H = 1;
      Matern-3/2:  the companion form itself (matern32.py:10-28): N = [[lam, 1], [-lam^2, -lam]], N^2 = 0,
                   Pinf = diag(s2, lam^2 s2), H = (1, 0);
      Matern-5/2:  balanced (matern52.py): the balancing iteration commutes with the lengthscale's time scaling, so
                   F = lam F1, Pinf = s2 P1, H = H1 with `unit` = (P1, H1, N, N^2 / 2) the SDE at lam = 1, s2 = 1."""
    if name == "Matern12":
        return 1.0 / ell, None, None, [[s2]], [[1.0]]
    if name == "Matern32":
        lam = np.sqrt(3.0) / ell
        return lam, [[lam, 1.0], [-lam * lam, -lam]], None, [[s2, 0.0], [0.0, lam * lam * s2]], [[1.0, 0.0]]
    lam = np.sqrt(5.0) / ell
    scaled = np.multiply.outer                  # (d, d) entries first, the batch axis (if any) last
    return lam, scaled(unit[2], lam), scaled(unit[3], lam * lam), scaled(unit[0], s2), unit[1]


class ModelForms:
    """_param_key, _device_forms and what they are made of (the model's memos: _key_memo, _struct_memo, _forms_memo,
    _packed_memo, _rbf_ref, _matern52_unit, _matern_fast)."""

    def _param_key(self):
        """The kernel's hyper-parameters as a tuple (the memo key of _device_forms: an evaluation repeated at the same
        setting -- predict_f after the objective, a benchmark loop -- does not rebuild the SDE): the float value of
        every variance / lengthscales / period leaf WHATEVER its type (int, numpy scalar, 0-d array), and what else
        shapes the SDE (order, balancing sweeps, the class of every node).  The memo keeps a reference to the kernel it
        was made for and is compared by identity (`is`), so a new kernel object never finds an old one's forms."""
        quick = getattr(self, "_key_memo", None)
        tree = _tree_ids(self.kernel)   # (a part swapped in place -- `kernel.kernels[0] = ...` -- assigns no attribute)
        if (quick is not None and quick[0] == Kernel._version and quick[1] is self.kernel
                and quick[2] == config.NUMBER_OF_BALANCING_STEPS and quick[4] == tree):
            return quick[3]             # no kernel attribute has been assigned since the key was built
        version = Kernel._version
        struct = getattr(self, "_struct_memo", None)
        if struct is None or struct[0] != Kernel._struct_version or struct[1] is not self.kernel or struct[4] != tree:
            def shape_of(k):
                sub = tuple(shape_of(x) for x in getattr(k, "kernels", ()))
                base = getattr(k, "base_kernel", None)
                return (type(k).__name__, getattr(k, "_order", None), getattr(k, "_balancing_iter", None), sub,
                        None if base is None else type(base).__name__)

            struct = self._struct_memo = (Kernel._struct_version, self.kernel, leaf_parameters(self.kernel), shape_of(self.kernel), tree)
        vals = tuple([float(o.__dict__[n]) for o, n in struct[2]])
        key = (struct[3], config.NUMBER_OF_BALANCING_STEPS) + vals
        self._key_memo = (version, self.kernel, config.NUMBER_OF_BALANCING_STEPS, key, tree)
        return key

    def _device_forms(self):
        key = self._param_key()
        memo = getattr(self, "_forms_memo", None)
        if memo is not None and memo[2] is self.kernel and memo[0] == key:
            return memo[1]
        out = self._device_forms_uncached()
        self._forms_memo = (key, out, self.kernel)
        return out

    def _fused_form(self):
        return self._device_forms()[0]

    def _lti_form(self):
        return self._device_forms()[1]

    def _packed_fused(self, fused):
        """The fused model as the contiguous arrays the series calls take, memoised with the forms."""
        memo = getattr(self, "_packed_memo", None)
        if memo is not None and memo[0] is fused:
            return memo[1]
        sde, form = fused
        d = form[1].shape[0]
        pb = getattr(self, "_pack_buffer", None)
        if pb is None or pb.d != d:
            pb = self._pack_buffer = _backend.PackBuffer(d)
        packed = pb.pack(form, sde.P0, sde.H)       # (views into the model's own buffer: valid until the next setting)
        self._packed_memo = (fused, packed)
        return packed

    def _matern_forms(self):
        """(sde-like, (lam, N1, N2)) of a SINGLE Matern-1/2, -3/2 or -5/2 kernel without building its SDE
        (matern_closed_forms): what a new hyper-parameter setting costs on the host in an optimiser loop (get_sde +
        stationarity check + nilpotent form: ~55 us for Matern-3/2, ~130 us for Matern-5/2 with its balancing sweep and
        Lyapunov solve) becomes a few scalar operations.  The Matern-5/2 unit SDE is built ONCE per model by get_sde() and
        the scaled form checked against get_sde() at the first setting it is used for (1e-10); a kernel for which that
        check fails keeps the general path.  None for anything else."""
        k = self.kernel
        name = type(k).__name__
        if name not in _MATERN_DIMS or getattr(k, "kernels", None):
            return None
        if getattr(self, "_matern_fast", None) is False:
            return None
        s2, ell = float(k.variance), float(k.lengthscales)
        if not (s2 > 0.0 and ell > 0.0):
            return None
        if name != "Matern52":
            lam, N1, _, Pinf, H = matern_closed_forms(name, s2, ell)
            d = len(Pinf)
            return (SimpleNamespace(P0=np.array(Pinf), H=np.array(H)),
                    (lam, np.zeros((d, d)) if N1 is None else np.array(N1), np.zeros((d, d))))
        ukey = (type(k), getattr(k, "_balancing_iter", None), config.NUMBER_OF_BALANCING_STEPS)
        unit = getattr(self, "_matern52_unit", None)
        if unit is None:
            # (shared by every model of the process: a model built per evaluation -- the reference's speed protocol -- would
            # otherwise balance and solve the unit SDE once per call)
            unit = _MATERN52_UNITS.get(ukey)
        if unit is None:
            sde1 = type(k)(1.0, np.sqrt(5.0), **({"balancing_iter": k._balancing_iter} if hasattr(k, "_balancing_iter") else {})).get_sde()
            form1 = _backend.nilpotent_form(sde1.F)
            if form1 is None or abs(form1[0] - 1.0) > 1e-12:
                self._matern_fast = False
                return None
            unit = _MATERN52_UNITS[ukey] = (np.asarray(sde1.P0, np.float64), np.asarray(sde1.H, np.float64).reshape(1, -1),
                                            np.asarray(form1[1], np.float64), np.asarray(form1[2], np.float64))
        self._matern52_unit = unit
        lam, N1, N2, Pinf, H = matern_closed_forms(name, s2, ell, unit)
        out = (SimpleNamespace(P0=Pinf, H=H), (lam, N1, N2))
        if getattr(self, "_matern_fast", None) is None:
            self._matern_fast = _MATERN52_CHECKED.get(ukey)
        if getattr(self, "_matern_fast", None) is None:            # first use in the process: against the kernel's own get_sde()
            sde = k.get_sde()
            form = _backend.nilpotent_form(sde.F)
            close = lambda a, b: np.max(np.abs(np.asarray(a) - np.asarray(b))) <= 1e-10 * (1.0 + np.max(np.abs(np.asarray(b))))
            self._matern_fast = bool(form is not None and close(out[1][0], form[0]) and close(out[1][1], form[1])
                                     and close(out[1][2], form[2]) and close(out[0].P0, sde.P0)
                                     and close(out[0].H, np.asarray(sde.H).reshape(1, -1)))
            _MATERN52_CHECKED[ukey] = self._matern_fast
            if not self._matern_fast:
                return None
        return out

    def _matern_table(self, thetas, params):
        """The (B, 1 + 3 d^2 + d + 1) table [lam | N1 | N2 | Pinf | H | R] of a SINGLE Matern-1/2, -3/2 or -5/2 kernel at the B
        rows (variance, lengthscales, noise variance) of `thetas`, built with array operations from matern_closed_forms:
        no parameter is assigned and no SDE built per row (the row-by-row path costs ~12 us per setting, and its search for
        a setting with the same lengthscale grows with B^2: 44 ms of a 45 ms call at B = 1000).  None where
        _matern_forms() does not apply or a row is not positive."""
        if self._matern_forms() is None or not np.all(thetas > 0.0):
            return None
        if [n for _, n in params] != ["variance", "lengthscales", "noise_variance"]:
            return None
        name = type(self.kernel).__name__
        d = _MATERN_DIMS[name]
        dd = d * d
        table = np.zeros((thetas.shape[0], 1 + 3 * dd + d + 1))
        lam, *blocks = matern_closed_forms(name, thetas[:, 0], thetas[:, 1], getattr(self, "_matern52_unit", None))
        at = 1
        for rows in blocks:                         # N1, N2, Pinf (d, d), H (1, d)
            for i, row in enumerate(() if rows is None else rows):
                for j, v in enumerate(row):
                    table[:, at + i * d + j] = v
            at += dd
        table[:, 0], table[:, -1] = lam, thetas[:, 2]
        return table

    def _rbf_scaled_sde(self):
        """A single RBF kernel near a setting whose SDE is already built: the lengthscale is a scaling of time and the
        variance a scaling of Pinf, so the model at (s2, l) is the reference one at (s2_0, l_0) with F l_0 / l and
        Pinf s2 / s2_0 -- the same likelihood as get_sde()'s realisation gives, to rounding (they differ by a diagonal
        similarity where the balancing sweeps have not converged; tests/test_gpu_lti.py) -- without the 0.2 - 0.4 ms of
        get_sde() (polynomial roots, balancing, Lyapunov solve at d = 6) per step of an optimiser.  The reference setting
        is renewed whenever the lengthscale has drifted by more than 25 % from it.  None for other kernels."""
        k = self.kernel
        if not isinstance(k, RBF) or getattr(k, "kernels", None):
            return None
        s2, ell = float(k.variance), float(k.lengthscales)
        if not (s2 > 0.0 and ell > 0.0):
            return None
        ref = getattr(self, "_rbf_ref", None)
        tag = (getattr(k, "_order", None), getattr(k, "_balancing_iter", None))
        if ref is not None and (ref[6] is not k or ref[5] != tag):
            ref = None                              # another kernel object (or order / balancing) than the reference's
        if ref is None or not (0.8 <= ell / ref[1] <= 1.25):
            sde = k.get_sde()
            F, P0 = np.asarray(sde.F, np.float64), np.asarray(sde.P0, np.float64)
            if not (_backend.LTI_DIM_MIN <= F.shape[0] <= _backend.LTI_DIM_MAX):
                return None
            residual, bound = stationarity_residual(sde, F, P0)
            if residual > bound:
                return None
            ref = self._rbf_ref = (s2, ell, F, P0, np.asarray(sde.H, np.float64), tag, k)
        return SimpleNamespace(F=ref[2] * (ref[1] / ell), P0=ref[3] * (s2 / ref[0]), H=ref[4])

    def _device_forms_uncached(self):
        """(fused, lti) from ONE get_sde() (for composite kernels that call is the host cost of an evaluation); both need
        parallel=True and a stationary P0.  The general-LTI path computes in fp64; a float32 model hands over its times and
        observations widened (N scalars each) and gets results rounded to float32 -- less traffic and better arithmetic
        than fp32 (N, d, d) arrays."""
        if not self.parallel:
            return None, None
        fast = self._matern_forms()
        if fast is not None:
            return fast, None
        scaled = self._rbf_scaled_sde()
        if scaled is not None:
            return None, scaled
        sde = self.kernel.get_sde()
        F, P0 = np.asarray(sde.F, np.float64), np.asarray(sde.P0, np.float64)
        residual, bound = stationarity_residual(sde, F, P0)
        if residual > bound:
            return None, None
        form = _backend.nilpotent_form(sde.F)
        if form is not None:
            return (sde, form), None
        if _backend.LTI_DIM_MIN <= F.shape[0] <= _backend.LTI_DIM_MAX:
            return None, sde
        return None, None
