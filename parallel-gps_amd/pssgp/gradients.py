"""Hyper-parameter gradients of StateSpaceGP: the models and derivatives the device passes take,
and the host half of the adjoint passes.  The pure parts are functions (the Matern contraction, the `wrt` mask); what reads
the model's memos is `ModelGradients`, a mixin of StateSpaceGP -- log_likelihood_and_grad itself, which routes between these,
is the model's.
"""
import numpy as np

from . import _backend, config
from .kernels.sde_grads import leaf_parameters, sde_with_grads
from .forms import stationarity_residual


class _StructureChanged(Exception):
    """_grad_rows_composite: the block partition of the drift is not the same at the perturbed parameters."""


def mask_wrt(g, wrt):
    """`wrt`: only these parameter indices (the last axis of g); one pass gives every direction, the ones not asked for read 0."""
    if wrt is None:
        return g
    keep = np.zeros(np.shape(g)[-1], bool)
    keep[[int(i) for i in wrt]] = True
    return np.where(keep, g, 0.0)


def matern_contract(Abar, Ubar, Rbar, F, PH, names, lengthscales, variances):
    """The host half of every adjoint gradient of a single Matern kernel: the lengthscale scales time (dF = -F / l) and the
    variance Pinf (dPinf = Pinf / s2), so with the device's adjoints Abar (flat d^2), Ubar (d) and Rbar, F = N1 - lam I (flat)
    and PH = Pinf H^T:
        d ll / d l = -<Abar, F> / l,   d ll / d s2 = Ubar . PH / s2,   d ll / d R = Rbar.
    One setting (1-D arguments: flat dot products, a (P,) gradient in the order of `names`) or the B rows of a batch (2-D
    arguments, (B,) lengthscales and variances: row sums, (B, P))."""
    if Abar.ndim == 1:
        aF, uPH, Rbar = float(Abar @ F), float(Ubar @ PH), float(Rbar)
    else:
        aF, uPH = np.sum(Abar * F, axis=1), np.sum(Ubar * PH, axis=1)
    by_name = {"variance": uPH / variances, "lengthscales": -aF / lengthscales, "noise_variance": Rbar}
    cols = [by_name[n] for n in names]
    return np.array(cols) if Abar.ndim == 1 else np.stack(cols, axis=1)


def time_scaled_prepared(kernel, F, P0, H):
    """(F, Pinf, H, derivatives) for the general adjoint pass of a single kernel whose lengthscale scales time (dF = -F / l)
    and whose variance scales Pinf (a Matern kernel from its fused form, RBF from its reference realisation): written down,
    no get_sde() per optimiser step."""
    F, P0 = np.ascontiguousarray(F, np.float64), np.ascontiguousarray(P0, np.float64)
    H = np.ascontiguousarray(np.asarray(H, np.float64).reshape(-1))
    zF, zP, zH = np.zeros_like(F), np.zeros_like(P0), np.zeros((1, H.size))
    rules = {"variance": (zF, P0 / float(kernel.variance), zH), "lengthscales": (-F / float(kernel.lengthscales), zP, zH)}
    return (F, P0, H, [rules[a] for _, a in leaf_parameters(kernel)])


def richardson(central, x0):
    """d/dx at x0 of every entry `central(h)` differences: two central differences, steps h and h / 2, extrapolated (the SDE
    coefficients are low-degree rational functions of the parameters: exact to ~1e-11)."""
    h = 1e-3 * max(abs(x0), 1e-3)
    d1, d2 = central(h), central(0.5 * h)
    return tuple((4.0 * b - a) / 3.0 for a, b in zip(d1, d2))


class ModelGradients:
    """The gradient methods of StateSpaceGP (the model's memos: _fadj_memo, _grads_memo, _contract_memo, _no_composite)."""

    def _grad_blocks_matern(self):
        """_grad_blocks() of a single Matern-1/2, -3/2 or -5/2 kernel in closed form, from the memoised get_sde() of the
        evaluation -- no further SDE construction (four of them per parameter were what a small-N gradient call cost on
        the host).  With lam = sqrt(2 nu) / l and F = -lam I + N:
          variance s2:  Pinf is linear in it, nothing else moves  ->  dPinf = Pinf / s2;
          lengthscale:  dlam = -lam / l.  Matern-3/2 keeps the companion form (matern32.py:10-28: N = [[lam, 1],
            [-lam^2, -lam]], Pinf = diag(s2, lam^2 s2)); Matern-5/2 is balanced (matern52.py: balance_ss + Lyapunov), and
            Osborne's balancing iteration commutes with the time scaling x_i -> lam^i x_i that relates the companion
            forms at two lengthscales, so the balanced drift is lam * (a constant matrix) and Pinf, H do not move:
            dN = N / lam * dlam, dPinf = 0, dH = 0  (checked against the differences: tests/test_model_host.py);
          noise:        R alone.
        None for any other kernel."""
        k = self.kernel
        name = type(k).__name__
        if name not in ("Matern12", "Matern32", "Matern52") or getattr(k, "kernels", None) or not k.variance:
            return None
        fused = self._fused_form() if self.parallel else None
        if fused is None:
            return None
        sde, form = fused
        lam, N = np.float64(form[0]), np.asarray(form[1], np.float64)
        Pinf, H = np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1)
        zN, zP, zH, z = np.zeros_like(N), np.zeros_like(Pinf), np.zeros_like(H), np.float64(0.0)
        dlam = -lam / k.lengthscales
        if name == "Matern32":
            dN = dlam * np.array([[1.0, 0.0], [-2.0 * lam, -1.0]])
            dP = np.diag([0.0, 2.0 * lam * k.variance * dlam])
        else:
            dN, dP = N * (dlam / lam), zP
        blocks = {"variance": (z, zN, Pinf / k.variance, zH, z), "lengthscales": (dlam, dN, dP, zH, z),
                  "noise_variance": (z, zN, zP, zH, np.float64(1.0))}
        return [(lam, N, Pinf, H, np.float64(self.noise_variance))] + [blocks[n] for _, n in self.trainable_parameters()]

    def _grad_blocks(self, closed_form=True):
        """The fused model (lam, N, Pinf, H, R) and its partial derivatives with respect to each
        trainable parameter: closed form for a single Matern kernel; otherwise Richardson-extrapolated central
        differences of get_sde()."""
        closed = self._grad_blocks_matern() if closed_form else None
        if closed is not None:
            return closed

        def block():
            sde = self.kernel.get_sde()
            form = _backend.nilpotent_form(sde.F)
            if form is None:
                raise NotImplementedError("gradients need the closed-form (Matern-family) discretisation")
            return [np.float64(form[0]), np.asarray(form[1], np.float64), np.asarray(sde.P0, np.float64),
                    np.asarray(sde.H, np.float64).reshape(-1), np.float64(self.noise_variance)]

        base = block()
        blocks = [tuple(base)]
        zeros = [np.zeros_like(np.asarray(v, np.float64)) for v in base]
        for owner, name in self.trainable_parameters():
            x0 = getattr(owner, name)
            # two of the three derivatives are known in closed form -- and get_sde() (balancing sweep + Lyapunov solve)
            # is what a small-N gradient call costs on the host: the observation noise enters through R alone, and a
            # single Matern kernel's variance through Pinf alone, linearly (balance_ss leaves F, H independent of q)
            if owner is self and name == "noise_variance":
                blocks.append(tuple(zeros[:4]) + (np.float64(1.0),))
                continue
            if owner is self.kernel and name == "variance" and x0 != 0.0:
                blocks.append((zeros[0], zeros[1], base[2] / x0, zeros[3], np.float64(0.0)))
                continue

            def central(h):
                setattr(owner, name, x0 + h)
                up = block()
                setattr(owner, name, x0 - h)
                dn = block()
                return [(u - v) / (2.0 * h) for u, v in zip(up, dn)]

            try:
                blocks.append(richardson(central, x0))
            finally:
                setattr(owner, name, x0)
        return blocks

    def _grad_rows_composite(self):
        """(rows, block sizes) for pgps_gp_ll_grad_blocks_*: the block-nilpotent model (lam_b, N, Pinf, H, R) of a sum /
        product of Matern kernels and its partial derivatives with respect to each trainable parameter (Richardson
        central differences of get_sde()), or (None, None) when the kernel's drift does not have that form, the state
        dimension is not 2..6, or the partition into blocks changes under the perturbation."""
        def row():
            sde = self.kernel.get_sde()
            F = np.asarray(sde.F, np.float64)
            blocks = _backend.nilpotent_blocks(F)
            if blocks is None:
                return None, None
            Nm = F.copy()
            for lo, n, lam, _ in blocks:
                Nm[lo:lo + n, lo:lo + n] += lam * np.eye(n)
            return ([np.array([b[2] for b in blocks]), Nm, np.asarray(sde.P0, np.float64),
                     np.asarray(sde.H, np.float64).reshape(-1), np.float64(self.noise_variance)],
                    [b[1] for b in blocks])

        base, sizes = row()
        d = None if base is None else base[1].shape[0]
        if base is None or not (2 <= d <= _backend.GRAD_BLOCKS_DIM_MAX) or len(sizes) > _backend.GRAD_BLOCKS_MAX:
            self._no_composite = True          # (a property of the kernel's structure: not asked again)
            return None, None
        rows = [tuple(base)]
        for owner, name in self.trainable_parameters():
            x0 = getattr(owner, name)

            def central(h):
                setattr(owner, name, x0 + h)
                up, su = row()
                setattr(owner, name, x0 - h)
                dn, sd = row()
                if up is None or dn is None or su != sizes or sd != sizes:
                    # (a coupling entry near nilpotent_blocks' threshold: the partition found at x0 +- h differs)
                    raise _StructureChanged()
                return [(u - v) / (2.0 * h) for u, v in zip(up, dn)]

            try:
                rows.append(richardson(central, x0))
            except _StructureChanged:
                return None, None               # the caller differentiates the likelihood itself instead
            finally:
                setattr(owner, name, x0)
        return rows, sizes

    # Matern-5/2 (d = 3, three directions): above the one-launch length the dual-number pass is three launches of kernels
    # three times as heavy as the filter's; the adjoint pass on the general-LTI kernels costs 1.5 likelihoods.  Measured
    # (tools/grad_methods.py, one MI355X): N = 4096 199 -> 117 us, 32 768 186 -> 151 us, 131 072 320 -> 238 us; a tie at
    # 1000; Matern-3/2 (d = 2) is better off on duals at every length (79 vs 102 us at 4096).
    _MATERN52_ADJOINT_FROM = 2048

    def _matern_prepared(self, fused):
        """time_scaled_prepared() of a single Matern kernel from its fused form, F = N1 - lam I."""
        sde_like, (lam, N1, _) = fused
        return time_scaled_prepared(self.kernel, np.asarray(N1, np.float64) - lam * np.eye(N1.shape[0]), sde_like.P0, sde_like.H)

    def _fused_adjoint_pays(self, n):
        """Automatic choice between the dual-number pass and the adjoint pass of the fused path, from measurements on one
        MI355X (tools/grad_methods.py, microseconds per call, dual / adjoint): Matern-5/2 96 / 78 at N = 200, 198 / 102 at
        4096, 592 / 147 at 2^20: always the adjoint; Matern-3/2 51 / 54 at 1000 (one launch each), 77 / 64 at 4096, 186 / 92
        at 2^20: above the one-launch length; Matern-1/2 (two directions, d = 1) 46 / 53: duals."""
        name = type(self.kernel).__name__
        return name == "Matern52" or (name == "Matern32" and n > 2048)

    def _multi_grad_pays(self, n, m):
        """Automatic choice between ONE multi-column adjoint call (host arrays: Y is copied per call) and the column loop (M
        single-column passes over series that are resident from a model's second evaluation on), from one run of
        tools/multi_grad_bench.py on an MI355X (profiles/multi_grad_bench.json; medians in ms, multi / loop).
        N = 4096, M = 2, 3, 4: Matern-1/2 0.100 / 0.073, 0.104 / 0.110, 0.097 / 0.147; Matern-3/2 0.109 / 0.095, 0.112 / 0.142,
        0.110 / 0.190; Matern-5/2 0.144 / 0.169, 0.150 / 0.257, 0.147 / 0.334: from M = 3 (Matern-5/2: from M = 2).
        M = 16, N = 2^15 .. 2^18, 2^20: Matern-3/2 0.27 / 0.77, 0.42 / 0.79, 0.80 / 0.81, 1.69 / 0.91, 6.64 / 1.33; Matern-5/2
        0.32 / 1.41, 0.61 / 1.41, 1.04 / 1.43, 2.25 / 1.64, 7.41 / 2.15: the copy of Y (8 N M bytes per call) overtakes the loop's M
        passes between 2^16 and 2^17 steps for Matern-3/2 and between 2^17 and 2^18 for Matern-5/2, whatever M (both sides
        grow with M): up to the last length measured as a win.  Matern-1/2 was not measured there and takes Matern-3/2's
        bound.  The passes alone (device-resident Y, pgps_gp_ll_grad_multi_dev_f64) win at every point measured."""
        name = type(self.kernel).__name__
        return m >= (2 if name == "Matern52" else 3) and n <= (131072 if name == "Matern52" else 65536)

    def _fused_contraction(self, packed):
        """(F = N1 - lam I flat, Pinf H^T, the gradient's parameter names) of the packed fused model, memoised with it: what
        matern_contract needs besides the device's adjoints."""
        memo = getattr(self, "_fadj_memo", None)
        if memo is None or memo[0] is not packed:
            lam, N1, _, Pinf, H, d = packed
            F = N1.reshape(-1).copy()
            F[::d + 1] -= lam                       # F = N1 - lam I
            self._param_key()
            memo = self._fadj_memo = (packed, F, Pinf @ H, [a for _, a in self._struct_memo[2]] + ["noise_variance"])
        return memo[1:]

    def _fused_adjoint_ll_and_grad(self, fused, wrt=None):
        """(ll, grad) of a single Matern kernel by the adjoint pass on the fused (closed-form discretisation) kernels
        (csrc/pgps_gpadj.hip.h): the device returns the model's adjoints [ll | Abar | Ubar | Hbar | Rbar] from one filter pass
        and one reverse pass over the resident series, matern_contract makes the gradient of them.  None when the series is
        not resident or the library has no such entry point."""
        ser = self._device_series()
        if ser is None or not getattr(ser, "has_gp_adj", False):
            return None
        packed = self._packed_fused(fused)
        d = packed[5]
        F, PH, names = self._fused_contraction(packed)
        out = ser.gp_ll_grad_adj_raw(packed, self.noise_variance)
        dd = d * d
        k = self.kernel
        g = matern_contract(out[1:1 + dd], out[1 + dd:1 + dd + d], out[1 + dd + 2 * d], F, PH, names,
                            float(k.lengthscales), float(k.variance))
        return config.default_float()(out[0]), mask_wrt(g, wrt)

    def _host_adjoint_grad(self, fused, stats, wrt):
        """The gradient from the adjoints (_, Abar (d, d), Ubar, Hbar, Rbar) a host-array adjoint pass of the fused model
        returned (several output columns, per-observation noise): contracted as _fused_adjoint_ll_and_grad contracts them."""
        _, Abar, Ubar, _, Rbar = stats
        F, PH, names = self._fused_contraction(self._packed_fused(fused))
        k = self.kernel
        return mask_wrt(matern_contract(Abar.reshape(-1), Ubar, Rbar, F, PH, names, float(k.lengthscales), float(k.variance)), wrt)

    def _adjoint_prepared(self):
        """(F, Pinf, H, [(dF, dPinf, dH)]) of the kernel at its CURRENT setting for the adjoint pass of the general-LTI device
        path, memoised by the setting; None when the kernel has no derivative rule, the model is not stationary or of a state
        dimension the device path does not cover, or a derivative of the drift does not commute with it (the contraction
        the device makes would not apply)."""
        key = self._param_key()
        memo = getattr(self, "_grads_memo", None)
        if memo is not None and memo[2] is self.kernel and memo[0] == key:
            return memo[1]
        prepared = None
        scaled = self._rbf_scaled_sde()
        if scaled is not None:
            # a single RBF kernel near a setting whose SDE is built (the steps of an optimiser or sampler): the model AND its
            # derivatives are written down from the reference realisation -- no polynomial roots, balancing or Lyapunov solve
            prepared = time_scaled_prepared(self.kernel, scaled.F, scaled.P0, scaled.H)
            sde = None
        else:
            try:
                sde, grads = sde_with_grads(self.kernel)
            except (NotImplementedError, ZeroDivisionError, FloatingPointError):
                sde = None
        if sde is not None:
            F, P0 = np.ascontiguousarray(sde.F, np.float64), np.ascontiguousarray(sde.P0, np.float64)
            H = np.ascontiguousarray(np.asarray(sde.H, np.float64).reshape(-1))
            fmax = max(1.0, float(np.max(np.abs(F))))
            ok = _backend.LTI_DIM_MIN <= F.shape[0] <= _backend.LTI_DIM_MAX and np.all(np.isfinite(F)) and np.all(np.isfinite(P0))
            if ok:
                residual, bound = stationarity_residual(sde, F, P0)
                ok = residual <= bound
            for dF, dP, dH in grads if ok else ():
                if not np.all(np.isfinite(dP)):
                    ok = False
                if not dF.any():
                    continue                    # (most parameters move Pinf or H only: nothing to commute)
                if not np.all(np.isfinite(dF)) or \
                        np.max(np.abs(F @ dF - dF @ F)) > 1e-9 * fmax * max(1.0, float(np.max(np.abs(dF)))):
                    ok = False
            if ok:
                prepared = (F, P0, H, grads)
        self._grads_memo = (key, prepared, self.kernel)
        return prepared

    def _adjoint_ll_and_grad(self, wrt=None, prepared=None):
        """(ll, grad) by the adjoint pass of the general-LTI device path (pgps_lti_ll_grad_f64): the device returns the
        adjoints of the model (F, Pinf, H, R) from one filter pass and one reverse pass, pssgp.kernels.sde_grads the
        model's derivatives in a frozen state basis; exact (no differences), ONE device call, any number of parameters.
        None when the kernel has no derivative rule, a derivative of the drift does not commute with it (the contraction
        the device makes would not apply), or the library lacks the entry point."""
        if prepared is None:                    # (else the caller wrote the model and its derivatives down: Matern family)
            prepared = self._adjoint_prepared()
        if prepared is None:
            return None
        F, P0, H, grads = prepared
        ts, Y = self.data
        ser = self._device_series() if ts.dtype == np.float64 else None
        try:
            if ser is not None and getattr(ser, "has_lti_grad", False):
                stats = ser.lti_ll_grad(F, P0, H, self.noise_variance)
            else:
                stats = _backend.lti_ll_grad(F, P0, H, self.noise_variance, ts.reshape(-1), Y.reshape(-1))
        except _backend.PgpsError as e:
            if getattr(e, "code", None) == _backend.E_UNSUPPORTED_DIM:
                return None
            raise
        except RuntimeError:
            return None
        # contraction <Abar, dF> + Ubar^T dPinf H^T + Hbar . dH per parameter, the identically-zero components skipped (a
        # parameter moves one of F, Pinf, H: one dot product each instead of three products on zeros -- `_backend.
        # contract_grad_stats` is the plain form the tests check this against)
        fast = getattr(self, "_contract_memo", None)
        if fast is None or fast[0] is not grads:
            h = H.reshape(-1)
            rows = [(dF.reshape(-1) if np.any(dF) else None, (np.asarray(dP) @ h) if np.any(dP) else None,
                     np.asarray(dH).reshape(-1) if np.any(dH) else None) for dF, dP, dH in grads]
            fast = self._contract_memo = (grads, rows)
        _, Abar, Ubar, Hbar, Rbar = stats
        Av = Abar.reshape(-1)
        g = np.array([(0.0 if a is None else float(Av @ a)) + (0.0 if u is None else float(Ubar @ u))
                      + (0.0 if hh is None else float(Hbar @ hh)) for a, u, hh in fast[1]] + [float(Rbar)])
        return config.default_float()(stats[0]), mask_wrt(g, wrt)

    def _lti_ll_and_grad(self, rel_step=1e-3, batched=True, wrt=None):
        """Kernels without the closed-form discretisation (RBF, Periodic, sums, products; d <= 16): the gradient by
        Richardson-extrapolated central differences -- 4 P + 1 likelihood evaluations, ALL IN ONE batched device call
        (pgps_lti_ll_batch_*), so its cost is that of one launch set, not of 4 P + 1.  Truncation error O(h^4):
        ~1e-8 relative for these smooth objectives (tests/test_gpu_lti.py checks it against the dense GP's
        gradient); the dual-number pass of the Matern family is exact."""
        params = self.trainable_parameters()
        x0 = np.array([getattr(o, n) for o, n in params], np.float64)
        rows = [x0]
        hs = rel_step * np.maximum(np.abs(x0), 1e-3)
        idx = list(range(len(params))) if wrt is None else [int(i) for i in wrt]   # `wrt`: only these parameters
        for i in idx:
            for mult in (1.0, -1.0, 0.5, -0.5):
                x = x0.copy()
                x[i] += mult * hs[i]
                rows.append(x)
        if batched:
            lls = self.log_likelihood_batch(np.stack(rows))
        else:
            lls = []
            try:
                for row in rows:
                    self._assign(params, row)
                    lls.append(float(self.maximum_log_likelihood_objective()))
            finally:
                self._assign(params, x0)
            lls = np.array(lls)
        grad = np.zeros(len(params))
        for j, i in enumerate(idx):
            up, dn, up2, dn2 = lls[1 + 4 * j:5 + 4 * j]
            d1 = (up - dn) / (2.0 * hs[i])
            d2 = (up2 - dn2) / hs[i]
            grad[i] = (4.0 * d2 - d1) / 3.0
        return float(lls[0]), grad
