"""Data and references of tests/test_gpu_batch_geometries.py: B hyper-parameter settings over one series.  No reference is a
device call: het_refs.ss_het with s = 0 is the scalar-noise numpy Kalman filter + RTS smoother, oracle/np_grad.py the numpy
reverse sweep, het_refs.workgroup_forgetting the size of the workgroup totals.  Everything is computed once per (kernel,
setting, shape) and handed out read-only."""
import functools

import numpy as np

from het_refs import merged, queries, spaced_series, ss_het, workgroup_forgetting
from oracle import np_grad as G
from oracle import np_oracle as O

KNAMES = ("m12", "m32", "m52")
LANES = 256
K = 50
START = 0.1         # added to the times of het_refs.spaced_series (case())
# (variance, lengthscale, R).  The last row is this suite's own: on the 2e-4 grid 256 steps span 51 of its lengthscales, so
# its totals forget even where a workgroup holds one step per lane (P3), where the (1, 0.005, 0.1) row does not for Matern-3/2
# and -5/2 (log2 max|A| about -72 and -44, measured on the CPU); dt / lengthscale is 0.2 there, 50 on the 0.05 grid.
SETTINGS = ((1.0, 0.5, 0.1), (1.3, 0.7, 0.2), (0.9, 0.1, 0.12), (2.5, 0.05, 0.03), (1.0, 0.005, 0.1), (0.7, 0.001, 0.15))
M12_EXTRA = (0.4, 2.5, 0.5)
# the row whose interior workgroup totals remember on the 2e-4 grid, and the one whose totals forget at every shape
REMEMBERER = {"m12": M12_EXTRA, "m32": SETTINGS[0], "m52": SETTINGS[0]}
FORGETTER = SETTINGS[5]
# the four settings the AUTO shapes cycle through: the rememberer first, a forgetter last
AUTO_SETTINGS = {"m12": (M12_EXTRA, SETTINGS[0], SETTINGS[2], SETTINGS[3]),
                 "m32": (SETTINGS[0], SETTINGS[1], SETTINGS[2], SETTINGS[4]),
                 "m52": (SETTINGS[0], SETTINGS[1], SETTINGS[2], SETTINGS[4])}
AUTO_FORGETTER = {"m12": SETTINGS[3], "m32": SETTINGS[4], "m52": SETTINGS[4]}


def settings(kname):
    return SETTINGS + ((M12_EXTRA,) if kname == "m12" else ())


def _dense_block(n, first, last):
    sp = np.full(n, 0.05)
    sp[first:last] = 2e-4
    return sp


# name -> (N, pgps_set_chunk, spacing, K, steps per lane, workgroups of the N-step and of the (N + K)-step series)
SHAPES = {"P1": (2600, 4, 2e-4, K, 4, 3, 3), "P2": (4696, 8, 2e-4, K, 8, 3, 3), "P3": (5000, 1, 2e-4, K, 1, 20, 20),
          "P4": (2600, 3, 2e-4, K, 3, 4, 4), "P5": (9000, 16, 2e-4, K, 16, 3, 3),
          "P6": (6744, 8, lambda n: _dense_block(n, 2048, 4096), K, 8, 4, 4), "P7": (5000, 0, 0.05, K, 4, 5, 5),
          # the automatic rule's own 16 and 8 steps per lane (B = 512 and B = 256): one series
          "AUTO": (7680, 0, 2e-4, 512, None, None, None),
          # form 1 at 80 steps per lane, and a series just above kBatchOneMax (no reference at that size)
          "LONG": (20000, 0, lambda n: _dense_block(n, 0, 4096), 480, None, None, None),
          "OVER": (65500, 0, 0.05, 50, None, None, None)}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(shape):
    """(t, y, tq) of a shape: computed once, read-only."""
    n, _, spacing, k = SHAPES[shape][:4]
    t, y, _ = spaced_series(n, spacing(n) if callable(spacing) else spacing)
    # spaced_series starts at 0.05 + one step and het_refs.queries puts a query 0.07 before the first training time: on the
    # 2e-4 grid that query would lie BEFORE the start time t0 = 0 of the call, a first step of negative length (at a
    # lengthscale of 0.5 the device and the reference extrapolate it alike; at 0.005 exp(-F dt) is 10^4 and means nothing)
    t += START
    if shape == "P1":
        y[1020:1030] = np.nan
    return _frozen(t, y, queries(t, k))


@functools.lru_cache(maxsize=None)
def sde(kname, setting):
    import pssgp.kernels as Kn
    cls = {"m12": Kn.Matern12, "m32": Kn.Matern32, "m52": Kn.Matern52}[kname]
    return cls(variance=setting[0], lengthscales=setting[1]).get_sde()


def _series(shape, with_queries, shift):
    """(t, y, R-free tq) of the series a call filters, the times moved by `shift` (a start time t0 = -shift)"""
    t, y, tq = case(shape)
    return t + shift, y, (tq + shift if with_queries else None)


@functools.lru_cache(maxsize=None)
def _ssm(kname, setting, shape, with_queries, shift):
    t, y, tq = _series(shape, with_queries, shift)
    tm = merged(t, y, np.zeros(t.size), tq)[0] if with_queries else t
    s = sde(kname, setting)
    with np.errstate(over="ignore", invalid="ignore"):        # (the long steps overflow there: replaced below)
        P0, Fs, Qs, H, Rm = O.get_ssm(s, tm, 1.0)
    # O.get_ssm takes Q_k from expm(dt [[F, L Q L^T], [0, -F^T]]) as the reference does; the -F^T block grows as
    # exp(+lam dt), and from lam dt of a few tens on -- the 0.11 to the query after the series at a lengthscale of 0.005, every
    # step of the 0.05 grid at 0.001 -- Q_k is lost to rounding (Matern-5/2 at (0.7, 0.001, 0.15), P1, against the dense GP:
    # variance off by 0.3, ll by 2.4e-6).  These kernels are stationary, so Q_k = Pinf - F_k Pinf F_k^T exactly, which has no
    # cancellation once F_k has decayed: that form is taken from lam dt = 1 on (there the 2 d x 2 d exponential has grown by
    # e at most, and 1 - e^-2 of Pinf is left in Q_k).  With it ss_het agrees with the dense GP to 1e-12 at every setting (CPU).
    lam = float(np.max(np.abs(np.linalg.eigvals(np.asarray(s.F, np.float64)))))
    long_steps = np.diff(np.concatenate([[0.0], tm])) * lam > 1.0
    Qs = Qs.copy()
    Qs[long_steps] = P0 - Fs[long_steps] @ P0 @ Fs[long_steps].transpose(0, 2, 1)
    return P0, Fs, Qs, H, Rm


@functools.lru_cache(maxsize=None)
def predict_ref(kname, setting, shape, shift=0.0):
    """(ll, mean, var) at the shape's queries: numpy Kalman filter + RTS smoother over the merged series"""
    t, y, tq = _series(shape, True, shift)
    ll, mean, var = ss_het(sde(kname, setting), t, y, setting[2], np.zeros(t.size), tq, ssm=_ssm(kname, setting, shape, True, shift))
    return (ll,) + _frozen(mean, var)


@functools.lru_cache(maxsize=None)
def grad_ref(kname, setting, shape, shift=0.0):
    """(ll, Abar, Ubar, Hbar, Rbar): the numpy reverse sweep"""
    t, y, _ = _series(shape, False, shift)
    s = sde(kname, setting)
    ll, Abar, Ubar, Hbar, Rbar = G.ll_grad_stats(s.F, s.P0, s.H, setting[2], t, y)
    return (ll,) + _frozen(Abar, Ubar, Hbar) + (Rbar,)


@functools.lru_cache(maxsize=None)
def forgetting(kname, setting, shape, with_queries, steps_per_lane):
    """het_refs.workgroup_forgetting of the series a call filters at workgroups of 256 x steps_per_lane steps: (workgroups, 2)
    log2 max|A|, log2 max|E|"""
    t, y, tq = _series(shape, with_queries, 0.0)
    Rk = np.full(t.size, setting[2])
    if with_queries:
        t, y, Rk, _ = merged(t, y, Rk, tq)
    return _frozen(workgroup_forgetting(sde(kname, setting), t, y, Rk, LANES * steps_per_lane,
                                        ssm=_ssm(kname, setting, shape, with_queries, 0.0)))[0]
