"""Data and references shared by test_gpu_panel_profile.py and test_panel_profile_host.py.  Nothing here is the code under test:
the records come from panel_trend_refs.np_gram (the numpy multi-column filter) and the solutions from
panel_trend_refs.gls_from_gram (numpy's dense inverse of the unit-diagonal A)."""
import functools

import numpy as np

import panel_trend_refs as T
from het_refs import LOG2PI, MATERNS, R

LENGTHS = (257, 12, 700, 37, 256, 16, 255)      # every series has more observed rows than basis functions
BASIS_C = {"constant": 2, "linear": 3, "cubic": 5}
EPS = float(np.finfo(np.float64).eps)


def theta_rows(S):
    """Per-series thetas in the order of trainable_parameters(): variance 1 + 0.1 i, lengthscale 0.5 (1 + 0.05 i), noise R (1 + 0.1 i)."""
    i = np.arange(S, dtype=np.float64)
    return np.stack([1.0 + 0.1 * i, 0.5 * (1.0 + 0.05 * i), R * (1.0 + 0.1 * i)], axis=1)


def kernel_at(kname, theta=None):
    import pssgp.kernels as Kn
    variance, ell = (1.0, 0.5) if theta is None else (float(theta[0]), float(theta[1]))
    return getattr(Kn, MATERNS[kname][0])(variance=variance, lengthscales=ell)


def columns_of(i, basis=None, C=None, lengths=LENGTHS):
    t, y, _ = T.panel(lengths)[i]
    return T.columns(t, y, T.design(basis, t)) if basis is not None else T.wide_columns(t, y, C)


@functools.lru_cache(maxsize=None)
def ref_solution(kname, i, het, basis=None, C=None, own_theta=False, lengths=LENGTHS):
    """(record [G | logdet | n_obs] (C C + 2,), beta, cov, profile, flat, cond) of series i from the reference alone, AFTER
    panel_trend_refs.well_posed holds on the reference record.  own_theta: at row i of theta_rows()."""
    t, y, s = T.panel(lengths)[i]
    if own_theta:
        th = theta_rows(len(lengths))[i]
        G, logdet, n_obs = T.np_gram(kernel_at(kname, th).get_sde(), t, columns_of(i, basis, C, lengths), float(th[2]), s if het else None)
    else:
        G, logdet, n_obs = T.ref_gram(kname, lengths, i, het, basis, C)
    cond = T.well_posed(G, logdet, n_obs, (kname, i, het, basis, C, own_theta))
    rec = np.concatenate([np.asarray(G, np.float64).reshape(-1), [logdet, float(n_obs)]])
    rec.setflags(write=False)
    if G.shape[0] == 1:
        return rec, np.zeros(0), np.zeros((0, 0)), -0.5 * (n_obs * LOG2PI + logdet + float(G[0, 0])), None, cond
    beta, cov, profile, flat, _, _ = T.gls_from_gram(G, logdet, n_obs)
    return rec, beta, cov, profile, flat, cond


def solve_bounds(rec, C, cond):
    """(bound, scale of profile, scale of flat without |logdet_A|): 64 p cond eps, the forward bound of a Cholesky solve with
    the project's own constant (_chol_design's 64 p eps), and what the two log-likelihoods are measured against."""
    p = C - 1
    n_obs, logdet, g_yy = rec[C * C + 1], rec[C * C], rec[0]
    scale = abs(n_obs * LOG2PI) + abs(logdet) + g_yy
    return 64.0 * p * cond * EPS, scale, scale + p * LOG2PI
