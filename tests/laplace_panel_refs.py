"""Data and references of the Laplace-panel tests (test_laplace_panel_host.py, test_gpu_laplace_panel.py; DESIGN.md section
4ab).  None of this is the code under test: the panels are laplace_refs.case's series with the observations drawn anew from a
seed per series (a read from a neighbour's rows moves a result); the references are the loop of single LaplaceStateSpaceGP
models -- the host twin, with the move of every Newton pass recorded -- and laplace_refs.dense_fit."""
import functools
import warnings

import numpy as np

import laplace_refs as LR
from laplace_refs import MATERNS, PARS, matern  # noqa: F401  (re-exported to the tests)

LENGTHS = (257, 1, 700, 37, 256, 2, 255)        # tests/test_gpu_panel.py's: one row, one lane, a full wave, 256 / 257, a ragged last wave
TOL_SEARCH = 1e-8                               # where the search stops: what two fp64 routes agree to
KNAMES = ("m12", "m32", "m52")
LIKELIHOODS = ("bernoulli", "poisson")


def likelihood(lik, par=None):
    from pssgp.likelihoods import Bernoulli, Poisson
    return Bernoulli() if lik == "bernoulli" else Poisson(PARS["poisson"] if par is None else par)


@functools.lru_cache(maxsize=None)
def panel(lik, lengths=LENGTHS):
    """[(t, y)] read-only: series i has the times and missing rows of laplace_refs.case(lik, n_i), observations of seed i."""
    out = []
    for i, n in enumerate(lengths):
        t, y0 = LR.case(lik, n)
        y = LR.observations(lik, np.asarray(t), np.isnan(y0), seed=i)
        t = np.array(t)
        for a in (t, y):
            a.setflags(write=False)
        out.append((t, y))
    return tuple(out)


def recording_model(t, y, kernel, lik_obj, parallel=False, tol=TOL_SEARCH, max_iter=50):
    """A LaplaceStateSpaceGP whose searches append every pass's move to .moves (the closing pass's included)."""
    from pssgp.laplace import LaplaceStateSpaceGP

    class Recording(LaplaceStateSpaceGP):
        def _search(self, start, newton, halve, accept):
            self.moves = []

            def counted():
                s = newton()
                self.moves.append(float(s[4]))
                return s
            return super()._search(start, counted, halve, accept)

    return Recording((np.asarray(t)[:, None], np.asarray(y)[:, None]), kernel, lik_obj, parallel=parallel, tol=tol, max_iter=max_iter)


@functools.lru_cache(maxsize=None)
def twin(kname, lik, i, lengths=LENGTHS, max_iter=50):
    """The host twin on series i of panel(lik, lengths): (fit_mode dict, fit_info, moves of the steps), computed once."""
    t, y = panel(lik, lengths)[i]
    m = recording_model(t, y, matern(kname), likelihood(lik), max_iter=max_iter)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        fit = m.fit_mode()
    for a in fit.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return fit, dict(m.fit_info), tuple(m.moves[:m.fit_info["iterations"]])


@functools.lru_cache(maxsize=None)
def dense(kname, lik, i, lengths=LENGTHS, grad=False):
    t, y = panel(lik, lengths)[i]
    return LR.dense_fit(kname, 1.0, 0.5, t, y, lik, PARS[lik], grad=grad)


def counts_agree(info, ref_info, ref_moves, tol=TOL_SEARCH):
    """The rule on counts: halvings equal; iterations equal, except that a series whose REFERENCE move sequence has an entry
    within [tol / 2, 2 tol] may differ by one."""
    if info["halvings"] != ref_info["halvings"]:
        return False
    near = any(0.5 * tol <= m <= 2.0 * tol for m in ref_moves)
    return abs(info["iterations"] - ref_info["iterations"]) <= (1 if near else 0)


def err(got, want):
    return LR.err(got, want)
