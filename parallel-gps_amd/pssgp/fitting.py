"""Per-series hyper-parameter fits: the control rule of csrc/pgps_fit.h in numpy, for S searches in lock
step.

The header is the definition; `bfgs_box` follows it operation by operation (every sum in index order, every product rounded
as written), so one search here and fit_search there visit the same iterates (tests/test_fit_ctl_host.py holds them
together to 1e-12).  StateSpaceGPPanel.fit_each(in_kernel=False) runs it over log_likelihoods_and_grads, one device call per
lock step; it also serves what leaves the launch (series above the panel's step limit).
"""
from collections import namedtuple

import numpy as np

FIT_MAX_HALVINGS = 20           # kFitMaxHalvings
FIT_MAX_ITER_CAP = 200          # kFitMaxIterCap
FIT_ARMIJO = 1e-4               # kFitArmijo
FIT_CURVATURE = 1e-10           # kFitCurvature

STATUS_CONVERGED = 0            # max |projected gradient| <= gtol
STATUS_MAX_ITER = 1             # max_iter iterations made
STATUS_LINE_SEARCH = 2          # no trial was accepted along the steepest descent direction
STATUS_NOT_FINITE = 3           # f or g not finite at the start
STATUS_NAMES = {STATUS_CONVERGED: "converged", STATUS_MAX_ITER: "max_iter", STATUS_LINE_SEARCH: "line_search",
                STATUS_NOT_FINITE: "not_finite"}

BoxResult = namedtuple("BoxResult", "x f f0 iterations evaluations status grad_norm")
PanelFit = namedtuple("PanelFit", "thetas log_likelihoods start_log_likelihoods iterations evaluations status grad_norm")


def check_controls(gtol, max_iter):
    """fit_gtol_valid, fit_max_iter_valid."""
    if not (np.isfinite(gtol) and gtol >= 0.0):
        raise ValueError(f"gtol must be finite and >= 0, got {gtol}")
    if int(max_iter) != max_iter or not 1 <= int(max_iter) <= FIT_MAX_ITER_CAP:
        raise ValueError(f"max_iter must be an integer in 1 .. {FIT_MAX_ITER_CAP}, got {max_iter}")


def _dot(a, b):
    acc = a[:, 0] * b[:, 0]
    for j in range(1, a.shape[1]):
        acc = acc + a[:, j] * b[:, j]
    return acc


def _matvec(H, v):
    """(S, P): row i of H[s] times v[s], summed in index order."""
    acc = H[:, :, 0] * v[:, 0:1]
    for j in range(1, v.shape[1]):
        acc = acc + H[:, :, j] * v[:, j:j + 1]
    return acc


def _finite(f, g):
    return np.isfinite(f) & np.all(np.isfinite(g), axis=1)


def _project(x, g, lo, hi):
    pinned = ((x <= lo) & (g > 0.0)) | ((x >= hi) & (g < 0.0))
    q = np.where(pinned, 0.0, g)
    return q, np.max(np.abs(q), axis=1)


def bfgs_box(evaluate, x0, lo, hi, free, gtol=1e-6, max_iter=100):
    """fit_search of csrc/pgps_fit.h for S searches in lock step: minimise f over lo <= x <= hi from x0 (S, P) each.
    evaluate(X (S, P)) -> (f (S,), g (S, P)) is any callable; it is asked once per lock step with one row per search (the row
    of a search that needs no evaluation in that step is its current iterate, and what comes back for it is not looked at).
    free (P,) flags: a coordinate that is not free must have g = 0 (the flags only matter to the rule that a change of the
    set of FREE coordinates on a bound resets the matrix).  Returns a BoxResult of (S, ...) arrays."""
    check_controls(gtol, max_iter)
    x0 = np.array(x0, np.float64, ndmin=2)
    S, P = x0.shape
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (S, P)), np.broadcast_to(np.asarray(hi, np.float64), (S, P))
    free = np.broadcast_to(np.asarray(free, bool), (P,))
    eye = np.broadcast_to(np.eye(P), (S, P, P))

    x = np.clip(x0, lo, hi)
    f, g = evaluate(x.copy())
    f, g = np.array(f, np.float64).reshape(S), np.array(g, np.float64).reshape(S, P)
    f0 = f.copy()
    evaluations = np.ones(S, np.int64)
    iterations = np.zeros(S, np.int64)
    status = np.where(_finite(f, g), -1, STATUS_NOT_FINITE).astype(np.int64)
    gnorm = np.full(S, np.nan)
    H = eye.copy()
    fresh = np.ones(S, bool)
    q, p = np.zeros((S, P)), np.zeros((S, P))
    qmax, alpha = np.zeros(S), np.ones(S)
    trial = np.zeros(S, np.int64)           # trials made in the current search
    pending = np.zeros(S, bool)             # a trial waits for its evaluation
    xt, s, gs = x.copy(), np.zeros((S, P)), np.zeros(S)

    def direction(rows):
        """Step 2 for `rows` (a mask): p, alpha; no trial made yet."""
        fr = rows & fresh
        bf = rows & ~fresh
        if fr.any():
            p[fr] = -q[fr]
            alpha[fr] = np.minimum(1.0, 1.0 / qmax[fr])
        if bf.any():
            p[bf] = -_matvec(H[bf], q[bf])
            alpha[bf] = 1.0
        trial[rows] = 0

    def begin(rows):
        """Step 1 for `rows`: converged, out of iterations, or a new direction."""
        if not rows.any():
            return
        qr, qm = _project(x[rows], g[rows], lo[rows], hi[rows])
        q[rows], qmax[rows] = qr, qm
        gnorm[rows] = qm
        idx = np.flatnonzero(rows)
        conv = qm <= gtol
        status[idx[conv]] = STATUS_CONVERGED
        late = ~conv & (iterations[idx] >= max_iter)
        status[idx[late]] = STATUS_MAX_ITER
        go = np.zeros(S, bool)
        go[idx[~conv & ~late]] = True
        direction(go)

    begin(status < 0)
    while np.any(status < 0):
        # step 3, up to the evaluation: propose until every running search has a descent trial pending, or has ended
        while True:
            todo = (status < 0) & ~pending
            if not todo.any():
                break
            spent = todo & (trial > FIT_MAX_HALVINGS)
            if spent.any():                                     # step 4
                status[spent & fresh] = STATUS_LINE_SEARCH
                again = spent & ~fresh
                H[again] = eye[again]
                fresh[again] = True
                direction(again)
                todo = (status < 0) & ~pending
                if not todo.any():
                    break
            xt[todo] = np.clip(x[todo] + alpha[todo, None] * p[todo], lo[todo], hi[todo])
            s[todo] = xt[todo] - x[todo]
            gs[todo] = _dot(g[todo], s[todo])
            ok = todo & (gs < 0.0)
            pending |= ok
            trial[todo] += 1
            alpha[todo] *= 0.5
        run = pending & (status < 0)
        if not run.any():
            break
        X = np.where(run[:, None], xt, x)
        ft, gt = evaluate(X.copy())
        ft, gt = np.array(ft, np.float64).reshape(S), np.array(gt, np.float64).reshape(S, P)
        evaluations[run] += 1
        pending[:] = False
        acc = run & _finite(ft, gt) & (ft <= f + FIT_ARMIJO * gs)
        if acc.any():                                           # step 5
            sa, xa = s[acc], xt[acc]
            was = free[None, :] & ((x[acc] <= lo[acc]) | (x[acc] >= hi[acc]))
            now = free[None, :] & ((xa <= lo[acc]) | (xa >= hi[acc]))
            changed = np.any(was != now, axis=1)                # the set of free coordinates on a bound
            y = np.where(now & (sa == 0.0), 0.0, gt[acc] - g[acc])
            sy, ss, yy = _dot(sa, y), _dot(sa, sa), _dot(y, y)
            with np.errstate(invalid="ignore"):
                reset = changed | ~(sy > FIT_CURVATURE * (np.sqrt(ss) * np.sqrt(yy)))
            Ha, fa = H[acc], fresh[acc]
            first = fa & ~reset
            with np.errstate(divide="ignore", invalid="ignore"):
                Ha[first] = (sy[first] / yy[first])[:, None, None] * eye[:int(first.sum())]
                Hy = _matvec(Ha, y)
                yHy = _dot(y, Hy)
                c1, c2 = (sy + yHy) / (sy * sy), 1.0 / sy
                upd = (Ha + c1[:, None, None] * (sa[:, :, None] * sa[:, None, :])) \
                    - c2[:, None, None] * (Hy[:, :, None] * sa[:, None, :] + sa[:, :, None] * Hy[:, None, :])
            Ha = np.where(reset[:, None, None], eye[:Ha.shape[0]], upd)
            H[acc], fresh[acc] = Ha, reset
            x[acc], f[acc], g[acc] = xa, ft[acc], gt[acc]
            iterations[acc] += 1
            begin(acc)
    return BoxResult(x, f, f0, iterations, evaluations, status, gnorm)


# -- x = log theta and back (fit_theta of csrc/pgps_fit_model.h) -------------------------------------------------------------------
def log_box(theta0, lo, hi, free):
    """(x0, xlo, xhi) (S, P) of a start and a box given in theta: logs at the free coordinates, 0 elsewhere (a coordinate that
    is not free is never taken through log / exp)."""
    free = np.asarray(free, bool)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return tuple(np.where(free, np.log(np.where(free, a, 1.0)), 0.0) for a in (theta0, lo, hi))


def thetas_of(x, x0, xlo, xhi, theta0, lo, hi, free):
    """theta (S, P) at x: exp(x) at a free coordinate -- but the start, a lower or an upper bound bit for bit where x still
    equals the value it was given for them -- and theta0 at the others."""
    free = np.asarray(free, bool)[None, :]
    th = np.exp(x)
    th = np.where(x == xhi, hi, th)
    th = np.where(x == xlo, lo, th)
    th = np.where(x == x0, np.clip(theta0, lo, hi), th)
    return np.where(free, th, theta0)
