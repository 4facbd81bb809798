"""The control rule of the per-series fit on the host (no GPU): parallel-gps_amd/csrc/pgps_fit.h -- fit_search, the loop
k_gpp_fit runs per workgroup -- and pgps_fit_model.h, compiled with g++ into a stand-alone program (tests/cpu_math/fit_ctl.cpp)
and run.  The program drives fit_search over toy problems (a convex quadratic, a curved valley, a minimum outside the box, NaN
beyond a radius, NaN always, a lying gradient, ...) and checks status, result and the evaluation cap of every search; one build
also runs under the address and undefined-behaviour sanitizers.  pssgp.fitting.bfgs_box, the rule's twin in numpy, is then run
on the same functions and must evaluate the same points in the same order: twin and header are one rule.  The header's Matern
closed forms and contraction are held against pssgp.forms.matern_closed_forms and pssgp.gradients.matern_contract."""
import os
import subprocess

import numpy as np
import pytest

from pssgp import fitting
from pssgp.forms import matern_closed_forms
from pssgp.gradients import matern_contract
from pssgp.kernels import Matern52
from pssgp.model import StateSpaceGP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# -ffp-contract=off: the twin rounds every product, so must the program (a compiler may otherwise fuse a * b + c)
FLAGS = {"O2": ["-O2", "-ffp-contract=off"],
         "sanitized": ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def _build(flags, where):
    exe = str(where / "fit_ctl")
    subprocess.run(["g++"] + FLAGS[flags] + ["-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "parallel-gps_amd", "csrc"),
                                             os.path.join(ROOT, "tests", "cpu_math", "fit_ctl.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build("O2", tmp_path_factory.mktemp("fit_ctl"))


@pytest.mark.parametrize("flags", list(FLAGS), ids=list(FLAGS))
def test_fit_control_rule(flags, tmp_path):
    exe = _build(flags, tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.strip().endswith("fit ok")


# ---- the toy problems of fit_ctl.cpp, product by product in the same order, on (S, 3) rows ------------------------------------
def _cols(X):
    return X[:, 0], X[:, 1], X[:, 2]


def f_quad(X):
    A = ((3.0, 1.0, 0.0), (1.0, 2.0, 0.5), (0.0, 0.5, 1.0))
    b = (1.0, -2.0, 0.5)
    x = _cols(X)
    Ax = [(A[i][0] * x[0] + A[i][1] * x[1]) + A[i][2] * x[2] for i in range(3)]
    f = 0.5 * ((x[0] * Ax[0] + x[1] * Ax[1]) + x[2] * Ax[2]) - ((b[0] * x[0] + b[1] * x[1]) + b[2] * x[2])
    return f, np.stack([Ax[i] - b[i] for i in range(3)], axis=1)


def f_valley(X):
    x0, x1, x2 = _cols(X)
    a, c, e = 1.0 - x0, x1 - x0 * x0, x2 - 0.5
    return (a * a + 10.0 * (c * c)) + e * e, np.stack([-2.0 * a - 40.0 * (c * x0), 20.0 * c, 2.0 * e], axis=1)


def f_outside(X):
    x0, x1, x2 = _cols(X)
    d0, d1, d2 = x0 - 5.0, x1 + 5.0, x2 - 0.3
    return (d0 * d0 + d1 * d1) + d2 * d2, np.stack([2.0 * d0, 2.0 * d1, 2.0 * d2], axis=1)


def f_radius(X):
    x0, x1, x2 = _cols(X)
    r2 = (x0 * x0 + x1 * x1) + x2 * x2
    d0, d1, d2 = x0 - 0.5, x1 - 0.2, x2 + 0.1
    f = (d0 * d0 + 4.0 * (d1 * d1)) + 0.25 * (d2 * d2)
    g = np.stack([2.0 * d0, 8.0 * d1, 0.5 * d2], axis=1)
    bad = r2 > 4.0
    return np.where(bad, np.nan, f), np.where(bad[:, None], np.nan, g)


def f_nan(X):
    return np.full(X.shape[0], np.nan), np.full(X.shape, np.nan)


def f_liar(X):
    x0, x1, x2 = _cols(X)
    return (x0 * x0 + x1 * x1) + x2 * x2, -2.0 * X


def f_fixed(X):
    f, g = f_valley(X)
    g[:, 1] = 0.0
    return f, g


# name -> (function, x0, lo, hi, free, gtol, max_iter): the table kProblems of fit_ctl.cpp
PROBLEMS = {
    "quad": (f_quad, (0.0, 0.0, 0.0), -10.0, 10.0, (1, 1, 1), 1e-10, 100),
    "valley": (f_valley, (-1.2, 1.0, 2.0), -3.0, 3.0, (1, 1, 1), 1e-9, 200),
    "outside": (f_outside, (0.0, 0.0, 0.0), -1.0, 1.0, (1, 1, 1), 1e-10, 100),
    "radius": (f_radius, (1.5, 1.0, 0.5), -3.0, 3.0, (1, 1, 1), 1e-10, 100),
    "nan": (f_nan, (0.5, 0.5, 0.5), -1.0, 1.0, (1, 1, 1), 1e-10, 100),
    "liar": (f_liar, (1.0, 1.0, 1.0), -10.0, 10.0, (1, 1, 1), 1e-10, 100),
    "fixed": (f_fixed, (-1.2, 0.7, 2.0), (-3.0, 0.7, -3.0), (3.0, 0.7, 3.0), (1, 0, 1), 1e-7, 100),
    "one_step": (f_valley, (-1.2, 1.0, 2.0), -3.0, 3.0, (1, 1, 1), 1e-9, 1),
    "start_clipped": (f_outside, (7.0, -7.0, 0.0), -1.0, 1.0, (1, 1, 1), 1e-10, 100),
}


def _trace(program, name):
    run = subprocess.run([program, "trace", name], capture_output=True, text=True, check=True)
    evals, result = [], None
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "eval":
            evals.append([float(v) for v in w[1:]])
        elif w[0] == "result":
            result = [float(v) for v in w[1:]]
    return np.array(evals), result


def _twin(name):
    fn, x0, lo, hi, free, gtol, max_iter = PROBLEMS[name]
    seen = []

    def evaluate(X):
        f, g = fn(X)
        seen.append(np.concatenate([X[0], [f[0]], g[0]]))
        return f, g

    r = fitting.bfgs_box(evaluate, np.array([x0]), np.broadcast_to(lo, (3,)), np.broadcast_to(hi, (3,)), free, gtol, max_iter)
    return np.array(seen), r


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_twin_evaluates_the_headers_points(program, name):
    """Every point fit_search evaluates, in order, with its f and g, and the result: bfgs_box to 1e-12."""
    want, result = _trace(program, name)
    got, r = _twin(name)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(np.concatenate([r.x[0], [r.f[0], r.f0[0], r.grad_norm[0]]]), result[:6], rtol=1e-12, atol=1e-12,
                               equal_nan=True)
    assert [int(r.iterations[0]), int(r.evaluations[0]), int(r.status[0])] == [int(v) for v in result[6:]]
    assert r.evaluations[0] <= 1 + 2 * (fitting.FIT_MAX_HALVINGS + 1) * PROBLEMS[name][6]


def test_twin_in_lock_step_is_the_single_search(program):
    """Four searches with different functions' worth of steps in ONE bfgs_box call: row s is the search run alone (searches
    that have ended keep their result while the others go on)."""
    starts = np.array([[-1.2, 1.0, 2.0], [0.5, -0.5, 0.1], [2.5, 2.5, -2.5], [1.0, 1.0, 0.5]])
    both = fitting.bfgs_box(f_valley, starts, -3.0 * np.ones(3), 3.0 * np.ones(3), (1, 1, 1), 1e-9, 200)
    for s in range(4):
        one = fitting.bfgs_box(f_valley, starts[s:s + 1], -3.0 * np.ones(3), 3.0 * np.ones(3), (1, 1, 1), 1e-9, 200)
        for a, b in zip(both, one):
            assert np.array_equal(a[s:s + 1], b, equal_nan=True)
    assert np.all(both.status == fitting.STATUS_CONVERGED) and both.iterations[3] == 0


def test_status_constants_and_controls():
    assert (fitting.STATUS_CONVERGED, fitting.STATUS_MAX_ITER, fitting.STATUS_LINE_SEARCH, fitting.STATUS_NOT_FINITE) == (0, 1, 2, 3)
    for bad in ({"gtol": -1.0}, {"gtol": np.nan}, {"max_iter": 0}, {"max_iter": fitting.FIT_MAX_ITER_CAP + 1}):
        with pytest.raises(ValueError):
            fitting.bfgs_box(f_quad, np.zeros((1, 3)), -np.ones(3), np.ones(3), (1, 1, 1), **bad)


def test_closed_forms_and_contraction(program):
    """fit_matern_model against matern_closed_forms and fit_contract against matern_contract, 1e-14 relative, d = 1, 2, 3."""
    model = StateSpaceGP((np.zeros((1, 1)), np.zeros((1, 1))), Matern52(variance=1.0, lengthscales=1.0), noise_variance=0.1)
    assert model._matern_forms() is not None
    P1, H1, N1, N2 = model._matern52_unit
    unit = np.concatenate([N1.reshape(-1), N2.reshape(-1), P1.reshape(-1), H1.reshape(-1)])
    run = subprocess.run([program, "forms"] + [repr(float(v)) for v in unit], capture_output=True, text=True, check=True)
    rows = [line.split()[1:] for line in run.stdout.splitlines() if line.startswith("forms")]
    assert len(rows) == 3 * 16
    names = {1: "Matern12", 2: "Matern32", 3: "Matern52"}
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-14, atol=1e-300)
    for w in rows:
        d = int(w[0])
        v = np.array([float(x) for x in w[1:]])
        s2, ell, R, n_obs, ll = v[:5]
        dd = d * d
        at = 5
        lam = v[at]
        N1_h, N2_h, Pinf_h = (v[at + 1 + i * dd:at + 1 + (i + 1) * dd].reshape(d, d) for i in range(3))
        H_h = v[at + 1 + 3 * dd:at + 1 + 3 * dd + d]
        at += 1 + 3 * dd + d
        stats = v[at:at + dd + 2 * d + 1]
        f_h, g_h = v[at + dd + 2 * d + 1], v[at + dd + 2 * d + 2:]
        lam_p, N1_p, N2_p, Pinf_p, H_p = matern_closed_forms(names[d], s2, ell, (P1, H1, N1, N2))
        zero = np.zeros((d, d))
        close(lam, lam_p)
        close(N1_h, zero if N1_p is None else np.array(N1_p, np.float64))
        close(N2_h, zero if N2_p is None else np.array(N2_p, np.float64))
        close(Pinf_h, np.array(Pinf_p, np.float64))
        close(H_h, np.array(H_p, np.float64).reshape(-1))
        F = (np.array(N1_h) - lam * np.eye(d)).reshape(-1)
        PH = np.array(Pinf_p, np.float64) @ np.array(H_p, np.float64).reshape(-1)
        grad = matern_contract(stats[:dd], stats[dd:dd + d], stats[dd + 2 * d], F, PH, ["variance", "lengthscales", "noise_variance"],
                               ell, s2)
        scale = max(1.0, n_obs)
        free = np.array([1, 1, 0 if d == 2 else 1], bool)
        close(f_h, -ll / scale)
        close(g_h, np.where(free, -np.array([s2, ell, R]) * grad / scale, 0.0))
