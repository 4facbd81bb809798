#!/usr/bin/env python3
"""Do two copies of the pssgp package compute the same numbers?  Runs the scenarios of tests/test_model_routes.py, a few
host-only (parallel=False) calls and the calls of tests/test_gpu_scratch_reuse.py once with each copy -- every side in a
process of its own, both against the same built library -- and compares every returned array bit for bit (NaN positions equal).

One difference is allowed: the lengthscale entry of the multi-output and per-observation gradients, whose contraction
<Abar, F> is a flat dot product in one copy and np.sum(Abar * F) in the other.  Two orderings of the same n = d^2 term sum
differ by at most 2 gamma sum |Abar_ij F_ij| / l, gamma = n eps / (1 - n eps), eps = 2^-52; the sum of the absolute terms
is taken from the adjoints the device returned in each process.

Usage: python tools/model_split_identity.py --parent DIR [--out FILE]
DIR holds the other copy's `pssgp/` (e.g. `git worktree add DIR/.. <commit>` and DIR = .../parallel-gps_amd).  One line per call:
`identical`, or the measured difference against its bound.  Exit status 1 if anything else differs."""
import argparse
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = os.path.join(ROOT, "parallel-gps_amd")
LENGTHSCALE = 1           # trainable_parameters() of a single Matern kernel: variance, lengthscales, noise_variance


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _flat(res):
    if isinstance(res, dict):
        res = [res[k] for k in sorted(res)]
    if not isinstance(res, (tuple, list)):
        res = [res]
    return [np.asarray(a) for a in res]


def _host_calls(rec):
    """parallel=False: merge, projection, covariance, draws, the batch loop and the per-observation twin on the host."""
    from pssgp.kernels import Matern32, RBF
    from pssgp.model import StateSpaceGP
    rng = np.random.RandomState(11)
    t = np.cumsum(rng.uniform(0.02, 0.08, 60))
    y = np.sin(2.0 * t) + 0.2 * rng.randn(60)
    y[7] = np.nan
    tq = rng.uniform(t[0], t[-1], 15)[:, None]
    thetas = np.array([[1.3, 0.7, 0.1], [0.9, 1.1, 0.2]])
    for name, kern in (("Matern32", lambda: Matern32(1.3, 0.7)), ("RBF", lambda: RBF(1.2, 0.8, order=3, balancing_iter=5))):
        m = StateSpaceGP((t, y), kern(), 0.1, parallel=False)
        rec(f"{name} objective", m.maximum_log_likelihood_objective)
        rec(f"{name} predict_f", lambda: m.predict_f(np.sort(tq, axis=0)))
        rec(f"{name} predict_f full_cov", lambda: m.predict_f(tq, full_cov=True))
        rec(f"{name} predict_f_samples", lambda: m.predict_f_samples(tq, num_samples=2, seed=1))
        rec(f"{name} predict_f_batch", lambda: m.predict_f_batch(tq, thetas, return_log_likelihood=True))
        rec(f"{name} predict_f_batch mixture", lambda: m.predict_f_batch(tq, thetas, reduce="mixture"))
        h = StateSpaceGP((t, y), kern(), 0.1, parallel=False, observation_variances=rng.uniform(0.0, 0.3, 60))
        rec(f"{name} per-observation objective", h.maximum_log_likelihood_objective)
        rec(f"{name} per-observation predict_f", lambda: h.predict_f(np.sort(tq, axis=0)))


def child(pkg, dump):
    sys.path[:0] = [ROOT, pkg]
    from pssgp import _backend
    import pssgp
    assert os.path.dirname(os.path.dirname(os.path.abspath(pssgp.__file__))) == os.path.abspath(pkg), pssgp.__file__
    out, terms = {}, []

    def spied(fn):
        def call(form, Pinf, H, *args, **kwargs):
            stats = fn(form, Pinf, H, *args, **kwargs)
            lam, N1, _ = form
            d = N1.shape[0]
            F = np.asarray(N1, np.float64) - float(lam) * np.eye(d)
            ell = np.sqrt(2.0 * d - 1.0) / float(lam)           # lam = sqrt(2 nu) / l, nu = d - 1/2
            terms.append((d, float(np.sum(np.abs(stats[1] * F))) / ell))
            return stats
        return call

    _backend.gp_ll_grad_multi = spied(_backend.gp_ll_grad_multi)
    _backend.gp_ll_grad_adj_het = spied(_backend.gp_ll_grad_adj_het)

    def recorder(prefix):
        def rec(label, fn):
            del terms[:]
            key = f"{prefix} | {label}"
            try:
                for i, a in enumerate(_flat(fn())):
                    out[f"{key} | {i}"] = a
            except Exception as e:              # noqa: BLE001 -- both sides must raise the same
                out[f"{key} | 0"] = np.asarray(type(e).__name__)
            if terms:
                out[f"{key} | terms"] = np.asarray(terms[-1])
        return rec

    census = _load("test_model_routes")
    for name, (fn, *args) in census.SCENARIOS.items():
        fn(recorder(name), *args)
    _host_calls(recorder("host"))
    try:
        steps = _load("test_gpu_scratch_reuse")._steps()
    except Exception as e:                      # noqa: BLE001 -- no device: recorded like any other call
        steps = [("steps", 0, lambda e=e: (_ for _ in ()).throw(e))]
    for name, budget, call in steps:
        def run(budget=budget, call=call):
            ctx = _backend.get_context()
            try:
                ctx.set_batch_scratch(budget)
                return call()
            finally:
                ctx.set_batch_scratch(0)
        recorder("scratch reuse")(name, run)
    np.savez(dump, **out)


def compare(parent, new, write):
    eps = 2.0 ** -52
    bad = 0
    calls = []
    for key in list(parent) + [k for k in new if k not in parent]:
        call = key.rsplit(" | ", 1)[0]
        if call not in calls:
            calls.append(call)
    for call in calls:
        keys = sorted(k for k in set(parent) | set(new) if k.rsplit(" | ", 1)[0] == call and not k.endswith("| terms"))
        verdict = "identical"
        for k in keys:
            a, b = parent.get(k), new.get(k)
            if a is None or b is None or a.shape != b.shape or a.dtype != b.dtype:
                verdict = f"DIFFERENT (output {k.rsplit(' | ', 1)[1]}: missing, or another shape or dtype)"
                break
            if a.dtype.kind in "US":
                if str(a) != str(b):
                    verdict = f"DIFFERENT (raised {a} / {b})"
                    break
                verdict = f"identical (both raise {a})"
                continue
            if np.array_equal(a, b, equal_nan=True):
                continue
            terms = [s.get(call + " | terms") for s in (parent, new)]
            rest = np.ones(a.shape, bool)
            if a.ndim == 1 and a.size > LENGTHSCALE and terms[0] is not None and terms[1] is not None:
                rest[LENGTHSCALE] = False
            if rest.all() or not np.array_equal(a[rest], b[rest], equal_nan=True):
                verdict = f"DIFFERENT (output {k.rsplit(' | ', 1)[1]}: max |difference| {np.nanmax(np.abs(a - b)):.3e})"
                break
            n = int(terms[0][0]) ** 2
            bound = 2.0 * (n * eps / (1.0 - n * eps)) * max(terms[0][1], terms[1][1])
            diff = abs(float(a[LENGTHSCALE]) - float(b[LENGTHSCALE]))
            verdict = f"lengthscale entry |new - parent| = {diff:.3e}, bound {bound:.3e}; every other entry identical"
            if not diff <= bound:
                verdict = "DIFFERENT: " + verdict
                break
        bad += verdict.startswith("DIFFERENT")
        write(f"{call}: {verdict}")
    write(f"{len(calls)} calls compared, {bad} different")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="directory that holds the other copy's pssgp/")
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=2, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    env = dict(os.environ, PGPS_LIB=os.environ.get("PGPS_LIB", os.path.join(OWN, "pssgp", "libpgps.so")))
    sides = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, pkg in (("parent", os.path.abspath(args.parent)), ("new", OWN)):
            dump = os.path.join(tmp, name + ".npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pkg, dump], check=True, env=env, timeout=600)
            with np.load(dump) as z:
                sides.append({k: z[k] for k in z.files})
    lines = []
    bad = compare(sides[0], sides[1], lines.append)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
