"""The exact gradient at B hyper-parameter settings: StateSpaceGP.log_likelihood_and_grad_batch (the batched adjoint pass
forced whatever B, so that the switch-over can be read off) against the loop a user writes without it (assign row b,
log_likelihood_and_grad(), on a model past its first evaluation: resident series).  The two are timed in child processes
of their own, alternated --rounds times; the loop's children load --baseline-lib when given (a build of the parent
commit), through PGPS_LIB.  Wall clock around calls that end in a stream synchronise, every shape warmed up first;
min / median / max over all repeats of all rounds.  Writes profiles/grad_batch_bench.json.

    python tools/grad_batch_bench.py [--baseline-lib PATH] [--rounds 3] [--reps 7] [--out PATH]

The figure behind StateSpaceGP._GRAD_BATCH_FROM / _GRAD_BATCH_FROM_LTI is `batch_from` of a family: the smallest B from which
on, at every length measured, the batch's median lies below the loop's minimum (null: the batch never wins there)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-gps_amd"))

BS = (1, 2, 4, 16, 64, 256)
SHAPES = [(kname, n, B) for kname in ("m32", "m52") for n in (1000, 4096, 16384) for B in BS] + [("c5", 1000, B) for B in BS]


def _kernel(kname):
    from pssgp.kernels import Matern32, Matern52, Periodic, SquaredExponential
    if kname == "m32":
        return Matern32(1.0, 1.0)
    if kname == "m52":
        return Matern52(1.0, 1.0)
    return Periodic(SquaredExponential(1., 1.), period=1., order=1) * Matern32(1., 1.) + Matern52(1., 1.)     # d = 11


def _problem(kname, n, B):
    from pssgp.model import StateSpaceGP
    rng = np.random.RandomState(n)
    t = np.cumsum(0.05 * (0.5 + rng.rand(n)))
    y = np.sin(0.7 * t) + 0.3 * rng.randn(n)
    m = StateSpaceGP((t[:, None], y[:, None]), _kernel(kname), noise_variance=0.1, parallel=True)
    base = np.array([getattr(o, a) for o, a in m.trainable_parameters()], np.float64)
    thetas = base[None, :] * np.exp(rng.uniform(-0.2, 0.2, (B, base.size)))
    m.log_likelihood_and_grad()
    m.log_likelihood_and_grad()         # past the first evaluation: the series is resident
    return m, thetas


def _time(fn, reps):
    fn()                                # warm-up of this shape
    out = []
    for _ in range(reps):
        tic = time.perf_counter()
        fn()
        out.append(time.perf_counter() - tic)
    return out


def child(mode, reps):
    res = {}
    for kname, n, B in SHAPES:
        m, thetas = _problem(kname, n, B)
        params = m.trainable_parameters()
        key = f"{kname} N={n} B={B}"
        if mode == "loop":
            def loop():
                saved = [getattr(o, a) for o, a in params]
                for row in thetas:
                    for (o, a), v in zip(params, row):
                        setattr(o, a, float(v))
                    m.log_likelihood_and_grad()
                for (o, a), v in zip(params, saved):
                    setattr(o, a, v)
            res[key] = {"loop": _time(loop, reps)}
            continue
        m._GRAD_BATCH_FROM = m._GRAD_BATCH_FROM_LTI = 1          # the batched launches whatever B
        res[key] = {"batch": _time(lambda: m.log_likelihood_and_grad_batch(thetas), reps)}
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["loop", "batch"])
    ap.add_argument("--baseline-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_batch_bench.json"))
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps)
        return
    merged = {}
    for r in range(args.rounds):
        for mode in ("loop", "batch"):
            env = dict(os.environ)
            if mode == "loop" and args.baseline_lib:
                env["PGPS_LIB"] = os.path.abspath(args.baseline_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(args.reps)]
            out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=600).stdout
            line = [ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1]
            for key, series in json.loads(line[7:]).items():
                for what, secs in series.items():
                    merged.setdefault(key, {}).setdefault(what, []).extend(secs)
    report = {"baseline": "a build of the parent commit" if args.baseline_lib else "the library under test", "rounds": args.rounds,
              "reps": args.reps, "unit": "milliseconds per call of all B settings", "shapes": {}, "batch_from": {}}
    wins = {}
    for key, series in merged.items():
        row = {what: {"min": round(1e3 * min(s), 4), "median": round(1e3 * statistics.median(s), 4),
                      "max": round(1e3 * max(s), 4), "n": len(s)} for what, s in series.items()}
        if "loop" in row and "batch" in row:
            row["batch_median_over_loop_min"] = round(row["batch"]["median"] / row["loop"]["min"], 4)
            kname, _, b = key.split()
            wins.setdefault(kname, {}).setdefault(int(b[2:]), []).append(row["batch"]["median"] < row["loop"]["min"])
        report["shapes"][key] = row
        print(key, json.dumps(row))
    for kname, by_b in wins.items():
        from_b = None
        for B in sorted(by_b, reverse=True):
            if not all(by_b[B]):
                break
            from_b = B
        report["batch_from"][kname] = from_b
    print("batch_from", json.dumps(report["batch_from"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
