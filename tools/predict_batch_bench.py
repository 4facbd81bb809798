"""predict_f at B hyper-parameter settings: StateSpaceGP.predict_f_batch against the loop a user writes without it (assign
row b, predict_f(Xnew), on a model past its first evaluation: resident series).  The two are timed in child processes
of their own, alternated --rounds times; the loop's children load --baseline-lib when given (a build of the parent
commit), through PGPS_LIB.  Wall clock around calls that end in a stream synchronise, every shape warmed up first;
min / median / max over all repeats of all rounds.  Writes profiles/predict_batch_bench.json.

    python tools/predict_batch_bench.py [--baseline-lib PATH] [--rounds 3] [--reps 5] [--out PATH] [--forms]

--forms adds, for the Matern shapes, the batch under pgps_set_batch_form 1 and 2 and under scratch budgets of 8 MiB to
1 GiB (the numbers behind the automatic form and kBatchScratchDefault, csrc/pgps_scratch.h), and for B <= 10 the batched
launches forced (the number behind StateSpaceGP._PREDICT_BATCH_FROM)."""
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

SHAPES = [("sunspot", "m32", 3000, 2000, B) for B in (1, 2, 4, 10, 100, 1000)] + \
         [("c1", "m32", 4096, 1024, B) for B in (8, 64, 512)] + \
         [("c5_qp_m52", "c5", 3192, 1024, B) for B in (8, 64)] + \
         [("long", "m32", 2 ** 17, 2 ** 15, 8)]


def _kernel(kname):
    from pssgp.kernels import Matern32, Matern52, Periodic, SquaredExponential
    if kname == "m32":
        return Matern32(1.0, 1.0)
    return Periodic(SquaredExponential(1., 1.), period=1., order=1) * Matern32(1., 1.) + Matern52(1., 1.)     # d = 11


def _problem(kname, n, k, B):
    from pssgp.model import StateSpaceGP
    rng = np.random.RandomState(n + k)
    t = np.cumsum(0.05 * (0.5 + rng.rand(n)))
    y = np.sin(0.7 * t) + 0.3 * rng.randn(n)
    tq = np.sort(rng.uniform(t[0], t[-1], k))[:, None]
    m = StateSpaceGP((t[:, None], y[:, None]), _kernel(kname), noise_variance=0.1, parallel=True)
    base = np.array([getattr(o, a) for o, a in m.trainable_parameters()], np.float64)
    thetas = base[None, :] * np.exp(rng.uniform(-0.3, 0.3, (B, base.size)))
    m.predict_f(tq)
    m.predict_f(tq)                     # past the first evaluation: the series is resident
    return m, tq, thetas


def _time(fn, reps):
    fn()                                # warm-up of this shape
    out = []
    for _ in range(reps):
        tic = time.perf_counter()
        fn()
        out.append(time.perf_counter() - tic)
    return out


def child(mode, reps, forms):
    from pssgp import _backend
    res = {}
    for name, kname, n, k, B in SHAPES:
        m, tq, thetas = _problem(kname, n, k, B)
        params = m.trainable_parameters()
        key = f"{name} N={n} K={k} B={B}"
        if mode == "loop":
            def loop():
                saved = [getattr(o, a) for o, a in params]
                for row in thetas:
                    for (o, a), v in zip(params, row):
                        setattr(o, a, float(v))
                    m.predict_f(tq)
                for (o, a), v in zip(params, saved):
                    setattr(o, a, v)
            res[key] = {"loop": _time(loop, reps)}
            continue
        res[key] = {"batch": _time(lambda: m.predict_f_batch(tq, thetas), reps),
                    "batch_mixture": _time(lambda: m.predict_f_batch(tq, thetas, reduce="mixture"), reps)}
        if forms and kname == "m32" and B <= 10:
            # the batched launches whatever B: the measurement behind StateSpaceGP._PREDICT_BATCH_FROM
            m._PREDICT_BATCH_FROM = 1
            res[key]["batch_forced"] = _time(lambda: m.predict_f_batch(tq, thetas), reps)
            del m._PREDICT_BATCH_FROM
        if forms and B >= 8:
            ctx = _backend.get_context()
            for form in ((1, 2) if kname == "m32" else ()):
                if form == 1 and n + k > 65536:
                    continue
                ctx.set_batch_form(form)
                try:
                    res[key][f"form{form}"] = _time(lambda: m.predict_f_batch(tq, thetas), reps)
                finally:
                    ctx.set_batch_form(0)
            for mib in (8, 16, 32, 64, 1024):
                ctx.set_batch_scratch(mib << 20)
                try:
                    res[key][f"scratch{mib}MiB"] = _time(lambda: m.predict_f_batch(tq, thetas), reps)
                finally:
                    ctx.set_batch_scratch(0)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["loop", "batch"])
    ap.add_argument("--baseline-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--forms", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_batch_bench.json"))
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps, args.forms)
        return
    merged = {}
    for r in range(args.rounds):
        for mode in ("loop", "batch"):
            env = dict(os.environ)
            if mode == "loop" and args.baseline_lib:
                env["PGPS_LIB"] = os.path.abspath(args.baseline_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(args.reps)]
            if args.forms and r == 0:
                cmd.append("--forms")
            out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=900).stdout
            line = [ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1]
            for key, series in json.loads(line[7:]).items():
                for what, secs in series.items():
                    merged.setdefault(key, {}).setdefault(what, []).extend(secs)
    report = {"baseline": "a build of the parent commit" if args.baseline_lib else "the library under test", "rounds": args.rounds, "reps": args.reps,
              "unit": "milliseconds per call of all B settings", "shapes": {}}
    for key, series in merged.items():
        row = {what: {"min": round(1e3 * min(s), 4), "median": round(1e3 * statistics.median(s), 4),
                      "max": round(1e3 * max(s), 4), "n": len(s)} for what, s in series.items()}
        if "loop" in row and "batch" in row:
            row["slowest_batch_over_fastest_loop"] = round(row["batch"]["max"] / row["loop"]["min"], 4)
        report["shapes"][key] = row
        print(key, json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
