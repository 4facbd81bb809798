"""Predictive checks: what pgps_gp_loo_dev_f64 costs, two ways -- the two scores only (no per-step store) and all four arrays
-- against what a user had to do without it: pgps_gp_predict_dev_f64 with the training times as the query times (tq = ts,
K = N: a merge, a filter + smoother over 2N steps, N means and variances of f, the noise algebra left to the caller).  That
entry point is code this library carries unchanged, so one build serves both sides.  Like is compared with like: the new call
exists in the multi-launch form only, so the resident launch and the one-launch forms are switched off (pgps_set_resident(0),
pgps_set_one_launch(0)) for the whole run and the baseline runs its three-launch form (plus its merge).  Device-resident
arrays, every call ends in a stream synchronise.

Every shape is warmed up first, the three sides alternate --reps times, medians (with min and max) over windows of at least
--min-window seconds of calls are reported, and the leave-one-out law computed from the baseline's (mean, var) on the host is
compared with the new call's arrays at the sizes that are timed.  Writes profiles/loo_bench.json and prints a table.

One size per process, every GPU step under its own time limit, chained so that trouble ends the run:

    timeout -k 10 300 python tools/loo_bench.py --size small && \\
    timeout -k 10 600 python tools/loo_bench.py --size large

small: N = 4096; large: N = 2^20.  Matern-3/2 (d = 2) and Matern-5/2 (d = 3)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-gps_amd"))

SIZES = {"small": 4096, "large": 2 ** 20}
R = 0.1
FIELDS = ("osa_mean", "osa_var", "loo_mean", "loo_var")


def _model(kname):
    from pssgp import _backend as Bk
    from pssgp.kernels import Matern32, Matern52
    sde = {"m32": Matern32, "m52": Matern52}[kname](1.0, 1.0).get_sde()
    return Bk.nilpotent_form(sde.F), np.asarray(sde.P0), np.asarray(sde.H).reshape(-1)


def _problem(n):
    rng = np.random.RandomState(n)
    t = np.cumsum(0.05 * (0.5 + rng.rand(n)))
    y = np.sin(0.7 * t) + 0.3 * rng.randn(n)
    y[rng.rand(n) < 0.05] = np.nan
    return t, y


def run(size, reps, min_window):
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    ctx.set_resident(0)
    ctx.set_one_launch(0)
    n = SIZES[size]
    rows = []
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)            # noqa: E731
    for kname in ("m32", "m52"):
        form, P, H = _model(kname)
        lam, N1, N2 = form
        d = P.shape[0]
        mp = [p(a) for a in [np.ascontiguousarray(a, np.float64) for a in (N1, N2, P, H)]]
        t, y = _problem(n)
        host = {"t": t, "y": y}
        sizes = {f: 8 * n for f in FIELDS + ("mean", "var")}
        sizes.update({"sums": 16, "sums0": 16, "ll": 16})
        dev = {key: ctx.malloc(a.nbytes) for key, a in host.items()}
        dev.update({key: ctx.malloc(b) for key, b in sizes.items()})
        D = {key: ctypes.c_void_p(ptr) for key, ptr in dev.items()}
        lib, h = ctx.lib, ctx.handle
        L, I, F = ctypes.c_long, ctypes.c_int, ctypes.c_double
        nn, dd, lm, z, Rh = L(n), I(d), F(lam), F(0.0), F(R)

        def call(name, *args):
            with ctx.lock:
                Bk.check(ctx, getattr(lib, name)(h, *args), name)
            ctx.synchronize()

        sides = {
            "scores": lambda: call("pgps_gp_loo_dev_f64", nn, dd, lm, *mp, Rh, D["t"], D["y"], z, None, None, None, None, D["sums0"]),
            "arrays": lambda: call("pgps_gp_loo_dev_f64", nn, dd, lm, *mp, Rh, D["t"], D["y"], z, *(D[f] for f in FIELDS), D["sums"]),
            "predict": lambda: call("pgps_gp_predict_dev_f64", nn, nn, dd, lm, *mp, Rh, D["t"], D["y"], z, D["t"], D["mean"], D["var"],
                                    D["ll"]),
        }
        try:
            for key, a in host.items():
                ctx.h2d(dev[key], a)
            for fn in sides.values():           # warm-up of this shape, and the comparison
                fn()
            got = {key: np.empty(sizes[key] // 8) for key in ("loo_mean", "loo_var", "mean", "var", "sums", "sums0", "ll")}
            for key, a in got.items():
                ctx.d2h(a, dev[key])
            obs = ~np.isnan(y)
            m, v = got["mean"][obs], got["var"][obs]
            want = (m * R - y[obs] * v) / (R - v), R * R / (R - v)
            err = max(float(np.max(np.abs(a[obs] - b)) / np.max(np.abs(b))) for a, b in zip((got["loo_mean"], got["loo_var"]), want))
            err = max(err, abs(got["sums"][0] - got["ll"][0]) / abs(got["ll"][0]))
            same_bits = bool(np.array_equal(got["sums"].view(np.uint64), got["sums0"].view(np.uint64)))
            tic = time.perf_counter()
            sides["arrays"]()
            inner = min(200, max(1, int(min_window / max(time.perf_counter() - tic, 1e-6))))
            times = {name: [] for name in sides}
            for _ in range(reps):
                for name, fn in sides.items():
                    tic = time.perf_counter()
                    for _ in range(inner):
                        fn()
                    times[name].append((time.perf_counter() - tic) / inner)
            row = {"size": size, "kernel": kname, "d": d, "N": n, "calls_per_window": inner, "relerr_against_predict": err,
                   "scores_only_same_bits": same_bits}
            for name, vals in times.items():
                row[name + "_ms"] = [1e3 * min(vals), 1e3 * statistics.median(vals), 1e3 * max(vals)]
            row["ratio_scores"] = row["scores_ms"][1] / row["predict_ms"][1]
            row["ratio_arrays"] = row["arrays_ms"][1] / row["predict_ms"][1]
            rows.append(row)
            print(f"{size} {kname} N={n}: scores {row['scores_ms'][1]:9.4f} ms   four arrays {row['arrays_ms'][1]:9.4f} ms   "
                  f"predict at tq = ts {row['predict_ms'][1]:9.4f} ms   ratios {row['ratio_scores']:5.3f} {row['ratio_arrays']:5.3f}   "
                  f"agree {err:.1e}", flush=True)
        finally:
            for ptr in dev.values():
                ctx.free(ptr)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=list(SIZES), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-window", type=float, default=0.05, help="seconds of calls per timed window, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_bench.json"))
    args = ap.parse_args()
    rows = run(args.size, args.reps, args.min_window)
    old = []
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = [r for r in json.load(f) if r["size"] != args.size]
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(old + rows, f, indent=1)


if __name__ == "__main__":
    main()
