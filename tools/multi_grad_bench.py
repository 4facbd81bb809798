"""Gradients of several outputs on one clock: _backend.gp_ll_grad_multi (ONE filter pass and ONE reverse pass for the M columns
of Y) against the loop of M single-column Series.gp_ll_grad_adj calls -- what StateSpaceGP's column loop runs per column, on
series that are already resident on the device, and code this library still carries unchanged, so one build serves both
sides.  Three times per point:

    multi       host arrays in, statistics out, ends in a stream synchronise (Y is copied per call: what a model pays)
    multi_dev   pgps_gp_ll_grad_multi_dev_f64 on device-resident (ts, Y) + a synchronise (the passes alone)
    loop        M calls on M resident series (each ends in a synchronise; no copy of the series)

Every shape is warmed up first, the sides alternate --reps times, medians (with min and max) are reported, and the results
are compared at the sizes that are timed.  Writes profiles/multi_grad_bench.json and prints a table.

One size per process, every GPU step under its own time limit, chained so that trouble ends the run:

    timeout -k 10 300 python tools/multi_grad_bench.py --size small && \\
    timeout -k 10 300 python tools/multi_grad_bench.py --size mid && \\
    timeout -k 10 600 python tools/multi_grad_bench.py --size large

small: N = 4096, M in {2, 3, 4, 16, 64}; mid: N = 2^15 .. 2^18, M = 16 (where the copy of Y per call starts to cost more than the
loop's M passes over resident series); large: N = 2^20, M = 16.  Matern-3/2 (d = 2) and Matern-5/2 (d = 3); small also
Matern-1/2 (d = 1)."""
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

# size -> [(N, M)], kernels
SIZES = {"small": ([(4096, m) for m in (2, 3, 4, 16, 64)], ("m12", "m32", "m52")),
         "mid": ([(2 ** e, 16) for e in (15, 16, 17, 18)], ("m32", "m52")),
         "large": ([(2 ** 20, 16)], ("m32", "m52"))}


def _model(kname):
    from pssgp import _backend as Bk
    from pssgp.kernels import Matern12, Matern32, Matern52
    sde = {"m12": Matern12, "m32": Matern32, "m52": Matern52}[kname](1.0, 1.0).get_sde()
    return Bk.nilpotent_form(sde.F), np.asarray(sde.P0), np.asarray(sde.H).reshape(-1)


def _problem(n, m):
    rng = np.random.RandomState(n + m)
    t = np.cumsum(0.05 * (0.5 + rng.rand(n)))
    Y = np.sin(0.7 * t)[:, None] * rng.uniform(0.5, 2.0, (1, m)) + 0.3 * rng.randn(n, m)
    Y[rng.rand(n) < 0.05] = np.nan              # rows missing in every column
    return t, Y


def _flat(stats):
    return np.concatenate([np.asarray(s, np.float64).reshape(-1) for s in stats])


def run(size, reps, min_window):
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    points, kernels = SIZES[size]
    rows = []
    for kname in kernels:
        form, P, H = _model(kname)
        lam, N1, N2 = form
        d = P.shape[0]
        packed = Bk.Series.pack(form, P, H)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)            # noqa: E731
        model = [np.ascontiguousarray(a, np.float64) for a in (N1, N2, P, H)]
        for n, m in points:
            t, Y = _problem(n, m)
            series = [Bk.Series(t, np.ascontiguousarray(Y[:, j])) for j in range(m)]
            nout = m + d * d + 2 * d + 1
            dev = {"t": ctx.malloc(t.nbytes), "y": ctx.malloc(Y.nbytes), "out": ctx.malloc(8 * nout)}
            try:
                ctx.h2d(dev["t"], t), ctx.h2d(dev["y"], Y)
                d_out = np.empty(nout)

                def multi():
                    return Bk.gp_ll_grad_multi(form, P, H, 0.1, t, Y)

                def multi_dev():
                    with ctx.lock:
                        Bk.check(ctx, ctx.lib.pgps_gp_ll_grad_multi_dev_f64(
                            ctx.handle, n, m, d, lam, *[p(a) for a in model], 0.1, ctypes.c_void_p(dev["t"]),
                            ctypes.c_void_p(dev["y"]), 0.0, ctypes.c_void_p(dev["out"])), "pgps_gp_ll_grad_multi_dev_f64")
                    ctx.synchronize()

                def loop():
                    return [s.gp_ll_grad_adj(packed, 0.1) for s in series]

                got, want = multi(), loop()     # warm-up of this shape, and the comparison
                multi_dev()
                ctx.d2h(d_out, dev["out"])
                same_bits = bool(np.array_equal(d_out.view(np.uint64), np.concatenate([got[0], _flat(got[1:])]).view(np.uint64)))
                ref = np.sum([_flat(w[1:]) for w in want], axis=0)
                err = float(np.max(np.abs(_flat(got[1:]) - ref)) / np.max(np.abs(ref)))
                err_ll = max(abs(got[0][j] - want[j][0]) / abs(want[j][0]) for j in range(m))
                # enough calls per timed window that the clock and the scheduler do not dominate a short call
                tic = time.perf_counter()
                multi()
                inner = max(1, int(min_window / max(time.perf_counter() - tic, 1e-6)))
                inner = min(inner, 200)
                times = {"multi": [], "multi_dev": [], "loop": []}
                for _ in range(reps):
                    for name, fn in (("multi", multi), ("multi_dev", multi_dev), ("loop", loop)):
                        tic = time.perf_counter()
                        for _ in range(inner):
                            fn()
                        times[name].append((time.perf_counter() - tic) / inner)
            finally:
                for ptr in dev.values():
                    ctx.free(ptr)
                for s in series:
                    s.close()
            row = {"size": size, "kernel": kname, "N": n, "M": m, "calls_per_window": inner, "stats_relerr": err,
                   "ll_relerr": err_ll, "dev_entry_same_bits": same_bits}
            for name, v in times.items():
                row[name + "_ms"] = [1e3 * min(v), 1e3 * statistics.median(v), 1e3 * max(v)]
            rows.append(row)
            mm, md, ml = row["multi_ms"][1], row["multi_dev_ms"][1], row["loop_ms"][1]
            print(f"{size} {kname} N={n} M={m:3d}: multi {mm:9.3f} ms   multi_dev {md:9.3f} ms   loop {ml:9.3f} ms   "
                  f"loop / multi {ml / mm:5.2f}   loop / multi_dev {ml / md:5.2f}   agree: stats {err:.1e} ll {err_ll:.1e} "
                  f"dev bits {same_bits}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=list(SIZES), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-window", type=float, default=0.05, help="seconds of calls per timed window, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_grad_bench.json"))
    args = ap.parse_args()
    rows = run(args.size, args.reps, args.min_window)
    old = []
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = [r for r in json.load(f) if r["size"] != args.size]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(old + rows, f, indent=1)


if __name__ == "__main__":
    main()
