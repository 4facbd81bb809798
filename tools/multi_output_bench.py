"""Several outputs on one clock: _backend.gp_predict_multi (ONE covariance pass for the M columns of Y) against the loop of M
_backend.gp_predict calls -- the only route before the multi-output scan existed, and code this library still carries
unchanged, so one build serves both sides.  Both sides take host arrays and end in a stream synchronise, so the host clock
around a call is the call's time (copies included: that is what a model pays).  Every shape is warmed up first, the two sides
alternate --reps times, medians (with min and max) are reported, and the two results are compared column by column at the
sizes that are timed.  Writes profiles/multi_output_bench.json and prints a table.

One size per process, every GPU step under its own time limit, chained so that trouble ends the run:

    timeout -k 10 600 python tools/multi_output_bench.py --size small && \\
    timeout -k 10 900 python tools/multi_output_bench.py --size large

small: (N, K) = (4096, 1024); large: (2^20, 2^18); M in {1, 4, 16, 64}; Matern-3/2 (d = 2) and Matern-5/2 (d = 3)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-gps_amd"))

SIZES = {"small": (4096, 1024), "large": (2 ** 20, 2 ** 18)}
COLUMNS = (1, 4, 16, 64)


def _model(kname):
    from pssgp import _backend as Bk
    from pssgp.kernels import Matern32, Matern52
    sde = {"m32": Matern32, "m52": Matern52}[kname](1.0, 1.0).get_sde()
    return Bk.nilpotent_form(sde.F), np.asarray(sde.P0), np.asarray(sde.H).reshape(-1)


def _problem(n, k, m):
    rng = np.random.RandomState(n + k + m)
    t = np.cumsum(0.05 * (0.5 + rng.rand(n)))
    Y = np.sin(0.7 * t)[:, None] * rng.uniform(0.5, 2.0, (1, m)) + 0.3 * rng.randn(n, m)
    Y[rng.rand(n) < 0.05] = np.nan              # rows missing in every column
    tq = np.sort(rng.uniform(t[0], t[-1], k))
    return t, Y, tq


def run(size, reps, min_window):
    from pssgp import _backend as Bk
    n, k = SIZES[size]
    rows = []
    for kname in ("m32", "m52"):
        form, P, H = _model(kname)
        for m in COLUMNS:
            t, Y, tq = _problem(n, k, m)
            cols = [np.ascontiguousarray(Y[:, j]) for j in range(m)]
            multi = lambda: Bk.gp_predict_multi(form, P, H, 0.1, t, Y, tq)                         # noqa: E731
            loop = lambda: [Bk.gp_predict(form, P, H, 0.1, t, c, tq) for c in cols]                # noqa: E731
            got, want = multi(), loop()         # warm-up of this shape, and the comparison
            err = max(float(np.max(np.abs(got[0][:, j] - want[j][0])) / max(1.0, float(np.max(np.abs(want[j][0])))))
                      for j in range(m))
            err_ll = max(abs(got[2][j] - want[j][2]) / abs(want[j][2]) for j in range(m))
            # enough calls per timed window that the clock and the scheduler do not dominate a short call
            tic = time.perf_counter()
            multi()
            inner = max(1, int(min_window / max(time.perf_counter() - tic, 1e-6)))
            inner = min(inner, 200)
            tm, tl = [], []
            for _ in range(reps):
                for fn, out in ((multi, tm), (loop, tl)):
                    tic = time.perf_counter()
                    for _ in range(inner):
                        fn()
                    out.append((time.perf_counter() - tic) / inner)
            row = {"size": size, "kernel": kname, "N": n, "K": k, "M": m, "calls_per_window": inner,
                   "multi_ms": [1e3 * min(tm), 1e3 * statistics.median(tm), 1e3 * max(tm)],
                   "loop_ms": [1e3 * min(tl), 1e3 * statistics.median(tl), 1e3 * max(tl)],
                   "mean_relerr": err, "ll_relerr": err_ll}
            rows.append(row)
            med_m, med_l = row["multi_ms"][1], row["loop_ms"][1]
            print(f"{size} {kname} N={n} K={k} M={m:3d}: multi {med_m:9.3f} ms ({med_m / m:8.3f} per column)   "
                  f"loop {med_l:9.3f} ms ({med_l / m:8.3f} per column)   loop / multi {med_l / med_m:5.2f}   "
                  f"agree: mean {err:.1e} ll {err_ll:.1e}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=list(SIZES), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-window", type=float, default=0.05, help="seconds of calls per timed window, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_output_bench.json"))
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
