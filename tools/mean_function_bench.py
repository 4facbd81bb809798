"""Mean functions: what pgps_gp_gram_multi_dev_f64 costs -- one covariance pass over the columns V = [y, phi_1 .. phi_p] with the
standardised innovations kept in scratch, one Gram pass, (1 + p)^2 doubles out -- against what one had to do before it existed:
1 + p single-column one-step-ahead passes (pgps_gp_loo_dev_f64 with the one-step-ahead arrays asked for and the leave-one-out
ones not; code this library carries unchanged, so one build serves both sides), their 2 (1 + p) N means and variances copied
back, and the host product W^T W of the innovations (v - mean) / sqrt(var).  Device-resident inputs on both sides; every call ends
in a stream synchronise; the copies back and the host product are part of the baseline's time, because the Gram matrix is what
is asked for -- the 1 + p passes alone (no copy, no product: a lower bound of any baseline) are timed as a third side.  The
resident launch and the one-launch forms are switched off for the whole run, as in tools/loo_bench.py.

Every shape is warmed up first, the three sides alternate --reps times, medians (with min and max) over windows of at least
--min-window seconds of calls are reported, and the two Gram matrices are compared at the sizes that are timed.  Writes
profiles/mean_function_bench.json and prints a table.

One size per process, every GPU step under its own time limit, chained so that trouble ends the run:

    timeout -k 10 300 python tools/mean_function_bench.py --size small && \\
    timeout -k 10 600 python tools/mean_function_bench.py --size large

small: N = 4096; large: N = 2^20.  Matern-3/2 (d = 2) and Matern-5/2 (d = 3); 1 + p = 4 and 16 columns."""
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
COLUMNS = (4, 16)
R = 0.1


def _model(kname):
    from pssgp import _backend as Bk
    from pssgp.kernels import Matern32, Matern52
    sde = {"m32": Matern32, "m52": Matern52}[kname](1.0, 1.0).get_sde()
    return Bk.nilpotent_form(sde.F), np.asarray(sde.P0), np.asarray(sde.H).reshape(-1)


def _problem(n, m):
    """(t (n,), V (n, m) = [y, 1, Fourier pairs on the record]); 5 % of the rows missing in every column."""
    rng = np.random.RandomState(n + m)
    t = np.cumsum(0.05 * (0.5 + rng.rand(n)))
    u = (t - t[0]) / (t[-1] - t[0])
    cols = [2.0 + u + np.sin(0.7 * t) + 0.3 * rng.randn(n), np.ones(n)]
    for j in range(1, m - 1):
        w = 2.0 * np.pi * ((j + 1) // 2)
        cols.append(np.sin(w * u) if j % 2 else np.cos(w * u))
    V = np.stack(cols, axis=1)
    V[rng.rand(n) < 0.05] = np.nan
    return t, np.ascontiguousarray(V)


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
        for m in COLUMNS:
            t, V = _problem(n, m)
            cols = np.ascontiguousarray(V.T)                    # the baseline's columns, each contiguous
            host = {"t": t, "V": V, "cols": cols}
            sizes = {"mean": 8 * n * m, "var": 8 * n * m, "sums": 16, "gram": 8 * m * m, "logdet": 8, "n_obs": 8}
            dev = {key: ctx.malloc(a.nbytes) for key, a in host.items()}
            dev.update({key: ctx.malloc(b) for key, b in sizes.items()})
            D = {key: ctypes.c_void_p(ptr) for key, ptr in dev.items()}
            col = lambda key, c: ctypes.c_void_p(dev[key] + 8 * n * c)         # noqa: E731
            lib, h = ctx.lib, ctx.handle
            L, I, F = ctypes.c_long, ctypes.c_int, ctypes.c_double
            nn, mm, dd, lm, z, Rh = L(n), I(m), I(d), F(lam), F(0.0), F(R)
            mean, var, G_new = np.empty((m, n)), np.empty((m, n)), np.empty((m, m))

            def call(name, *args):
                with ctx.lock:
                    Bk.check(ctx, getattr(lib, name)(h, *args), name)

            def gram():
                call("pgps_gp_gram_multi_dev_f64", nn, mm, dd, lm, *mp, Rh, D["t"], D["V"], z, D["gram"], D["logdet"], D["n_obs"])
                ctx.d2h(G_new, dev["gram"])
                ctx.synchronize()
                return G_new

            def device_passes():
                for c in range(m):
                    call("pgps_gp_loo_dev_f64", nn, dd, lm, *mp, Rh, D["t"], col("cols", c), z, col("mean", c), col("var", c), None,
                         None, D["sums"])
                ctx.synchronize()

            def passes():
                device_passes()
                ctx.d2h(mean, dev["mean"])
                ctx.d2h(var, dev["var"])
                ctx.synchronize()
                W = np.where(np.isnan(cols), 0.0, (cols - mean) / np.sqrt(var))
                return W @ W.T

            sides = {"gram": gram, "passes": passes, "device_passes": device_passes}
            try:
                for key, a in host.items():
                    ctx.h2d(dev[key], a)
                G, G_old = np.array(gram()), np.array(passes())             # warm-up of this shape, and the comparison
                dg = np.sqrt(np.diag(G_old))
                err = float(np.max(np.abs(G - G_old) / np.outer(dg, dg)))
                tic = time.perf_counter()
                passes()
                inner = min(200, max(1, int(min_window / max(time.perf_counter() - tic, 1e-6))))
                times = {name: [] for name in sides}
                for _ in range(reps):
                    for name, fn in sides.items():
                        tic = time.perf_counter()
                        for _ in range(inner):
                            fn()
                        times[name].append((time.perf_counter() - tic) / inner)
                row = {"size": size, "kernel": kname, "d": d, "N": n, "columns": m, "calls_per_window": inner,
                       "relerr_against_passes": err}
                for name, vals in times.items():
                    row[name + "_ms"] = [1e3 * min(vals), 1e3 * statistics.median(vals), 1e3 * max(vals)]
                row["ratio"] = row["gram_ms"][1] / row["passes_ms"][1]
                row["ratio_device_passes"] = row["gram_ms"][1] / row["device_passes_ms"][1]
                rows.append(row)
                print(f"{size} {kname} N={n} 1+p={m}: gram {row['gram_ms'][1]:9.4f} ms   {m} one-step-ahead passes + host product "
                      f"{row['passes_ms'][1]:9.4f} ms (the passes alone {row['device_passes_ms'][1]:9.4f} ms)   ratios {row['ratio']:5.3f} "
                      f"{row['ratio_device_passes']:5.3f}   agree {err:.1e}", flush=True)
            finally:
                for ptr in dev.values():
                    ctx.free(ptr)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=list(SIZES), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-window", type=float, default=0.05, help="seconds of calls per timed window, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mean_function_bench.json"))
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
