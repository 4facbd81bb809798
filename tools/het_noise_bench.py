"""Per-observation noise variances: what the `rs` path costs.  The three entry points pgps_gp_ll_het_dev_f64 /
pgps_gp_predict_het_dev_f64 / pgps_gp_ll_grad_adj_het_dev_f64 against their scalar namesakes pgps_gp_dev_f64 (log-likelihood
only) / pgps_gp_predict_dev_f64 / pgps_gp_ll_grad_adj_dev_f64 -- code this library still carries unchanged, so one build serves
both sides.  Like is compared with like: the per-observation calls exist in the three-launch forms only, so the resident launch
and the one-launch forms are switched off (pgps_set_resident(0), pgps_set_one_launch(0)) for the whole run and the scalar side
runs its three-launch forms too.  Device-resident arrays, every call ends in a stream synchronise.

Every shape is warmed up first, the two sides alternate --reps times, medians (with min and max) over windows of at least
--min-window seconds of calls are reported, and the results are compared at the sizes that are timed (s constant = c on the
per-observation side, R + c on the scalar side: the same model).  Writes profiles/het_noise_bench.json and prints a table.

One size per process, every GPU step under its own time limit, chained so that trouble ends the run:

    timeout -k 10 300 python tools/het_noise_bench.py --size small && \\
    timeout -k 10 600 python tools/het_noise_bench.py --size large

small: (N, K) = (4096, 1024); large: (2^20, 2^18).  Matern-3/2 (d = 2) and Matern-5/2 (d = 3)."""
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

SIZES = {"small": (4096, 1024), "large": (2 ** 20, 2 ** 18)}
R, C = 0.1, 0.05


def _model(kname):
    from pssgp import _backend as Bk
    from pssgp.kernels import Matern32, Matern52
    sde = {"m32": Matern32, "m52": Matern52}[kname](1.0, 1.0).get_sde()
    return Bk.nilpotent_form(sde.F), np.asarray(sde.P0), np.asarray(sde.H).reshape(-1)


def _problem(n, k):
    rng = np.random.RandomState(n + k)
    t = np.cumsum(0.05 * (0.5 + rng.rand(n)))
    y = np.sin(0.7 * t) + 0.3 * rng.randn(n)
    y[rng.rand(n) < 0.05] = np.nan
    tq = np.sort(rng.uniform(t[0], t[-1], k))
    return t, y, np.full(n, C), tq


def run(size, reps, min_window):
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    ctx.set_resident(0)
    ctx.set_one_launch(0)
    n, k = SIZES[size]
    rows = []
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)            # noqa: E731
    for kname in ("m32", "m52"):
        form, P, H = _model(kname)
        lam, N1, N2 = form
        d = P.shape[0]
        model = [np.ascontiguousarray(a, np.float64) for a in (N1, N2, P, H)]
        mp = [p(a) for a in model]
        t, y, s, tq = _problem(n, k)
        nout = 1 + d * d + 2 * d + 1
        host = {"t": t, "y": y, "s": s, "tq": tq}
        sizes = {"mean": 8 * k, "var": 8 * k, "ll": 16, "out": 8 * nout, "mean2": 8 * k, "var2": 8 * k, "ll2": 16, "out2": 8 * nout}
        dev = {key: ctx.malloc(a.nbytes) for key, a in host.items()}
        dev.update({key: ctx.malloc(b) for key, b in sizes.items()})
        D = {key: ctypes.c_void_p(ptr) for key, ptr in dev.items()}
        lib, h = ctx.lib, ctx.handle
        L, I, F = ctypes.c_long, ctypes.c_int, ctypes.c_double
        nn, kk, dd, lm, z, Rh, Rs = L(n), L(k), I(d), F(lam), F(0.0), F(R), F(R + C)

        def call(name, *args):
            with ctx.lock:
                Bk.check(ctx, getattr(lib, name)(h, *args), name)
            ctx.synchronize()

        sides = {
            "ll": (lambda: call("pgps_gp_ll_het_dev_f64", nn, dd, lm, *mp, Rh, D["t"], D["y"], D["s"], z, D["ll"]),
                   lambda: call("pgps_gp_dev_f64", nn, dd, lm, *mp, Rs, D["t"], z, D["y"], None, None, None, None, D["ll2"])),
            "predict": (lambda: call("pgps_gp_predict_het_dev_f64", nn, kk, dd, lm, *mp, Rh, D["t"], D["y"], D["s"], z, D["tq"],
                                     D["mean"], D["var"], D["ll"]),
                        lambda: call("pgps_gp_predict_dev_f64", nn, kk, dd, lm, *mp, Rs, D["t"], D["y"], z, D["tq"], D["mean2"],
                                     D["var2"], D["ll2"])),
            "grad": (lambda: call("pgps_gp_ll_grad_adj_het_dev_f64", nn, dd, lm, *mp, Rh, D["t"], z, D["y"], D["s"], D["out"]),
                     lambda: call("pgps_gp_ll_grad_adj_dev_f64", nn, dd, lm, *mp, Rs, D["t"], z, D["y"], D["out2"])),
        }
        try:
            for key, a in host.items():
                ctx.h2d(dev[key], a)
            for what, (het, scalar) in sides.items():
                het(), scalar()                 # warm-up of this shape, and the comparison
                outs = {"ll": ("ll", "ll2", 1), "predict": ("mean", "mean2", k), "grad": ("out", "out2", nout)}[what]
                a, b = np.empty(outs[2]), np.empty(outs[2])
                ctx.d2h(a, dev[outs[0]]), ctx.d2h(b, dev[outs[1]])
                err = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
                tic = time.perf_counter()
                het()
                inner = min(200, max(1, int(min_window / max(time.perf_counter() - tic, 1e-6))))
                times = {"het": [], "scalar": []}
                for _ in range(reps):
                    for name, fn in (("het", het), ("scalar", scalar)):
                        tic = time.perf_counter()
                        for _ in range(inner):
                            fn()
                        times[name].append((time.perf_counter() - tic) / inner)
                row = {"size": size, "kernel": kname, "d": d, "N": n, "K": k, "call": what, "calls_per_window": inner,
                       "relerr_against_scalar": err}
                for name, v in times.items():
                    row[name + "_ms"] = [1e3 * min(v), 1e3 * statistics.median(v), 1e3 * max(v)]
                row["ratio"] = row["het_ms"][1] / row["scalar_ms"][1]
                rows.append(row)
                print(f"{size} {kname} N={n} K={k} {what:8s}: per-observation {row['het_ms'][1]:9.4f} ms   scalar "
                      f"{row['scalar_ms'][1]:9.4f} ms   ratio {row['ratio']:5.3f}   agree {err:.1e}", flush=True)
        finally:
            for ptr in dev.values():
                ctx.free(ptr)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=list(SIZES), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-window", type=float, default=0.05, help="seconds of calls per timed window, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "het_noise_bench.json"))
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
