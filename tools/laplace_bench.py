"""Laplace inference: what ONE Newton pass on device-resident arrays costs (pgps_gp_newton_dev_f64 and the six sums brought
back) against what a user had to do without it: pgps_gp_predict_het_dev_f64 with the training times as the query times (tq = ts,
K = N: a merge, a filter + smoother over 2N steps), three copies back (mean, var, ll), the site update in numpy and two copies
up (zs, ss).  The device part of that alone (the predict call and a synchronise) is timed too: a lower bound of any host-side
loop.  bench.py does not call this.  Both sides exist in the multi-launch form only; the resident launch and the one-launch
forms are switched off for the whole run.

Every shape is warmed up first, the sides alternate --reps times, medians (with min and max) over windows of at least
--min-window seconds of calls are reported, and the new iterate of both sides is compared at the sizes that are timed.  Writes
profiles/laplace_bench.json and prints a table.

One size per process, every GPU step under its own time limit, chained so that trouble ends the run:

    timeout -k 10 300 python tools/laplace_bench.py --size small && \\
    timeout -k 10 600 python tools/laplace_bench.py --size large

small: N = 4096; large: N = 2^20.  Matern-3/2 (d = 2) and Matern-5/2 (d = 3), Bernoulli and Poisson observations."""
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
ARRAYS = ("f", "v", "alpha", "zs_new", "ss_new")


def _model(kname):
    from pssgp import _backend as Bk
    from pssgp.kernels import Matern32, Matern52
    sde = {"m32": Matern32, "m52": Matern52}[kname](1.0, 1.0).get_sde()
    return Bk.nilpotent_form(sde.F), np.asarray(sde.P0), np.asarray(sde.H).reshape(-1)


def _problem(n, lik):
    rng = np.random.RandomState(n)
    t = np.cumsum(0.05 * (0.5 + rng.rand(n)))
    latent = np.sin(0.7 * t)
    y = (rng.rand(n) < 1.0 / (1.0 + np.exp(-2.0 * latent))).astype(float) if lik.name == "Bernoulli" else rng.poisson(2.0 * np.exp(latent)).astype(float)
    y[rng.rand(n) < 0.05] = np.nan
    return t, y


def _sites(lik, y, f):
    """The numpy site update of the baseline: (zs, ss) at f, NaN / 1 at the missing rows."""
    obs = ~np.isnan(y)
    _, g, W, _ = lik.log_prob_derivs(np.where(obs, y, 0.0), f)
    return np.where(obs, f + g / W, np.nan), np.where(obs, 1.0 / W, 1.0)


def run(size, reps, min_window):
    from pssgp import _backend as Bk
    from pssgp.likelihoods import Bernoulli, Poisson
    ctx = Bk.get_context()
    ctx.set_resident(0)
    ctx.set_one_launch(0)
    n = SIZES[size]
    rows = []
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)            # noqa: E731
    for kname in ("m32", "m52"):
        for lik in (Bernoulli(), Poisson(1.0)):
            form, P, H = _model(kname)
            lam, N1, N2 = form
            d = P.shape[0]
            mp = [p(a) for a in [np.ascontiguousarray(a, np.float64) for a in (N1, N2, P, H)]]
            t, y = _problem(n, lik)
            f0 = 0.3 * np.sin(t)
            zs, ss = _sites(lik, y, f0)
            host = {"t": t, "y": y, "zs": zs, "ss": ss, "f0": f0}
            sizes = {f: 8 * n for f in ARRAYS + ("mean", "var")}
            sizes.update({"sums": 64, "ll": 16})
            dev = {key: ctx.malloc(a.nbytes) for key, a in host.items()}
            dev.update({key: ctx.malloc(b) for key, b in sizes.items()})
            D = {key: ctypes.c_void_p(ptr) for key, ptr in dev.items()}
            lib, h = ctx.lib, ctx.handle
            L, I, F = ctypes.c_long, ctypes.c_int, ctypes.c_double
            nn, dd, lm, z = L(n), I(d), F(lam), F(0.0)
            sums, mean, var, ll = np.zeros(8), np.empty(n), np.empty(n), np.zeros(2)

            def call(name, *args):
                with ctx.lock:
                    Bk.check(ctx, getattr(lib, name)(h, *args), name)

            def newton():
                call("pgps_gp_newton_dev_f64", nn, dd, lm, *mp, I(lik.lik_id), F(lik.par), D["t"], D["y"], D["zs"], D["ss"], D["f0"], z,
                     *(D[a] for a in ARRAYS), D["sums"])
                ctx.d2h(sums, dev["sums"])

            def predict():
                call("pgps_gp_predict_het_dev_f64", nn, nn, dd, lm, *mp, z, D["t"], D["zs"], D["ss"], z, D["t"], D["mean"], D["var"], D["ll"])

            def baseline_device():
                predict()
                ctx.synchronize()

            def baseline():
                predict()
                ctx.d2h(mean, dev["mean"])
                ctx.d2h(var, dev["var"])
                ctx.d2h(ll, dev["ll"])
                z_new, s_new = _sites(lik, y, mean)
                ctx.h2d(dev["zs_new"], z_new)           # (into the spare arrays: every window starts from the same sites)
                ctx.h2d(dev["ss_new"], s_new)

            sides = {"newton": newton, "baseline": baseline, "baseline_device": baseline_device}
            try:
                for key, a in host.items():
                    ctx.h2d(dev[key], a)
                for fn in (baseline, newton):       # warm-up of this shape, and the comparison (newton last: it owns the arrays)
                    fn()
                baseline_device()
                newton()
                got = {key: np.empty(n) for key in ("f", "v")}
                for key, a in got.items():
                    ctx.d2h(a, dev[key])
                err = max(float(np.max(np.abs(got["f"] - mean)) / np.max(np.abs(mean))), float(np.max(np.abs(got["v"] - var)) / np.max(np.abs(var))),
                          abs(sums[0] - ll[0]) / abs(ll[0]))
                tic = time.perf_counter()
                baseline()
                inner = min(200, max(1, int(min_window / max(time.perf_counter() - tic, 1e-6))))
                times = {name: [] for name in sides}
                for _ in range(reps):
                    for name, fn in sides.items():
                        tic = time.perf_counter()
                        for _ in range(inner):
                            fn()
                        times[name].append((time.perf_counter() - tic) / inner)
                row = {"size": size, "kernel": kname, "d": d, "likelihood": lik.name, "N": n, "calls_per_window": inner,
                       "relerr_against_predict": err}
                for name, vals in times.items():
                    row[name + "_ms"] = [1e3 * min(vals), 1e3 * statistics.median(vals), 1e3 * max(vals)]
                row["ratio_baseline"] = row["newton_ms"][1] / row["baseline_ms"][1]
                row["ratio_baseline_device"] = row["newton_ms"][1] / row["baseline_device_ms"][1]
                rows.append(row)
                print(f"{size} {kname} {lik.name:9s} N={n}: Newton pass {row['newton_ms'][1]:9.4f} ms   baseline {row['baseline_ms'][1]:9.4f} ms   "
                      f"its device part {row['baseline_device_ms'][1]:9.4f} ms   ratios {row['ratio_baseline']:5.3f} "
                      f"{row['ratio_baseline_device']:5.3f}   agree {err:.1e}", flush=True)
            finally:
                for ptr in dev.values():
                    ctx.free(ptr)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=list(SIZES), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-window", type=float, default=0.05, help="seconds of calls per timed window, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laplace_bench.json"))
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
