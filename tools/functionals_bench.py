"""Functionals of the state: what pgps_lti_predict_lin_dev_f64 costs at J = 1, 2, 8 rows of C against two baselines.

  (a) pgps_lti_predict_dev_f64 on the same series and queries: the price of the functionals flavour at J = 1 and its growth
      with J (the chains, scans and filter passes are the same launches; only the projecting smoother differs).
  (b) what one had to do before: discretise the MERGED series (pgps_discretise_dev_f64) and run pgps_pkfs_dev_f64 with whole
      filtered and smoothed moments written -- timed alone (a lower bound: the merge is done on the host beforehand and not
      timed), and once more with sms / sPs copied back and  C sm, C sP C^T  formed at the query rows in numpy.

Device-resident arrays, every side ends in ONE stream synchronise ((b)'s two calls share one).  Every shape is warmed up
first, the sides alternate --reps times and medians (with min and max) over windows of at least --min-window seconds are reported; the copy-back variant is
timed once per shape.  The new call's results are compared with (b)'s projection at the sizes that are timed.  Writes
profiles/functionals_bench.json and prints a table.

One size per process, every GPU step under its own time limit, chained so that trouble ends the run:

    timeout -k 10 300 python tools/functionals_bench.py --size small && \\
    timeout -k 10 900 python tools/functionals_bench.py --size large

small: (N, K) = (4096, 1024); large: (2^20, 2^18).  Kernels: m32+m52 (d = 5), the quasi-periodic d = 11 configuration, the CO2
kernel (d = 18)."""
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
R = 0.1
JS = (1, 2, 8)


def _kernels():
    from pssgp.kernels import Matern32, Matern52, Periodic, SquaredExponential
    return {
        "m32+m52": Matern32(1., 0.5) + Matern52(1., 0.5),
        "c5_qp_m52": Periodic(SquaredExponential(1., 1.), period=1., order=1) * Matern32(1., 1.) + Matern52(1., 1.),
        "co2_d18": Periodic(SquaredExponential(1., 1.), period=1., order=3) * Matern32(0.5, 5.) + Matern32(1., 2.),
    }


def _rows(kernel, J):
    """J = 1: H; J = 2: the two additive parts; J = 8: parts, H F and fixed-seed random rows."""
    sde = kernel.get_sde()
    H = np.asarray(sde.H, np.float64).reshape(1, -1)
    if J == 1:
        return H
    comps = kernel.component_functionals()[1]
    if J == 2:
        return comps
    extra = np.random.RandomState(J).randn(J - 3, H.shape[1])
    return np.ascontiguousarray(np.vstack([comps, H @ np.asarray(sde.F, np.float64), extra]))


def _problem(n, k):
    rng = np.random.RandomState(n % (2 ** 31))
    t = np.cumsum(0.05 * (0.5 + rng.rand(n)))
    y = np.sin(0.7 * t) + 0.3 * rng.randn(n)
    tq = np.sort(rng.uniform(t[0], t[-1], k))
    from pssgp.model import _merge_queries
    all_t, all_y, flags = _merge_queries(t, y[:, None], tq)
    return t, y, tq, np.ascontiguousarray(all_t), np.ascontiguousarray(all_y[:, 0]), flags


def _windows(sides, reps, min_window, probe):
    tic = time.perf_counter()
    sides[probe]()
    inner = min(200, max(1, int(min_window / max(time.perf_counter() - tic, 1e-6))))
    times = {name: [] for name in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            tic = time.perf_counter()
            for _ in range(inner):
                fn()
            times[name].append((time.perf_counter() - tic) / inner)
    return inner, {name: [1e3 * min(v), 1e3 * statistics.median(v), 1e3 * max(v)] for name, v in times.items()}


def run(size, reps, min_window):
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    n, k = SIZES[size]
    m = n + k
    rows = []
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)            # noqa: E731
    L, I, F = ctypes.c_long, ctypes.c_int, ctypes.c_double
    t, y, tq, all_t, all_y, flags = _problem(n, k)
    for kname, kernel in _kernels().items():
        sde = kernel.get_sde()
        Fm, Pm, Hm = (np.ascontiguousarray(a, np.float64) for a in (sde.F, sde.P0, np.asarray(sde.H).reshape(-1)))
        d = Fm.shape[0]
        host = {"t": t, "y": y, "tq": tq, "all_t": all_t, "all_y": all_y, "F": Fm, "P": Pm, "H": Hm}
        sizes = {"mean": 8 * k * max(JS), "cov": 8 * k * max(JS) ** 2, "var": 8 * k, "ll": 16,
                 "Fs": 8 * m * d * d, "Qs": 8 * m * d * d, "fPs": 8 * m * d * d, "sPs": 8 * m * d * d, "fms": 8 * m * d, "sms": 8 * m * d}
        dev = {key: ctx.malloc(a.nbytes) for key, a in host.items()}
        dev.update({key: ctx.malloc(b) for key, b in sizes.items()})
        D = {key: ctypes.c_void_p(ptr) for key, ptr in dev.items()}
        lib, h = ctx.lib, ctx.handle

        def call(name, *args, sync=True):
            with ctx.lock:
                Bk.check(ctx, getattr(lib, name)(h, *args), name)
            if sync:
                ctx.synchronize()

        def arrays():               # (two calls on one stream, ONE synchronise: every side ends in exactly one)
            call("pgps_discretise_dev_f64", L(m), I(d), D["F"], D["P"], D["all_t"], F(0.0), D["Fs"], D["Qs"], sync=False)
            call("pgps_pkfs_dev_f64", L(m), I(d), D["P"], D["Fs"], D["Qs"], D["H"], F(R), D["all_y"], D["fms"], D["fPs"], D["sms"],
                 D["sPs"], D["ll"])

        sms, sPs = np.zeros((m, d)), np.zeros((m, d, d))          # (touched here: the timed copy-back pays no page faults)
        sms.fill(0.0)
        sPs.fill(0.0)

        def arrays_projected(C):
            arrays()
            ctx.d2h(sms, dev["sms"])
            ctx.d2h(sPs, dev["sPs"])
            return sms[flags] @ C.T, np.einsum("ia,nab,jb->nij", C, sPs[flags], C)

        try:
            for key, a in host.items():
                ctx.h2d(dev[key], a)
            Cs = {J: _rows(kernel, J) for J in JS}
            sides = {"predict": lambda: call("pgps_lti_predict_dev_f64", L(n), L(k), I(d), p(Fm), p(Pm), p(Hm), F(R), D["t"], D["y"],
                                             F(0.0), D["tq"], D["mean"], D["var"], D["ll"]),
                     "arrays": arrays}
            for J in JS:
                sides[f"lin{J}"] = (lambda J=J: call("pgps_lti_predict_lin_dev_f64", L(n), L(k), I(d), I(J), p(Fm), p(Pm), p(Hm),
                                                     p(Cs[J]), F(R), D["t"], D["y"], F(0.0), D["tq"], D["mean"], D["cov"], D["ll"]))
            for fn in sides.values():           # warm-up of this shape
                fn()
            # the copy-back variant once per J (timed), and the comparison with the new call
            back_ms, err = {}, 0.0
            for J in JS:
                tic = time.perf_counter()
                mean_b, cov_b = arrays_projected(Cs[J])
                back_ms[J] = 1e3 * (time.perf_counter() - tic)
                sides[f"lin{J}"]()
                mean, cov = np.empty((k, J)), np.empty((k, J, J))
                ctx.d2h(mean, dev["mean"])
                ctx.d2h(cov, dev["cov"])
                err = max(err, float(np.max(np.abs(mean - mean_b)) / max(1.0, np.max(np.abs(mean_b)))),
                          float(np.max(np.abs(cov - cov_b)) / max(1.0, np.max(np.abs(cov_b)))))
            inner, ms = _windows(sides, reps, min_window, "predict")
            row = {"size": size, "kernel": kname, "d": d, "N": n, "K": k, "calls_per_window": inner, "relerr_against_arrays": err}
            row.update({name + "_ms": v for name, v in ms.items()})
            for J in JS:
                row[f"arrays_copied_back_J{J}_ms"] = back_ms[J]
                row[f"ratio_lin{J}_predict"] = ms[f"lin{J}"][1] / ms["predict"][1]
                row[f"ratio_lin{J}_arrays"] = ms[f"lin{J}"][1] / ms["arrays"][1]
            rows.append(row)
            print(f"{size} {kname} d={d} N={n} K={k}: predict {ms['predict'][1]:9.4f} ms   arrays {ms['arrays'][1]:9.4f} ms   "
                  + "   ".join(f"J={J} {ms[f'lin{J}'][1]:9.4f} ms (x{row[f'ratio_lin{J}_predict']:5.3f} predict, "
                               f"x{row[f'ratio_lin{J}_arrays']:5.3f} arrays; copied back {back_ms[J]:9.1f} ms)" for J in JS)
                  + f"   agree {err:.1e}", flush=True)
        finally:
            for ptr in dev.values():
                ctx.free(ptr)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=list(SIZES), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-window", type=float, default=0.05, help="seconds of calls per timed window, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "functionals_bench.json"))
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
