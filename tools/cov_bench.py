#!/usr/bin/env python3
"""Joint-covariance timings: one JSON line per (d, dtype, N, K) with the time of the gain-product pass
(pgps_pks_cov_gains_dev), of the fill (pgps_cov_fill_dev, projected), of the whole pgps_lti_predict_cov_dev_f64, and on the
same visit of pgps_pks_sample_dev at S = 1 over the same N + K merged steps, of pgps_lti_predict_dev_f64 at the same N, K,
and of the host twin (seconds, one call).  Every device time is the mean of `--reps` back-to-back calls on the context's
stream between two synchronisations, after `--warmup` calls, taken `--repeats` times: [min, median, max] in microseconds,
so the spread between repeats is on the line.  The gain-product call includes its check of the selection (one kernel, a
4-byte copy back and a stream synchronisation) and the slot scatter next to its two scan kernels.  The fill is also given
as bytes stored over time against the 8 TB/s HBM peak.

usage: python tools/cov_bench.py [--reps 10] [--warmup 2] [--repeats 3] [--cases 2,6] [--sizes 65536,1048576] [--queries 1024,8192]
                                 [--out profiles/predict_cov_bench.json] [--no-host]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "parallel-gps_amd")]

from pssgp import _backend  # noqa: E402
from pssgp.kalman.sequential import ks_cov  # noqa: E402
from pssgp.kernels import Matern32, Matern52  # noqa: E402
from pssgp.model import _merge_sorted  # noqa: E402

C = ctypes
HBM_PEAK = 8e12


def model(d):
    if d == 2:
        return Matern32(variance=1.0, lengthscales=0.5)
    if d == 3:
        return Matern52(variance=1.0, lengthscales=0.5)
    return Matern32(variance=1.0, lengthscales=0.5) * Matern52(variance=1.0, lengthscales=0.5)


def timed(ctx, fn, reps, warmup, repeats):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.synchronize()
        out.append((time.perf_counter() - t0) / reps * 1e6)
    out.sort()
    return [round(out[0], 1), round(out[len(out) // 2], 1), round(out[-1], 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default="2,6", help="state dimensions (fp64)")
    ap.add_argument("--sizes", default="65536,1048576", help="training points N")
    ap.add_argument("--queries", default="1024,8192", help="query points K")
    ap.add_argument("--out", default=None, help="also write the lines to this file as a JSON list")
    ap.add_argument("--no-host", action="store_true", help="skip the host twin")
    args = ap.parse_args()
    ctx = _backend.get_context()
    lines = []
    for d in (int(v) for v in args.cases.split(",")):
        sde = model(d).get_sde()
        F, P0, H = (np.ascontiguousarray(np.asarray(a, np.float64)) for a in (sde.F, sde.P0, sde.H))
        H = H.reshape(-1)
        for N in (int(v) for v in args.sizes.split(",")):
            rng = np.random.default_rng(N + d)
            ts = np.cumsum(np.full(N, 0.05))
            ys = np.sin(ts) + 0.3 * rng.standard_normal(N)
            for K in (int(v) for v in args.queries.split(",")):
                tq = np.sort(rng.uniform(ts[0], ts[-1], K))
                all_ts, all_ys, flags = _merge_sorted(ts, tq, (ys, np.full(K, np.nan)), (np.zeros(N, bool), np.ones(K, bool)))
                m = N + K
                sel = np.flatnonzero(flags).astype(np.int64)
                Fs, Qs = _backend.discretise(F, P0, all_ts)
                host = {"ts": ts, "ys": ys, "tq": tq, "Fs": Fs, "Qs": Qs, "P0": P0, "H": H, "ys_m": all_ys, "sel": sel}
                dev = {}
                for k, v in host.items():
                    dev[k] = ctx.malloc(v.nbytes + 256)
                    ctx.h2d(dev[k], v)
                for k, cnt in (("fms", m * d), ("fPs", m * d * d), ("sms", m * d), ("sPs", m * d * d), ("B", K * d * d),
                               ("sPsel", K * d * d), ("cov", K * K), ("mean", K), ("var", K), ("x", m * d), ("ll", 2)):
                    dev[k] = ctx.malloc(cnt * 8 + 256)
                vp = {k: C.c_void_p(v) for k, v in dev.items()}
                cl, ci = C.c_long, C.c_int
                ctx.call("pgps_pkfs_dev_f64", cl(m), ci(d), vp["P0"], vp["Fs"], vp["Qs"], vp["H"], C.c_double(0.1), vp["ys_m"],
                         vp["fms"], vp["fPs"], vp["sms"], vp["sPs"], vp["ll"])
                fPs, sPs = np.empty((m, d, d)), np.empty((m, d, d))
                ctx.d2h(fPs, dev["fPs"])
                ctx.d2h(sPs, dev["sPs"])
                ctx.h2d(dev["sPsel"], np.ascontiguousarray(sPs[sel]))

                def gains():
                    ctx.call("pgps_pks_cov_gains_dev_f64", cl(m), ci(d), vp["Fs"], vp["Qs"], vp["fPs"], cl(K), vp["sel"], vp["B"])

                def fill():
                    ctx.call("pgps_cov_fill_dev_f64", cl(K), ci(d), vp["B"], vp["sPsel"], _backend._ptr(H), vp["cov"])

                def whole():
                    ctx.call("pgps_lti_predict_cov_dev_f64", cl(N), cl(K), ci(d), _backend._ptr(F), _backend._ptr(P0),
                             _backend._ptr(H), C.c_double(0.1), vp["ts"], vp["ys"], C.c_double(0.0), vp["tq"], vp["mean"],
                             vp["cov"], vp["ll"])

                def sample():
                    ctx.call("pgps_pks_sample_dev_f64", cl(m), ci(d), vp["Fs"], vp["Qs"], vp["fms"], vp["fPs"], ci(1), cl(0),
                             C.c_ulonglong(1), None, None, vp["x"])

                def predict():
                    ctx.call("pgps_lti_predict_dev_f64", cl(N), cl(K), ci(d), _backend._ptr(F), _backend._ptr(P0),
                             _backend._ptr(H), C.c_double(0.1), vp["ts"], vp["ys"], C.c_double(0.0), vp["tq"], vp["mean"],
                             vp["var"], vp["ll"])
                t = {name: timed(ctx, fn, args.reps, args.warmup, args.repeats)
                     for name, fn in (("gains", gains), ("fill", fill), ("whole", whole), ("sample_s1", sample), ("predict", predict))}
                cov = np.empty((K, K))
                ctx.d2h(cov, dev["cov"])
                line = {"d": d, "dtype": "f64", "N": N, "K": K, "merged_steps": m,
                        "gains_us": t["gains"], "fill_us": t["fill"], "lti_predict_cov_us": t["whole"],
                        "pks_sample_s1_us": t["sample_s1"], "lti_predict_us": t["predict"],
                        "gains_over_sample_s1": round(t["gains"][1] / t["sample_s1"][1], 2),
                        "input_bytes_per_step_per_phase": 3 * d * d * 8,
                        "fill_bytes_stored": K * K * 8,
                        "fill_GBps": round(K * K * 8 / (t["fill"][1] * 1e-6) / 1e9, 1),
                        "fill_fraction_of_hbm_peak": round(K * K * 8 / (t["fill"][1] * 1e-6) / HBM_PEAK, 3),
                        "symmetric": bool(np.array_equal(cov, cov.T))}
                if not args.no_host:
                    t0 = time.perf_counter()
                    want = ks_cov((None, Fs, Qs), fPs, sPs, sel, H=H)
                    line["host_twin_s"] = round(time.perf_counter() - t0, 3)
                    line["relerr_against_host_twin"] = float(np.max(np.abs(cov - want)) / np.max(np.abs(want)))
                print(json.dumps(line), flush=True)
                lines.append(line)
                for v in dev.values():
                    ctx.free(v)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
