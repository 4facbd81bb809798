#!/usr/bin/env python3
"""Backward-sampler timings: one JSON line per (d, dtype, N, S) with the time of pgps_pkf_dev and of
pgps_pks_sample_dev with the library's draws (z = NULL) and with z supplied, the input bytes one sampler phase reads per
step, and the host twin's steps/s.  Times are the mean of `--reps` back-to-back calls on the context's stream between two
synchronisations, after `--warmup` calls.

usage: python tools/sample_bench.py [--reps 20] [--warmup 3] [--quick] [--cases 2:f64,6:f64] [--samples 1,16] [--label NAME]

To compare two builds of the library, run the tool once per build (PGPS_LIB=<path to the other libpgps.so>) in alternation
and tell the lines apart by --label."""
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
from pssgp.kalman.sequential import ks_sample  # noqa: E402
from pssgp.kernels import Matern32, Matern52  # noqa: E402

C = ctypes


def model(d):
    if d == 2:
        return Matern32(variance=1.0, lengthscales=0.5)
    if d == 3:
        return Matern52(variance=1.0, lengthscales=0.5)
    return Matern32(variance=1.0, lengthscales=0.5) * Matern52(variance=1.0, lengthscales=0.5)


def timed(ctx, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="N = 2^16 only")
    ap.add_argument("--cases", default="2:f64,3:f64,6:f32", help="d:dtype pairs")
    ap.add_argument("--samples", default="1,4,16,64", help="sample counts S")
    ap.add_argument("--full-only", action="store_true", help="N = 2^20 only")
    ap.add_argument("--label", default=None, help="copied into every output line")
    args = ap.parse_args()
    ctx = _backend.get_context()
    cases = [(int(c.split(":")[0]), {"f64": np.float64, "f32": np.float32}[c.split(":")[1]]) for c in args.cases.split(",")]
    for d, dt in cases:
        suf, real = _backend._suffix(dt)
        sde = model(d).get_sde()
        for N in ((1 << 16,) if args.quick else (1 << 20,) if args.full_only else (1 << 16, 1 << 20)):
            ts = np.cumsum(np.full(N, 0.05))
            Fs, Qs = _backend.discretise(np.asarray(sde.F, np.float64), np.asarray(sde.P0, np.float64), ts)
            host = {"Fs": Fs.astype(dt), "Qs": Qs.astype(dt), "P0": np.asarray(sde.P0, dt), "H": np.asarray(sde.H, dt).reshape(-1),
                    "ys": np.sin(ts).astype(dt)}
            dev = {}
            for k, v in host.items():
                dev[k] = ctx.malloc(v.nbytes + 256)
                ctx.h2d(dev[k], v)
            dev["fms"] = ctx.malloc(N * d * dt().itemsize + 256)
            dev["fPs"] = ctx.malloc(N * d * d * dt().itemsize + 256)
            vp = {k: C.c_void_p(v) for k, v in dev.items()}

            def pkf():
                ctx.call(f"pgps_pkf_dev_{suf}", C.c_long(N), C.c_int(d), vp["P0"], vp["Fs"], vp["Qs"], vp["H"], real(1.0),
                         vp["ys"], vp["fms"], vp["fPs"], None)
            t_pkf = timed(ctx, pkf, args.reps, args.warmup)
            fms, fPs = np.empty((N, d), dt), np.empty((N, d, d), dt)
            ctx.d2h(fms, dev["fms"])
            ctx.d2h(fPs, dev["fPs"])
            t = time.perf_counter()
            ks_sample((None, host["Fs"][:4096], host["Qs"][:4096]), fms[:4096], fPs[:4096], 1, 1)
            host_rate = 4096 / (time.perf_counter() - t)
            for S in (int(v) for v in args.samples.split(",")):
                z = ctx.malloc(S * N * d * dt().itemsize + 256)
                out = ctx.malloc(S * N * d * dt().itemsize + 256)
                ctx.call(f"pgps_sample_normals_dev_{suf}", C.c_long(N), C.c_int(d), C.c_int(S), C.c_long(0), C.c_ulonglong(1),
                         C.c_void_p(z))

                def run(zp):
                    ctx.call(f"pgps_pks_sample_dev_{suf}", C.c_long(N), C.c_int(d), vp["Fs"], vp["Qs"], vp["fms"], vp["fPs"],
                             C.c_int(S), C.c_long(0), C.c_ulonglong(1), zp, None, C.c_void_p(out))
                t_draw = timed(ctx, lambda: run(None), args.reps, args.warmup)
                t_z = timed(ctx, lambda: run(C.c_void_p(z)), args.reps, args.warmup)
                isz = dt().itemsize
                print(json.dumps({**({"label": args.label} if args.label else {}), "d": d, "dtype": suf, "N": N, "S": S, "pkf_us": round(t_pkf, 1),
                                  "sample_us": round(t_draw, 1), "sample_z_us": round(t_z, 1),
                                  "input_bytes_per_step_per_phase": (2 * d * d + d + d * d) * isz,
                                  "group_passes": 2 * -(-S // (8 if d <= 2 else 4 if d <= 4 else 2)),
                                  "host_twin_steps_per_s": round(host_rate)}), flush=True)
                ctx.free(z)
                ctx.free(out)
            for v in dev.values():
                ctx.free(v)


if __name__ == "__main__":
    main()
