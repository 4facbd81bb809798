"""Phase stamps of the resident launch (csrc/pgps_resident.hip.h) at 2^20 steps, array and fused form, with the per-wave
split of the reduce and Kalman-pass ends (libraries that have pgps_resident_wave_stamps).  Medians over the workgroups of
one launch, for `--reps` launches.   PGPS_LIB=<library> python tools/res_stamps.py [--reps 3] [--no-filtered]

--no-filtered: the fused form without the filtered outputs (fms, fPs not requested: the Kalman pass then stores nothing; the
array entry point always returns them) -- what the pass costs without its stores.

Stamps (slots of resident_stamps(), wave 0 lane 0): 0 start, 1 reduce done, 2 forward scan done (and, where the total is
published from inside the scan, published), 3 carry in, 4 applied, 5 Kalman pass + last element done, 6 suffix scan done,
7 carry in, 8 applied, 9 end; 14 (between 5 and 6) the head of the suffix scan: 5 -> 14 is whatever of the lane's smoothing
aggregate the compiler has left behind the Kalman pass, 14 -> 6 the scan itself.  The rows "scan ... wait"
are the part of the launch in which the memory path idles: (3 - 1) + (7 - 5)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "parallel-gps_amd"), os.path.join(ROOT, "tools")]
from res_check import series                # noqa: E402
from oracle import np_oracle as O           # noqa: E402
from pssgp import _backend as B             # noqa: E402
from pssgp.kernels import Matern32          # noqa: E402


def table(st, ws):
    d = lambda a, b: np.median(st[:, b] - st[:, a])            # noqa: E731
    rows = [("load+reduce", d(0, 1)), ("forward scan (+publish)", d(1, 2)), ("wait left neighbour", d(2, 3)),
            ("fold+apply", d(3, 4)), ("kalman pass", d(4, 5)), ("suffix scan (+publish)", d(5, 6)),
            ("ll + wait right neighbour", d(6, 7)), ("fold+apply", d(7, 8)), ("rts pass", d(8, 9))]
    out = [f"    {n:28s} {v:9.0f}" for n, v in rows]
    if np.all((st[:, 14] >= st[:, 5]) & (st[:, 14] <= st[:, 6])):
        # libraries with the diagnostic stamp in front of the suffix scan (slot 14): what stands between the pass and the scan
        out[6:6] = [f"    {'  aggregate block (5->14)':28s} {d(5, 14):9.0f}", f"    {'  scan proper (14->6)':28s} {d(14, 6):9.0f}",
                    f"    {'kalman + aggregate + suffix':28s} {d(4, 6):9.0f}"]
    out.append(f"    {'scan + hand-off (1->3, 5->7)':28s} {d(1, 3) + d(5, 7):9.0f}")
    out.append(f"    {'total':28s} {d(0, 9):9.0f}")
    if ws is not None:
        red, kal = ws[:, 0:4], ws[:, 4:8]
        out.append("    per wave (median over workgroups; wave 0 .. 3):")
        out.append("      reduce end - start      " + " ".join(f"{np.median(red[:, w] - st[:, 0]):8.0f}" for w in range(4)))
        out.append("      kalman end - applied    " + " ".join(f"{np.median(kal[:, w] - st[:, 4]):8.0f}" for w in range(4)))
        out.append(f"      forward scan from the slowest wave   {np.median(st[:, 2] - red.max(axis=1)):8.0f}"
                   f"   (wave imbalance {np.median(red.max(axis=1) - red.min(axis=1)):.0f})")
        out.append(f"      suffix scan from the slowest wave    {np.median(st[:, 6] - kal.max(axis=1)):8.0f}"
                   f"   (wave imbalance {np.median(kal.max(axis=1) - kal.min(axis=1)):.0f})")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-filtered", action="store_true", help="fused form only, filtered outputs not requested")
    args = ap.parse_args()
    ctx = B.get_context(0)
    kern = Matern32(variance=1.0, lengthscales=1.0)
    sde = kern.get_sde()
    lam, N1, N2 = B.nilpotent_form(sde.F)
    n = 1 << 20
    t, y = series(n, seed=1)
    P0, Fs, Qs, H, R = tuple(np.asarray(a, np.float64) for a in O.get_ssm(sde, t, 0.1))
    arrs = dict(P0=P0.reshape(-1), Fs=Fs.reshape(-1), Qs=Qs.reshape(-1), H=np.asarray(H, np.float64).reshape(-1), ys=y, ts=t)
    dev = {}
    for k, v in arrs.items():
        v = np.ascontiguousarray(v, np.float64)
        dev[k] = ctx.malloc(v.nbytes)
        ctx.h2d(dev[k], v)
    for k, sz in (("fms", 2), ("fPs", 4), ("sms", 2), ("sPs", 4)):
        dev[k] = ctx.malloc(n * sz * 8)
    dev["ll"] = ctx.malloc(8)
    N1 = np.ascontiguousarray(N1, np.float64)
    N2 = np.ascontiguousarray(N2, np.float64)
    Pinf = np.ascontiguousarray(sde.P0, np.float64)
    Hh = np.ascontiguousarray(sde.H.reshape(-1), np.float64)
    from ctypes import c_double, c_int, c_long

    def run_array():
        ctx.call("pgps_pkfs_dev_f64", c_long(n), c_int(2), dev["P0"], dev["Fs"], dev["Qs"], dev["H"],
                 c_double(float(np.asarray(R).reshape(-1)[0])), dev["ys"], dev["fms"], dev["fPs"], dev["sms"], dev["sPs"], dev["ll"])

    def run_fused():
        fms, fPs = (None, None) if args.no_filtered else (dev["fms"], dev["fPs"])
        ctx.call("pgps_gp_dev_f64", c_long(n), c_int(2), c_double(lam), B._ptr(N1), B._ptr(N2), B._ptr(Pinf), B._ptr(Hh),
                 c_double(0.1), dev["ts"], c_double(0.0), dev["ys"], fms, fPs, dev["sms"], dev["sPs"], dev["ll"])

    has_waves = hasattr(ctx.lib, "pgps_resident_wave_stamps")
    print(f"library {B._LIB_PATH}, per-wave stamps: {'yes' if has_waves else 'no'}")
    ctx.set_resident(2)
    forms = (("fused, no filtered outputs", run_fused),) if args.no_filtered else (("array", run_array), ("fused", run_fused))
    for name, fn in forms:
        for _ in range(10):
            fn()
        ctx.synchronize()
        for r in range(args.reps):
            fn()
            ctx.synchronize()
            assert ctx.status() == 0
            st = ctx.resident_stamps()
            ws = ctx.resident_wave_stamps() if has_waves else None
            print(f"{name} launch {r}: phase stamps (cycles, median over {st.shape[0]} workgroups)")
            print(table(st, ws), flush=True)
    ctx.set_resident(-1)


if __name__ == "__main__":
    main()
