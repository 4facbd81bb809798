"""The predictive checks of a panel of S series -- pgps_gp_panel_loo_dev_f64 on the concatenated, device-resident series, one
workgroup per series, one launch per group -- against what a user could do without it.  Two variants of a pass over all S
series: "scores" (the two sums per series, no per-row array) and "arrays" (the four per-row arrays as well).

Baselines.  Scalar noise: the loop of S pgps_gp_loo_dev_f64 calls on slices of the same resident arrays, queued back to back
and synchronised once per pass.  Per-observation variances `rs`: no device call existed -- the single model sends such data to
its sequential host twin -- so the baseline is the MODEL-LEVEL loop of StateSpaceGP host twins (loo_log_predictive_density for
"scores"; one_step_ahead and leave_one_out for "arrays"), timed ONCE and at S = 64 only, and labelled as such.

The protocol is tools/panel_bench.py's: the same four panels, every shape warmed up first, the two sides alternating --reps
times, medians (with min and max) over windows of at least --min-window seconds, every pass ending in one stream synchronise;
the sums of the two sides are compared at the sizes that are timed.  Writes profiles/panel_checks_bench.json and prints a table.

One size per process, every GPU step under its own time limit, chained so that trouble ends the run:

    timeout -k 10 120 python tools/panel_checks_bench.py --size s64 && timeout -k 10 200 python tools/panel_checks_bench.py --size s1024 && \\
    timeout -k 10 500 python tools/panel_checks_bench.py --size s8192 && timeout -k 10 200 python tools/panel_checks_bench.py --size full2048
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-gps_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from panel_bench import R, SIZES, _model, _problem, _timed  # noqa: E402


def _host_twins(cases, kname, arrays):
    """Seconds of ONE pass of the model-level loop over `cases` with observation_variances (the single model's host twin)."""
    from pssgp.kernels import Matern32, Matern52
    from pssgp.model import StateSpaceGP
    kernel = {"m32": Matern32, "m52": Matern52}[kname](1.0, 1.0)
    models = [StateSpaceGP((t[:, None], y[:, None]), kernel, noise_variance=R, parallel=True, observation_variances=s)
              for t, y, s, _ in cases]
    tic = time.perf_counter()
    scores = []
    for m in models:
        if arrays:
            m.one_step_ahead()
            scores.append(float(np.nansum(m.leave_one_out()[2])))
        else:
            scores.append(float(m.loo_log_predictive_density()))
    return time.perf_counter() - tic, np.asarray(scores)


def run(size, reps, min_window):
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    lib, h = ctx.lib, ctx.handle
    L, I, F, P = ctypes.c_long, ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(P)                          # noqa: E731
    rows = []
    cases = _problem(size, False)
    S = SIZES[size]
    offs = np.concatenate([[0], np.cumsum([c[0].size for c in cases])]).astype(np.int64)
    n = int(offs[-1])
    host = {"t": np.concatenate([c[0] for c in cases]), "y": np.concatenate([c[1] for c in cases]),
            "s": np.concatenate([c[2] for c in cases])}
    dev = {key: ctx.malloc(a.nbytes) for key, a in host.items()}
    dev.update({key: ctx.malloc(b) for key, b in (("rows", 8 * 4 * n), ("sums", 8 * 2 * S), ("rows2", 8 * 4 * n), ("sums2", 8 * 2 * S))})
    try:
        for key, a in host.items():
            ctx.h2d(dev[key], a)

        def call(name, *args):
            with ctx.lock:
                Bk.check(ctx, getattr(lib, name)(h, *args), name)

        for kname in ("m32", "m52"):
            form, Pinf, H = _model(kname)
            lam, N1, N2 = form
            d = Pinf.shape[0]
            table, _ = Bk._gp_rows([(form, Pinf, H, R)])
            model = [np.ascontiguousarray(a, np.float64) for a in (N1, N2, Pinf, H)]
            mp = [p(a) for a in model]
            for het in (False, True):
                for arrays in (False, True):
                    rs = P(dev["s"]) if het else None
                    out = [P(dev["rows"] + 8 * n * i) if arrays else None for i in range(4)]

                    def panel():
                        call("pgps_gp_panel_loo_dev_f64", L(S), p(offs), I(d), I(1), p(table), P(dev["t"]), P(dev["y"]), rs, *out,
                             P(dev["sums"]))
                        ctx.synchronize()

                    z, lm, Rh, dd = F(0.0), F(lam), F(R), I(d)
                    at = lambda key, i, stride=1: P(dev[key] + 8 * stride * int(i))        # noqa: E731

                    def loop():
                        for i in range(S):
                            o = offs[i]
                            per = [P(dev["rows2"] + 8 * (n * j + int(o))) if arrays else None for j in range(4)]
                            call("pgps_gp_loo_dev_f64", L(int(offs[i + 1] - o)), dd, lm, *mp, Rh, at("t", o), at("y", o),
                                 F(float(host["t"][o])), *per, at("sums2", i, 2))
                        ctx.synchronize()

                    what = "arrays" if arrays else "scores"
                    row = {"size": size, "S": S, "rows": n, "kernel": kname, "d": d, "rs": het, "pass": what}
                    panel()
                    a = np.empty(2 * S)
                    ctx.d2h(a, dev["sums"])
                    if not het:
                        loop()
                        b = np.empty(2 * S)
                        ctx.d2h(b, dev["sums2"])
                        ms, inner = _timed({"panel": panel, "loop": loop}, reps, min_window)
                        row.update(baseline=f"loop of {S} pgps_gp_loo_dev_f64 calls, one synchronise per pass",
                                   relerr_sums_against_baseline=float(np.max(np.abs(a - b) / np.abs(b))), passes_per_window=inner,
                                   panel_ms=ms["panel"], baseline_ms=ms["loop"], speedup=ms["loop"][1] / ms["panel"][1])
                    else:
                        ms, inner = _timed({"panel": panel}, reps, min_window)
                        row.update(baseline=None, passes_per_window=inner, panel_ms=ms["panel"], baseline_ms=None, speedup=None)
                        if size == "s64":
                            sec, scores = _host_twins(cases, kname, arrays)
                            row.update(baseline="MODEL-LEVEL loop of 64 StateSpaceGP host twins (no device call existed), timed ONCE",
                                       relerr_sums_against_baseline=float(np.max(np.abs(a[1::2] - scores) / np.abs(scores))),
                                       baseline_ms=[1e3 * sec] * 3, speedup=1e3 * sec / ms["panel"][1])
                    rows.append(row)
                    base = "            -" if row["baseline_ms"] is None else f"{row['baseline_ms'][1]:13.4f}"
                    ratio = "      -" if row["speedup"] is None else f"{row['speedup']:7.2f}"
                    agree = "" if "relerr_sums_against_baseline" not in row else f"   agree {row['relerr_sums_against_baseline']:.1e}"
                    print(f"{size} {kname} rs={int(het)} {what:6s}: panel {row['panel_ms'][1]:10.4f} ms   baseline {base} ms   "
                          f"baseline / panel {ratio}{agree}", flush=True)
    finally:
        for ptr in dev.values():
            ctx.free(ptr)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=list(SIZES), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-window", type=float, default=0.05, help="seconds of calls per timed window, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_checks_bench.json"))
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
