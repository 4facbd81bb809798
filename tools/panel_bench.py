"""A panel of S series against the loop of S single-series calls.  The panel side: pgps_gp_panel_ll_dev_f64 /
pgps_gp_panel_ll_grad_dev_f64 / pgps_gp_panel_predict_dev_f64 on the concatenated, device-resident series (one workgroup per
series, one launch per group).  The baseline is the fastest thing a user could do without them: every series resident on the
device already and one call per series -- Series.gp_ll / Series.gp_ll_grad_adj_raw / Series.gp_predict (query grid merged once,
at set_queries) for scalar noise; with per-observation variances `rs` the device-pointer entry points pgps_gp_ll_het_dev_f64 /
pgps_gp_ll_grad_adj_het_dev_f64 / pgps_gp_predict_het_dev_f64 on slices of the same resident arrays, queued back to back and
synchronised once per pass.  Every timed pass ends in a stream synchronise.

Every shape is warmed up first, the two sides alternate --reps times, medians (with min and max) over windows of at least
--min-window seconds are reported, and the log-likelihoods of the two sides are compared at the sizes that are timed.  Writes
profiles/panel_bench.json and prints a table.

One size per process, every GPU step under its own time limit, chained so that trouble ends the run:

    timeout -k 10 120 python tools/panel_bench.py --size s64 && timeout -k 10 200 python tools/panel_bench.py --size s1024 && \\
    timeout -k 10 500 python tools/panel_bench.py --size s8192 && timeout -k 10 200 python tools/panel_bench.py --size full2048

s64, s1024, s8192: S series with lengths uniform in [100, 1000]; full2048: 256 series of 2048 points (the limit; its predict has
1536 points and 512 queries per series).  Predict asks for K_i = n_i / 4 queries.  Matern-3/2 (d = 2) and Matern-5/2 (d = 3)."""
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

SIZES = {"s64": 64, "s1024": 1024, "s8192": 8192, "full2048": 256}
R = 0.1


def _model(kname):
    from pssgp import _backend as Bk
    from pssgp.kernels import Matern32, Matern52
    sde = {"m32": Matern32, "m52": Matern52}[kname](1.0, 1.0).get_sde()
    return Bk.nilpotent_form(sde.F), np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1)


def _problem(size, predict):
    """[(t, y, s, tq)]: irregular times, a noisy sine, 5 % missing, s log-uniform over two decades."""
    rng = np.random.RandomState(len(size) + SIZES[size])
    out = []
    for _ in range(SIZES[size]):
        n = (1536 if predict else 2048) if size == "full2048" else int(rng.randint(100, 1001))
        k = 512 if size == "full2048" else n // 4
        t = np.cumsum(0.05 * (0.5 + rng.rand(n)))
        y = np.sin(0.7 * t) + 0.3 * rng.randn(n)
        y[rng.rand(n) < 0.05] = np.nan
        y[0] = 0.1
        out.append((t, y, R * 10.0 ** rng.uniform(-2.0, 0.0, n), np.sort(rng.uniform(t[0], t[-1], k))))
    return out


def _timed(sides, reps, min_window):
    """({name: [min, median, max] ms per pass}, {name: passes per window}) of the alternating sides; every side repeats its
    pass until its own window lasts min_window seconds."""
    inner = {}
    for name, fn in sides.items():
        fn()
        tic = time.perf_counter()
        fn()
        inner[name] = min(200, max(1, int(min_window / max(time.perf_counter() - tic, 1e-6))))
    times = {name: [] for name in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            tic = time.perf_counter()
            for _ in range(inner[name]):
                fn()
            times[name].append((time.perf_counter() - tic) / inner[name])
    return {name: [1e3 * min(v), 1e3 * statistics.median(v), 1e3 * max(v)] for name, v in times.items()}, inner


def run(size, reps, min_window):
    from pssgp import _backend as Bk
    ctx = Bk.get_context()
    lib, h = ctx.lib, ctx.handle
    L, I, F, P = ctypes.c_long, ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(P)                          # noqa: E731
    rows = []
    problems = {False: _problem(size, False), True: _problem(size, True)}
    S = SIZES[size]
    resident = {}                                              # the baseline's resident series, made once per data set
    for kname in ("m32", "m52"):
        form, Pinf, H = _model(kname)
        lam, N1, N2 = form
        d = Pinf.shape[0]
        nout = 2 + d * d + 2 * d
        table, _ = Bk._gp_rows([(form, Pinf, H, R)])
        packed = Bk.Series.pack(form, Pinf, H)
        model = [np.ascontiguousarray(a, np.float64) for a in (N1, N2, Pinf, H)]
        mp = [p(a) for a in model]
        for het in (False, True):
            for what in ("ll", "grad", "predict"):
                cases = problems[what == "predict"]
                offs = np.concatenate([[0], np.cumsum([c[0].size for c in cases])]).astype(np.int64)
                qoffs = np.concatenate([[0], np.cumsum([c[3].size for c in cases])]).astype(np.int64)
                K = int(qoffs[-1])
                host = {"t": np.concatenate([c[0] for c in cases]), "y": np.concatenate([c[1] for c in cases]),
                        "s": np.concatenate([c[2] for c in cases]), "tq": np.concatenate([c[3] for c in cases])}
                dev = {key: ctx.malloc(a.nbytes) for key, a in host.items()}
                dev.update({key: ctx.malloc(b) for key, b in (("out", 8 * S * nout), ("mean", 8 * K), ("var", 8 * K), ("ll", 8 * S),
                                                               ("out2", 8 * S * nout), ("mean2", 8 * K), ("var2", 8 * K), ("ll2", 8 * S))})
                try:
                    for key, a in host.items():
                        ctx.h2d(dev[key], a)
                    rs = P(dev["s"]) if het else None

                    def call(name, *args):
                        with ctx.lock:
                            Bk.check(ctx, getattr(lib, name)(h, *args), name)

                    def panel():
                        if what == "ll":
                            call("pgps_gp_panel_ll_dev_f64", L(S), p(offs), I(d), I(1), p(table), P(dev["t"]), P(dev["y"]), rs, P(dev["ll"]))
                        elif what == "grad":
                            call("pgps_gp_panel_ll_grad_dev_f64", L(S), p(offs), I(d), I(1), p(table), P(dev["t"]), P(dev["y"]), rs,
                                 P(dev["out"]))
                        else:
                            call("pgps_gp_panel_predict_dev_f64", L(S), p(offs), p(qoffs), I(d), I(1), p(table), P(dev["t"]), P(dev["y"]),
                                 rs, P(dev["tq"]), P(dev["mean"]), P(dev["var"]), P(dev["ll"]))
                        ctx.synchronize()

                    ll_loop = np.empty(S)
                    if not het:
                        if (what == "predict") not in resident:
                            group = resident[what == "predict"] = []
                            for t, y, _, tq in cases:
                                group.append(Bk.Series(t, y))
                                if what == "predict":
                                    group[-1].set_queries(tq)
                        series = resident[what == "predict"]

                        def loop():
                            for i, ser in enumerate(series):
                                if what == "ll":
                                    ll_loop[i] = ser.gp_ll(packed, R)
                                elif what == "grad":
                                    ll_loop[i] = ser.gp_ll_grad_adj_raw(packed, R)[0]
                                else:
                                    ll_loop[i] = ser.gp_predict(packed, R)[2]
                    else:
                        z, lm, Rh, dd = F(0.0), F(lam), F(R), I(d)
                        at = lambda key, i, stride=1: P(dev[key] + 8 * stride * int(i))        # noqa: E731

                        def loop():
                            for i in range(S):
                                o, q, n = offs[i], qoffs[i], L(int(offs[i + 1] - offs[i]))
                                if what == "ll":
                                    call("pgps_gp_ll_het_dev_f64", n, dd, lm, *mp, Rh, at("t", o), at("y", o), at("s", o), z, at("ll2", i))
                                elif what == "grad":
                                    call("pgps_gp_ll_grad_adj_het_dev_f64", n, dd, lm, *mp, Rh, at("t", o), z, at("y", o), at("s", o),
                                         at("out2", i, nout))
                                else:
                                    call("pgps_gp_predict_het_dev_f64", n, L(int(qoffs[i + 1] - q)), dd, lm, *mp, Rh, at("t", o), at("y", o),
                                         at("s", o), z, at("tq", q), at("mean2", q), at("var2", q), at("ll2", i))
                            ctx.synchronize()

                    panel(), loop()
                    a = np.empty(S * nout if what == "grad" else S)
                    ctx.d2h(a, dev["out" if what == "grad" else "ll"])
                    a = a.reshape(S, -1)[:, 0]
                    if het:
                        b = np.empty(S * nout if what == "grad" else S)
                        ctx.d2h(b, dev["out2" if what == "grad" else "ll2"])
                        b = b.reshape(S, -1)[:, 0]
                    else:
                        b = ll_loop
                    err = float(np.max(np.abs(a - b) / np.abs(b)))
                    ms, inner = _timed({"panel": panel, "loop": loop}, reps, min_window)
                    row = {"size": size, "S": S, "rows": int(offs[-1]), "queries": K if what == "predict" else 0, "kernel": kname,
                           "d": d, "rs": het, "call": what, "passes_per_window": inner, "relerr_ll_against_loop": err,
                           "panel_ms": ms["panel"], "loop_ms": ms["loop"], "speedup": ms["loop"][1] / ms["panel"][1]}
                    rows.append(row)
                    print(f"{size} {kname} rs={int(het)} {what:8s}: panel {row['panel_ms'][1]:10.4f} ms   loop of {S} calls "
                          f"{row['loop_ms'][1]:10.4f} ms   loop / panel {row['speedup']:7.2f}   agree {err:.1e}", flush=True)
                finally:
                    for ptr in dev.values():
                        ctx.free(ptr)
    for group in resident.values():
        for ser in group:
            ser.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=list(SIZES), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-window", type=float, default=0.05, help="seconds of calls per timed window, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_bench.json"))
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
