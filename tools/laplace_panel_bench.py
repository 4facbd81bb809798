"""The mode searches of a panel of S series in one launch (pgps_gp_panel_laplace_dev_f64 and its gradient / predict companions,
on a device-resident PanelData) against what one has to do without them: the loop of S searches driven from the host, each on
a _backend.SiteBuffers whose series is on the device already (LaplaceStateSpaceGP._search's loop: four launches and a copy of
six doubles per Newton step, no thresholds fixed in advance).  Three timings per point: the fit; fit + gradient; fit + predict
at K_i = n_i / 4.  Both sides' total Newton passes are recorded, so that a ratio is not an artefact of different iteration
counts.  Every timed pass ends in one stream synchronise.

Every shape is warmed up first, the two sides alternate --reps times, medians (with min and max) over windows of at least
--min-window seconds are reported.  Writes profiles/laplace_panel_bench.json and prints a table.

One size per process, every GPU step under its own time limit, chained so that trouble ends the run:

    timeout -k 10 200 python tools/laplace_panel_bench.py --size s64 && timeout -k 10 900 python tools/laplace_panel_bench.py --size s1024

s64, s1024, s8192: S series with lengths uniform in [100, 1000]; full2048: 256 series of 2048 points (its predict has 1536 points
and 512 queries per series).  Matern-3/2 (d = 2) and Matern-5/2 (d = 3); Bernoulli and Poisson.  --kernels / --liks / --what
narrow a run (the loop side of s8192 takes tens of seconds per pass)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-gps_amd"))

SIZES = {"s64": 64, "s1024": 1024, "s8192": 8192, "full2048": 256}
TOL, MAX_ITER = 1e-8, 50


def _kernel(kname):
    from pssgp.kernels import Matern32, Matern52
    return {"m32": Matern32, "m52": Matern52}[kname](1.0, 1.0)


def _problem(size, lik, predict):
    """[(t, y, tq)]: irregular times, draws of the likelihood under a smooth latent function, 5 % missing."""
    rng = np.random.RandomState(len(size) + SIZES[size])
    out = []
    for _ in range(SIZES[size]):
        n = (1536 if predict else 2048) if size == "full2048" else int(rng.randint(100, 1001))
        k = 512 if size == "full2048" else n // 4
        t = np.cumsum(0.05 * (0.5 + rng.rand(n)))
        latent = np.sin(0.7 * t) + 0.5 * np.sin(0.13 * t + 1.0)
        if lik == "bernoulli":
            y = (rng.rand(n) < 1.0 / (1.0 + np.exp(-2.0 * latent))).astype(np.float64)
        else:
            y = rng.poisson(2.0 * np.exp(latent)).astype(np.float64)
        y[rng.rand(n) < 0.05] = np.nan
        out.append((t, y, np.sort(rng.uniform(t[0], t[-1], k))))
    return out


def _timed(sides, reps, min_window):
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


def run(size, reps, min_window, knames, liks, whats):
    from pssgp import _backend as Bk
    from pssgp._backend.fused import _fused_model
    from pssgp.laplace import LaplaceStateSpaceGP
    from pssgp.likelihoods import Bernoulli, Poisson
    S = SIZES[size]
    rows = []
    for lik in liks:
        lik_obj = Bernoulli() if lik == "bernoulli" else Poisson(1.5)
        for predict in sorted({w == "fit+predict" for w in whats}):
            cases = _problem(size, lik, predict)
            offs = np.concatenate([[0], np.cumsum([c[0].size for c in cases])]).astype(np.int64)
            qoffs = np.concatenate([[0], np.cumsum([c[2].size for c in cases])]).astype(np.int64)
            tq = np.concatenate([c[2] for c in cases])
            data = Bk.PanelData(offs, np.concatenate([c[0] for c in cases]), np.concatenate([c[1] for c in cases]))
            bufs = [Bk.SiteBuffers(t, y, lik_obj.lik_id, lik_obj.par) for t, y, _ in cases]
            ctx = data.ctx
            try:
                for kname in knames:
                    kern = _kernel(kname)
                    driver = LaplaceStateSpaceGP((cases[0][0][:, None], cases[0][1][:, None]), kern, lik_obj, tol=TOL, max_iter=MAX_ITER)
                    sde, form = driver._fused()
                    P0, H = np.asarray(sde.P0, np.float64), np.asarray(sde.H, np.float64).reshape(-1)
                    d, model = _fused_model(form, P0, H)
                    table = [(form, P0, H, 0.0)]
                    passes = {"panel": 0, "loop": 0}
                    ev = {"panel": np.zeros(S), "loop": np.zeros(S)}
                    for what in [w for w in whats if (w == "fit+predict") == predict]:
                        def panel():
                            info = Bk.panel.gp_panel_laplace_dev(data, table, lik_obj.lik_id, [lik_obj.par], TOL, MAX_ITER)
                            if what == "fit+grad":
                                Bk.panel.gp_panel_laplace_grad_dev(data, table, lik_obj.lik_id, [lik_obj.par])
                            elif what == "fit+predict":
                                Bk.panel.gp_panel_laplace_predict_dev(data, table, qoffs, tq)
                            ctx.synchronize()
                            passes["panel"] = int(np.sum(info[:, 3] + 1))
                            ev["panel"] = info[:, 0] + info[:, 1]

                        def loop():
                            total = 0
                            for i, (buf, (t, y, q)) in enumerate(zip(bufs, cases)):
                                with ctx.lock:
                                    ll, corr, info = driver._search(lambda: buf.start(), lambda: buf.newton(model, d), buf.halve, buf.accept)
                                total += info["iterations"] + 1
                                ev["loop"][i] = ll + corr
                                if what == "fit+grad":
                                    f, v, z, s = buf.fetch("f"), buf.fetch("v", proposal=True), buf.fetch("zs"), buf.fetch("ss")
                                    obs = ~np.isnan(y)
                                    _, _, W, d3 = lik_obj.log_prob_derivs(np.where(obs, y, 0.0), f)
                                    w = np.where(obs, 0.5 * v * d3 / W, np.nan)
                                    for x in (z + w, w, np.where(obs, 0.0, np.nan)):
                                        Bk.gp_ll_grad_adj_het(form, P0, H, 0.0, t, x, s)
                                elif what == "fit+predict":
                                    Bk.gp_predict_het(form, P0, H, 0.0, t, buf.fetch("zs"), buf.fetch("ss"), q)
                            ctx.synchronize()
                            passes["loop"] = total

                        panel(), loop()
                        err = float(np.max(np.abs(ev["panel"] - ev["loop"]) / np.maximum(1.0, np.abs(ev["loop"]))))
                        ms, inner = _timed({"panel": panel, "loop": loop}, reps, min_window)
                        row = {"size": size, "S": S, "rows": int(offs[-1]), "queries": int(qoffs[-1]) if predict else 0, "kernel": kname,
                               "d": d, "likelihood": lik, "call": what, "passes_per_window": inner, "newton_passes": dict(passes),
                               "relerr_evidence_against_loop": err, "panel_ms": ms["panel"], "loop_ms": ms["loop"],
                               "speedup": ms["loop"][1] / ms["panel"][1]}
                        rows.append(row)
                        print(f"{size} {kname} {lik:9s} {what:11s}: panel {row['panel_ms'][1]:10.3f} ms   loop of {S} searches "
                              f"{row['loop_ms'][1]:10.3f} ms   loop / panel {row['speedup']:7.2f}   passes {passes['panel']} / {passes['loop']}   "
                              f"agree {err:.1e}", flush=True)
            finally:
                data.close()
                for b in bufs:
                    b.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=list(SIZES), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-window", type=float, default=0.05, help="seconds of calls per timed window, at least")
    ap.add_argument("--kernels", default="m32,m52")
    ap.add_argument("--liks", default="bernoulli,poisson")
    ap.add_argument("--what", default="fit,fit+grad,fit+predict")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laplace_panel_bench.json"))
    args = ap.parse_args()
    rows = run(args.size, args.reps, args.min_window, args.kernels.split(","), args.liks.split(","), args.what.split(","))
    old = []
    if os.path.exists(args.out):
        with open(args.out) as f:
            keys = {(r["size"], r["kernel"], r["likelihood"], r["call"]) for r in rows}
            old = [r for r in json.load(f) if (r["size"], r["kernel"], r["likelihood"], r["call"]) not in keys]
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(old + rows, f, indent=1)


if __name__ == "__main__":
    main()
