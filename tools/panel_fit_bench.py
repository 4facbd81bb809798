"""StateSpaceGPPanel.fit_each: all searches inside ONE launch per group against the same rule driven from the host.

The in-kernel side: fit_each(in_kernel=True) -- pgps_gp_panel_fit_dev_f64 on the device-resident series, one workgroup per series,
the whole projected-BFGS search of csrc/pgps_fit.h inside.  The baseline is what a user could do without it: the SAME rule
(pssgp.fitting.bfgs_box, all series in lock step) over StateSpaceGPPanel.log_likelihoods_and_grads(thetas) as that method stands
-- one device call, one table and one contraction per series per lock step.  Beside them: fit_each(in_kernel=False), the twin
with the table and the contraction in array operations, and pgps_gp_panel_ll_grad_dev_f64 alone times the mean number of
evaluations of the in-kernel fit -- the device work of the host-driven routes, a lower bound for them.  The total evaluations of
every side are reported beside the times, so that no ratio comes from different iteration counts.

The panels and the protocol are those of tools/panel_bench.py: lengths uniform in [100, 1000] for s16 (the small end: a few workgroups
iterate alone), s64, s1024, s8192, 256 series of 2048 points for full2048; irregular times, a noisy sine, 5 % missing, s log-uniform over two decades; every shape warmed up,
every side timed over --reps passes in turn, medians (min, max) are reported, every pass ends in a stream synchronise.  A side whose pass
takes seconds is timed once.  Start (1, 1, 1), bounds start times [1e-4, 1e4], gtol 1e-6, max_iter 100.  Writes
profiles/panel_fit_bench.json and prints a table.

One size per process, every GPU step under its own time limit, chained so that trouble ends the run:

    timeout -k 10 120 python tools/panel_fit_bench.py --size s16 && timeout -k 10 200 python tools/panel_fit_bench.py --size s64 && \\
    timeout -k 10 300 python tools/panel_fit_bench.py --size s1024 && \\
    timeout -k 10 500 python tools/panel_fit_bench.py --size s8192 && timeout -k 10 300 python tools/panel_fit_bench.py --size full2048
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-gps_amd"))

SIZES = {"s16": 16, "s64": 64, "s1024": 1024, "s8192": 8192, "full2048": 256}
R = 0.1
START = (1.0, 1.0, 1.0)
GTOL, MAX_ITER = 1e-6, 100


def _problem(size):
    """[(t, y, s)]: the training series of tools/panel_bench.py."""
    rng = np.random.RandomState(len(size) + SIZES[size])
    out = []
    for _ in range(SIZES[size]):
        n = 2048 if size == "full2048" else int(rng.randint(100, 1001))
        t = np.cumsum(0.05 * (0.5 + rng.rand(n)))
        y = np.sin(0.7 * t) + 0.3 * rng.randn(n)
        y[rng.rand(n) < 0.05] = np.nan
        y[0] = 0.1
        out.append((t, y, R * 10.0 ** rng.uniform(-2.0, 0.0, n)))
    return out


def _time(fn, reps, long_pass=1.0):
    """[min, median, max] ms of fn(), which ends in a stream synchronise: `reps` passes, ONE where a pass takes `long_pass` s."""
    tic = time.perf_counter()
    fn()
    first = time.perf_counter() - tic
    if first >= long_pass:
        return [1e3 * first] * 3, 1
    times = []
    for _ in range(reps):
        tic = time.perf_counter()
        fn()
        times.append(time.perf_counter() - tic)
    return [1e3 * min(times), 1e3 * statistics.median(times), 1e3 * max(times)], reps


def run(size, reps):
    from pssgp import _backend as Bk
    from pssgp import fitting
    from pssgp.kernels import Matern32, Matern52
    from pssgp.panel import StateSpaceGPPanel
    ctx = Bk.get_context()
    cases = _problem(size)
    S = len(cases)
    rows = []
    for kname, kernel in (("m32", Matern32), ("m52", Matern52)):
        for het in (False, True):
            panel = StateSpaceGPPanel([(t, y) for t, y, _ in cases], kernel(variance=START[0], lengthscales=START[1]),
                                      noise_variance=START[2], observation_variances=[s for _, _, s in cases] if het else None)
            params = panel.trainable_parameters()
            theta0 = np.tile(np.array(START), (S, 1))
            lo, hi = theta0 * 1e-4, theta0 * 1e4
            free = np.ones(3, bool)
            n_obs = panel._n_obs()
            kept = {}

            def in_kernel():
                kept["kernel"] = panel.fit_each(gtol=GTOL, max_iter=MAX_ITER)
                ctx.synchronize()

            def twin():
                kept["twin"] = panel.fit_each(gtol=GTOL, max_iter=MAX_ITER, in_kernel=False)
                ctx.synchronize()

            def baseline():
                # the rule over the method as it stands: what the parent commit allows
                rows_ = panel._fit_twin(np.arange(S), panel.log_likelihoods_and_grads, theta0, lo, hi, free, n_obs, GTOL, MAX_ITER)
                kept["baseline"] = fitting.PanelFit(*rows_)
                ctx.synchronize()

            table = panel._helper()._matern_table(theta0, params)

            def evaluation():
                Bk.panel.gp_panel_ll_grad_dev(panel._resident(), table)
                ctx.synchronize()

            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                for fn in (in_kernel, evaluation):                      # warm up
                    fn()
                t_kernel, n_kernel = _time(in_kernel, reps)
                t_eval, _ = _time(evaluation, max(reps, 20))
                t_twin, n_twin = _time(twin, reps)
                t_base, n_base = _time(baseline, reps)
            fk, ft, fb = kept["kernel"], kept["twin"], kept["baseline"]
            gap = float(np.max(np.abs(np.log(fk.thetas) - np.log(fb.thetas))))
            ll_gap = float(np.max(np.abs(fk.log_likelihoods - fb.log_likelihoods) / np.maximum(1.0, np.abs(fb.log_likelihoods))))
            mean_evals = float(np.mean(fk.evaluations))
            row = {"size": size, "S": S, "rows": int(sum(c[0].size for c in cases)), "kernel": kname, "noise": "rs" if het else "scalar",
                   "in_kernel_ms": t_kernel, "in_kernel_passes": n_kernel, "twin_ms": t_twin, "twin_passes": n_twin,
                   "baseline_ms": t_base, "baseline_passes": n_base, "evaluation_ms": t_eval,
                   "evaluation_floor_ms": t_eval[1] * mean_evals,
                   "evaluations": {"in_kernel": int(fk.evaluations.sum()), "twin": int(ft.evaluations.sum()), "baseline": int(fb.evaluations.sum())},
                   "lock_steps": {"twin": int(ft.evaluations.max()), "baseline": int(fb.evaluations.max())},
                   "not_converged": {"in_kernel": int(np.count_nonzero(fk.status)), "twin": int(np.count_nonzero(ft.status)),
                                     "baseline": int(np.count_nonzero(fb.status))},
                   "max_abs_log_theta_gap": gap, "max_rel_ll_gap": ll_gap,
                   "baseline_over_in_kernel": t_base[1] / t_kernel[1], "twin_over_in_kernel": t_twin[1] / t_kernel[1]}
            rows.append(row)
            print(f"{size:9s} S {S:5d} {kname} {row['noise']:6s}  in-kernel {t_kernel[1]:9.2f} ms ({row['evaluations']['in_kernel']} evals)"
                  f"  twin {t_twin[1]:10.2f} ms ({row['evaluations']['twin']})  baseline {t_base[1]:10.2f} ms ({row['evaluations']['baseline']})"
                  f"  evaluation x mean evals {row['evaluation_floor_ms']:8.2f} ms  baseline / in-kernel {row['baseline_over_in_kernel']:7.1f} x"
                  f"  not converged {row['not_converged']}  max |dlog theta| {gap:.1e}", flush=True)
            panel._release()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", choices=list(SIZES), required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_fit_bench.json"))
    args = ap.parse_args()
    rows = run(args.size, args.reps)
    have = []
    if os.path.exists(args.out):
        with open(args.out) as f:
            have = [r for r in json.load(f)["rows"] if r["size"] != args.size]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/panel_fit_bench.py", "start": START, "gtol": GTOL, "max_iter": MAX_ITER, "rows": have + rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
