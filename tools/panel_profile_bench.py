"""The panel's profile gradient in one call against the sequence it replaces.  The panels and the protocol are
tools/panel_trend_bench.py's (lengths uniform in [100, 1000]; V = [y, 1, u, u^2] cut to C = 2 and 4 columns; Matern-3/2 and
-5/2, scalar noise and rs; warm-up, alternating sides, medians with min and max over --reps windows of at least --min-window
seconds; every timed pass ends in a stream synchronise or a blocking copy back).

Per point (size, kernel, rs, C):
  fused       pgps_gp_panel_profile_grad_dev_f64 through _backend.panel.gp_panel_profile_grad_dev: Gram, the S solves, the
              residuals and the adjoint pass queued back to back, ONE copy back of [betas | sol | rows]
  sequence    the device sequence of StateSpaceGPPanel.profile_log_likelihood_and_grad as it stands: the Gram call, the records
              back, S small solves on the host, betas up, the residual kernel, the adjoint call, the rows back
  device      the three device calls of that sequence alone, with NO host solves (betas of zeros go up): a lower bound of any
              baseline that keeps the three calls
  solve       pgps_gp_panel_trend_solve_dev_f64 alone on resident records, then a stream synchronise
  each_theta  (once per point, not a median) StateSpaceGPPanel.profile_log_likelihoods_and_grads(thetas) with S rows of thetas: its
              model table and its S contractions are Python loops

Before anything is timed the fused call's rows are compared with the sequence's (agree: max relative difference of the summed
row; the solves differ in rounding between the host and the device).

Writes profiles/panel_profile_bench.json and prints a table.  One size per process, every GPU step under its own time limit:

    timeout -k 10 150 python tools/panel_profile_bench.py --size s64 && timeout -k 10 300 python tools/panel_profile_bench.py --size s1024
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-gps_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from panel_bench import R, SIZES, _model, _problem, _timed  # noqa: E402
from panel_trend_bench import COLUMNS, _columns  # noqa: E402


def _each_theta_ms(cases, kname, het, C):
    """One evaluation of the class method at per-series thetas, after one warm-up evaluation."""
    from pssgp.kernels import Matern32, Matern52
    from pssgp.mean_functions import Basis
    from pssgp.panel import StateSpaceGPPanel
    S = len(cases)

    def design(t):
        u = (t - 0.5 * (t[0] + t[-1])) / max(0.5 * (t[-1] - t[0]), 1e-9) if t.size > 1 else np.zeros(t.size)
        return np.stack([np.ones(t.size), u, u * u][:C - 1], axis=1)

    panel = StateSpaceGPPanel([(c[0], c[1]) for c in cases], {"m32": Matern32, "m52": Matern52}[kname](1.0, 1.0), noise_variance=R,
                              observation_variances=[c[2] for c in cases] if het else None, mean_function=Basis(design, C - 1))
    i = np.arange(S, dtype=np.float64) / S
    thetas = np.stack([1.0 + 0.1 * i, 1.0 + 0.05 * i, R * (1.0 + 0.1 * i)], axis=1)
    panel.profile_log_likelihoods_and_grads(thetas)
    tic = time.perf_counter()
    panel.profile_log_likelihoods_and_grads(thetas)
    ms = 1e3 * (time.perf_counter() - tic)
    panel._release()
    return ms


def run(size, reps, min_window):
    from pssgp import _backend as Bk
    from pssgp.trend import _chol_design, _chol_solve
    ctx = Bk.get_context()
    cases = _problem(size, False)
    S = SIZES[size]
    offs = np.concatenate([[0], np.cumsum([c[0].size for c in cases])]).astype(np.int64)
    ts, ss = np.concatenate([c[0] for c in cases]), np.concatenate([c[2] for c in cases])
    rows = []
    for kname in ("m32", "m52"):
        form, Pinf, H = _model(kname)
        d = Pinf.shape[0]
        table, _ = Bk._gp_rows([(form, Pinf, H, R)])
        for het in (False, True):
            for C in COLUMNS:
                V = np.concatenate([_columns(c[0], c[1], C) for c in cases])
                data = Bk.PanelData(offs, ts, V[:, 0], ss if het else None, V=V)
                p = C - 1
                try:
                    view = data.residual_view()
                    zeros = np.zeros((S, p))
                    drec = data._buffer("bench_rec", 8 * S * (C * C + 2))
                    dsol = data._buffer("bench_sol", 8 * S * (p + p * p + 4))

                    def fused():
                        return Bk.panel.gp_panel_profile_grad_dev(data, table)

                    def sequence():
                        G, logdet, n_obs = Bk.panel.gp_panel_gram_dev(data, table)
                        betas = np.empty((S, p))
                        for s in range(S):
                            Lc, sc = _chol_design(G[s, 1:, 1:])
                            betas[s] = _chol_solve(Lc, sc, G[s, 1:, 0])
                        Bk.panel.gp_panel_residual_dev(data, betas, view)
                        return Bk.panel.gp_panel_ll_grad_dev(view, table)

                    def device():
                        Bk.panel.gp_panel_gram_dev(data, table)
                        Bk.panel.gp_panel_residual_dev(data, zeros, view)
                        return Bk.panel.gp_panel_ll_grad_dev(view, table)

                    def solve():
                        ctx.call("pgps_gp_panel_trend_solve_dev_f64", S, C, drec, dsol, dsol + 8 * S * p)
                        ctx.synchronize()

                    # resident records for the solve kernel alone, and the agreement of the two routes
                    ctx.call("pgps_gp_panel_gram_dev_f64", S, offs.ctypes.data, d, 1, table.ctypes.data, C, data.ts, data.V, data.rs, drec)
                    ctx.synchronize()
                    a, b = np.sum(fused()[0], axis=0), np.sum(sequence(), axis=0)
                    err = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
                    ms, inner = _timed({"fused": fused, "sequence": sequence, "device": device, "solve": solve}, reps, min_window)
                finally:
                    data.close()
                row = {"size": size, "S": S, "rows": int(offs[-1]), "kernel": kname, "d": d, "rs": het, "C": C, "passes_per_window": inner,
                       "fused_ms": ms["fused"], "sequence_ms": ms["sequence"], "device_calls_ms": ms["device"], "solve_ms": ms["solve"],
                       "sequence_over_fused": ms["sequence"][1] / ms["fused"][1], "device_calls_over_fused": ms["device"][1] / ms["fused"][1],
                       "agree": err,
                       # (building S single models for the class takes longer than everything else at S = 8192: not timed there)
                       "each_theta_ms_once": _each_theta_ms(cases, kname, het, C) if S <= 1024 else None}
                rows.append(row)
                print(f"{size} {kname} rs={int(het)} C={C}: fused {row['fused_ms'][1]:9.4f} ms   sequence {row['sequence_ms'][1]:9.4f} ms "
                      f"({row['sequence_over_fused']:6.2f} x)   device calls {row['device_calls_ms'][1]:9.4f} ms ({row['device_calls_over_fused']:5.2f} x)"
                      f"   solve {row['solve_ms'][1]:8.4f} ms   agree {err:.1e}   per-series thetas {row['each_theta_ms_once'] or float('nan'):9.2f} ms (once)",
                      flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=["s64", "s1024", "s8192"], required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-window", type=float, default=0.05, help="seconds of calls per timed window, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_profile_bench.json"))
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
