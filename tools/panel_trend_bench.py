"""Mean functions of a panel: the Gram call of S series against the loop of S single-series Gram calls, and the price of the
columns.  The panels and the protocol are tools/panel_bench.py's (lengths uniform in [100, 1000], full2048: 256 series of 2048
points; warm-up, alternating sides, medians with min and max over windows of at least --min-window seconds, every timed pass
ends in a stream synchronise).  V = [y, 1, u, u^2] cut to C = 2 and 4 columns, u the series' times centred and scaled.

Per point (size, kernel, rs, C):
  gram      pgps_gp_panel_gram_dev_f64 on the resident ts, V (and rs)
  profile   the device sequence of StateSpaceGPPanel.profile_log_likelihood_and_grad: the Gram call, the records back, S small
            solves on the host, betas up, pgps_gp_panel_residual_dev_f64, pgps_gp_panel_ll_grad_dev_f64, the rows back
  ll        pgps_gp_panel_ll_dev_f64 on the same panel's y: what one column costs, the price of the columns is gram / ll
  loop      scalar noise: S pgps_gp_gram_multi_dev_f64 calls on slices of the same resident arrays, queued back to back and
            synchronised once per pass -- the fastest thing a user could do without the panel call.  With rs there is NO device
            baseline (the single model has no such route): the panel's time stands alone, and at s64 the host twins
            (panel_trend.whiten_host per series) are timed ONCE as a baseline of a different kind ("host_twin_ms").

Writes profiles/panel_trend_bench.json and prints a table.  One size per process, every GPU step under its own time limit:

    timeout -k 10 120 python tools/panel_trend_bench.py --size s64 && timeout -k 10 200 python tools/panel_trend_bench.py --size s1024
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from panel_bench import R, SIZES, _model, _problem, _timed  # noqa: E402

COLUMNS = (2, 4)


def _columns(t, y, C):
    u = (t - 0.5 * (t[0] + t[-1])) / max(0.5 * (t[-1] - t[0]), 1e-9)
    V = np.stack([y, np.ones(t.size), u, u * u][:C], axis=1)
    V[np.isnan(y)] = np.nan
    return np.ascontiguousarray(V)


def run(size, reps, min_window):
    from pssgp import _backend as Bk
    from pssgp.kernels import Matern32, Matern52
    from pssgp.panel_trend import whiten_host
    from pssgp.trend import _chol_design, _chol_solve
    ctx = Bk.get_context()
    lib, h = ctx.lib, ctx.handle
    L, I, F, P = ctypes.c_long, ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(P)                          # noqa: E731
    cases = _problem(size, False)
    S = SIZES[size]
    offs = np.concatenate([[0], np.cumsum([c[0].size for c in cases])]).astype(np.int64)
    ts, ss = np.concatenate([c[0] for c in cases]), np.concatenate([c[2] for c in cases])
    rows = []
    for kname in ("m32", "m52"):
        form, Pinf, H = _model(kname)
        lam, N1, N2 = form
        d = Pinf.shape[0]
        table, _ = Bk._gp_rows([(form, Pinf, H, R)])
        mp = [p(np.ascontiguousarray(a, np.float64)) for a in (N1, N2, Pinf, H)]
        keep = (N1, N2, Pinf, H)                                # noqa: F841 -- (the arrays behind mp stay alive)
        for het in (False, True):
            for C in COLUMNS:
                V = np.concatenate([_columns(c[0], c[1], C) for c in cases])
                data = Bk.PanelData(offs, ts, V[:, 0], ss if het else None, V=V)
                rec = C * C + 2
                dloop = ctx.malloc(8 * S * rec)
                try:
                    view = data.residual_view()

                    def gram():
                        return Bk.panel.gp_panel_gram_dev(data, table)

                    def profile():
                        G, logdet, n_obs = Bk.panel.gp_panel_gram_dev(data, table)
                        betas = np.empty((S, C - 1))
                        for s in range(S):
                            Lc, sc = _chol_design(G[s, 1:, 1:])
                            betas[s] = _chol_solve(Lc, sc, G[s, 1:, 0])
                        Bk.panel.gp_panel_residual_dev(data, betas, view)
                        return Bk.panel.gp_panel_ll_grad_dev(view, table)

                    def ll():
                        return Bk.panel.gp_panel_ll_dev(data, table)

                    def loop():
                        z, lm, Rh = F(0.0), F(lam), F(R)
                        with ctx.lock:
                            for i in range(S):
                                o, n = int(offs[i]), int(offs[i + 1] - offs[i])
                                out = dloop + 8 * rec * i
                                Bk.check(ctx, lib.pgps_gp_gram_multi_dev_f64(h, L(n), I(C), I(d), lm, *mp, Rh, P(data.ts + 8 * o),
                                                                             P(data.V + 8 * C * o), z, P(out), P(out + 8 * C * C),
                                                                             P(out + 8 * (C * C + 1))), "pgps_gp_gram_multi_dev_f64")
                        ctx.synchronize()

                    sides = {"gram": gram, "profile": profile, "ll": ll}
                    err = None
                    if not het:
                        sides["loop"] = loop
                        loop()
                        back = np.empty(S * rec)
                        ctx.d2h(back, dloop)
                        G = gram()[0]
                        Gl = back.reshape(S, rec)[:, :C * C].reshape(S, C, C)
                        dg = np.sqrt(np.einsum("sii->si", Gl))
                        err = float(np.max(np.abs(G - Gl) / (dg[:, :, None] * dg[:, None, :])))
                    ms, inner = _timed(sides, reps, min_window)
                    row = {"size": size, "S": S, "rows": int(offs[-1]), "kernel": kname, "d": d, "rs": het, "C": C,
                           "passes_per_window": inner, "gram_ms": ms["gram"], "profile_ms": ms["profile"], "ll_ms": ms["ll"],
                           "gram_over_ll": ms["gram"][1] / ms["ll"][1]}
                    if not het:
                        row.update({"loop_ms": ms["loop"], "loop_over_gram": ms["loop"][1] / ms["gram"][1], "gram_err_against_loop": err})
                    elif size == "s64":
                        kern = {"m32": Matern32, "m52": Matern52}[kname](1.0, 1.0)
                        tic = time.perf_counter()
                        for i, c in enumerate(cases):
                            whiten_host(kern, R, c[0], V[offs[i]:offs[i + 1]], c[2])
                        row["host_twin_ms"] = 1e3 * (time.perf_counter() - tic)     # (once; a baseline of a different kind)
                    rows.append(row)
                    tail = (f"loop of {S} calls {row['loop_ms'][1]:10.4f} ms   loop / gram {row['loop_over_gram']:7.2f}   agree {err:.1e}"
                            if not het else f"host twins {row.get('host_twin_ms', float('nan')):10.2f} ms (once)")
                    print(f"{size} {kname} rs={int(het)} C={C}: gram {row['gram_ms'][1]:9.4f} ms   profile {row['profile_ms'][1]:9.4f} ms   "
                          f"ll {row['ll_ms'][1]:9.4f} ms   gram / ll {row['gram_over_ll']:5.2f}   {tail}", flush=True)
                finally:
                    ctx.free(dloop)
                    data.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=list(SIZES), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-window", type=float, default=0.05, help="seconds of calls per timed window, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_trend_bench.json"))
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
