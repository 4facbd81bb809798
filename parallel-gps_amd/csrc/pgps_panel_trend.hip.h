// pgps_panel_trend.hip.h -- the generalised-least-squares solves of EVERY series of a panel in ONE launch, where the Gram records
// already lie.
//
// A record [G (C, C) | logdet | n_obs] of k_gpp_gram (pgps_panel_gram.hip.h) holds, with C = 1 + p, g_yy = G[0,0], b = G[1:,0] and
// A = G[1:,1:].  k_panel_trend_solve gives ONE LANE to a series -- p <= 7 is a few hundred fp64 operations, and the S systems
// are independent -- and follows the rule of pssgp/trend.py (_chol_design, _chol_solve):
//
//   s_i = 1 / sqrt(A_ii),  Au = diag(s) A diag(s)  (unit diagonal: a pivot measures what a basis function's predecessors leave)
//   L = chol(Au), row by row, every sum in index order
//   beta = s o L^-T L^-1 (s o b)                   by the two triangular solves
//   cov  = s o (L^-T L^-1) o s                     from M = L^-1: entry (i, j), i <= j, is ONE value stored at (i, j) and (j, i)
//   logdet_A = 2 sum log L_ii - 2 sum log s_i
//   profile  = -(n_obs log 2 pi + logdet + g_yy - b . beta) / 2,   flat = profile - logdet_A / 2 + p log 2 pi / 2
//
//   status (a double)   0 solved; 1 an entry of A is not finite or a diagonal entry is <= 0; 2 a pivot's square (the value under
//                       the square root) is <= 0 or not finite; 3 the smallest pivot squared is <= 64 p eps, _chol_design's
//                       threshold.  The FIRST of these that holds, in this order.  At status != 0 the series' betas, cov,
//                       profile, flat and logdet_A are NaN; the arithmetic runs on regardless (no lane leaves early, nothing it
//                       computes is kept), and no other series sees it.
//   C = 1               nothing to solve: status 0, logdet_A = 0, flat = profile = -(n_obs log 2 pi + logdet + g_yy) / 2
//
//   registers   every loop runs to kPanelTrendMax = kPanelGramMax - 1 with guards on p, fully unrolled, so Au / L (in place), M, s
//               and b are registers under constant indices: no scratch.  Rows and columns beyond p are those of the identity
//               (s = 1, b = 0) and are guarded out of every sum and store.
//   bits        no cross-lane arithmetic, no atomics; the body is compiled with contraction off (every product and sum rounded
//               once, as k_panel_residual): a series' outputs depend on its own record and C alone -- not on S, its place in the
//               panel or what its neighbours hold.
//   memory      lane s reads C C + 2 doubles at records + s (C C + 2) and writes p doubles of betas and p p + 4 of sol; lanes
//               s >= S return before any access.
#pragma once

#include <cmath>

#include "pgps_internal.h"

namespace pgps {

constexpr int kPanelTrendMax = kPanelGramMax - 1;       // basis functions p of a series' trend

__global__ __launch_bounds__(kBlock) void k_panel_trend_solve(long S, int C, const double* __restrict__ records,
                                                              double* __restrict__ betas, double* __restrict__ sol) {
    constexpr int P = kPanelTrendMax;
    constexpr double kLog2Pi = 1.8378770664093453, kEps = 2.220446049250313e-16;
    const long sidx = (long)blockIdx.x * kBlock + threadIdx.x;
    if (sidx >= S) return;
    const int p = C - 1;
    const double* rec = records + sidx * ((long)C * C + 2);
    double* bo = betas + sidx * (long)p;                // (not formed into an access at p = 0)
    double* so = sol + sidx * ((long)p * p + 4);
    {
#pragma clang fp contract(off)
        const double g_yy = rec[0], logdet = rec[C * C], n_obs = rec[C * C + 1];
        // ---- A (lower triangle; the upper one is only looked at), b, the scaling
        double L[P][P], M[P][P], b[P], sc[P];
        bool ok1 = true;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            b[i] = 0.0;
#pragma unroll
            for (int j = 0; j < P; ++j) { L[i][j] = i == j ? 1.0 : 0.0; M[i][j] = 0.0; }
        }
#pragma unroll
        for (int i = 0; i < P; ++i) {
            if (i < p) {
                b[i] = rec[(1 + i) * C];
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    if (j < p) {
                        const double a = rec[(1 + i) * C + 1 + j];
                        ok1 = ok1 && isfinite(a);
                        if (j <= i) L[i][j] = a;
                    }
                }
                ok1 = ok1 && L[i][i] > 0.0;
            }
        }
#pragma unroll
        for (int i = 0; i < P; ++i) sc[i] = i < p ? 1.0 / sqrt(L[i][i]) : 1.0;
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j)
                if (i < p) L[i][j] = (L[i][j] * sc[i]) * sc[j];

        // ---- L = chol(Au) in place, column by column; the pivots' squares
        bool ok2 = true;
        double piv_min = 1.0;               // (a pivot's square of a unit-diagonal matrix is at most 1)
#pragma unroll
        for (int j = 0; j < P; ++j) {
            double dj = L[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) dj = dj - L[j][k] * L[j][k];
            if (j < p) {
                ok2 = ok2 && dj > 0.0 && isfinite(dj);
                piv_min = dj < piv_min ? dj : piv_min;
            }
            const double ljj = j < p ? sqrt(dj) : 1.0;
            L[j][j] = ljj;
#pragma unroll
            for (int i = j + 1; i < P; ++i) {
                double v = L[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
                L[i][j] = i < p ? v / ljj : 0.0;
            }
        }
        const bool ok3 = piv_min > 64.0 * (double)p * kEps;
        const double status = !ok1 ? 1.0 : (!ok2 ? 2.0 : (!ok3 ? 3.0 : 0.0));

        // ---- beta = s o L^-T L^-1 (s o b)
        double z[P], x[P];
#pragma unroll
        for (int i = 0; i < P; ++i) {
            double v = b[i] * sc[i];
#pragma unroll
            for (int k = 0; k < i; ++k) v = v - L[i][k] * z[k];
            z[i] = v / L[i][i];
        }
#pragma unroll
        for (int i = P - 1; i >= 0; --i) {
            double v = z[i];
#pragma unroll
            for (int k = P - 1; k > i; --k)
                if (k < p) v = v - L[k][i] * x[k];
            x[i] = v / L[i][i];
        }
        double dot = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            x[i] = x[i] * sc[i];
            if (i < p) dot = dot + b[i] * x[i];
        }

        // ---- M = L^-1 (lower triangular), column by column
#pragma unroll
        for (int j = 0; j < P; ++j) {
            M[j][j] = 1.0 / L[j][j];
#pragma unroll
            for (int i = j + 1; i < P; ++i) {
                double v = 0.0;
#pragma unroll
                for (int k = j; k < i; ++k) v = v - L[i][k] * M[k][j];
                M[i][j] = v / L[i][i];
            }
        }

        // ---- the logarithms, the likelihoods
        double ldL = 0.0, lds = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i)
            if (i < p) { ldL = ldL + std::log(L[i][i]); lds = lds + std::log(sc[i]); }
        const double nan = __builtin_nan("");
        const bool good = status == 0.0;
        const double logdet_A = 2.0 * ldL - 2.0 * lds;
        const double profile = -0.5 * (n_obs * kLog2Pi + logdet + g_yy - dot);
        const double flat = profile - 0.5 * logdet_A + 0.5 * (double)p * kLog2Pi;

        // ---- stores: cov (i, j) and (j, i) from ONE value
#pragma unroll
        for (int i = 0; i < P; ++i) {
            if (i < p) bo[i] = good ? x[i] : nan;
#pragma unroll
            for (int j = i; j < P; ++j) {
                if (j < p) {
                    double v = 0.0;
#pragma unroll
                    for (int k = j; k < P; ++k)
                        if (k < p) v = v + M[k][i] * M[k][j];
                    v = (v * sc[i]) * sc[j];
                    v = good ? v : nan;
                    so[i * p + j] = v;
                    so[j * p + i] = v;
                }
            }
        }
        so[p * p] = good ? profile : nan;
        so[p * p + 1] = good ? flat : nan;
        so[p * p + 2] = good ? logdet_A : nan;
        so[p * p + 3] = status;
    }
}

}  // namespace pgps
