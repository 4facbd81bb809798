// pgps_fit.h -- the control rule of a per-series hyper-parameter fit, in ONE place for the host and the
// device alike (the header also compiles as plain C++: tests/cpu_math/fit_ctl.cpp drives it over toy problems), as
// pgps_newton.h holds the rule of the Laplace mode search.  pssgp/fitting.py (bfgs_box) is its twin in numpy and follows it.
//
// The problem: minimise f(x) over the box lo <= x <= hi, x = log theta, P = kFitP = 3 coordinates in the order of
// trainable_parameters() (variance, lengthscales, noise_variance), f = -ll / max(1, n_obs), g = df / dx.  A coordinate that
// is not free has g = 0 and never moves (its theta is kept beside the search and never taken through log / exp).
//
// The rule: BFGS on the INVERSE matrix H (P x P) with a backtracking Armijo search and projection onto the box; `fresh`
// means "H is the identity".
//   0  x = clip(x0), evaluate; f or g not finite: status kFitNotFinite, stop
//   1  q = the projected gradient: g with component i zeroed where (x_i <= lo_i and g_i > 0) or (x_i >= hi_i and g_i < 0);
//      max |q| <= gtol: status kFitConverged;  iterations == max_iter: status kFitMaxIter
//   2  p = -q (fresh) or -H q;  alpha = min(1, 1 / max |q|) (fresh) or 1
//   3  at most kFitMaxHalvings + 1 trials: x_t = clip(x + alpha p), s = x_t - x; a trial with g . s >= 0 is rejected WITHOUT an
//      evaluation; otherwise evaluate, accept when f_t and g_t are finite and f_t <= f + kFitArmijo g . s; on rejection alpha /= 2
//   4  nothing accepted: not fresh -> H = I, fresh, back to 2 within the same iteration; fresh -> status kFitLineSearch, stop
//   5  accepted: y = g_t - g, with y_i = 0 at a free coordinate that stayed ON a bound (x_t,i on a bound and s_i = 0): the
//      matrix is built on the coordinates that move.  The SET of free coordinates on a bound changed in this step, or
//      s . y <= kFitCurvature |s| |y|: fresh.  Otherwise, if fresh, H = (s . y / y . y) I first; then the BFGS update of the
//      inverse, fresh cleared.  x, f, g = x_t, f_t, g_t; iterations += 1; back to 1
//      (A reset at EVERY step that ends on a bound would leave a fit whose optimum lies on a bound -- a lengthscale capped
//      below its optimum -- with steepest descent for the other coordinates: 60 iterations do not reach gtol = 1e-6 there.
//      While a coordinate rests on its bound its row and column of H stay those of the last reset, a multiple of the identity's.)
// fit_search runs the loop over ONE operation of a route, eval(x, &f, g).  It ends after at most
// 1 + 2 (kFitMaxHalvings + 1) max_iter evaluations whatever the numbers are (NaN, infinite): every loop below counts.
// Every sum is formed in index order (0, 1, 2), every product rounded as written: the twin repeats the operations one by one.
#pragma once

#include <cmath>

#ifndef PGPS_HD
#if defined(__HIPCC__)
#define PGPS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PGPS_HD inline
#endif
#endif

namespace pgps {

constexpr int kFitP = 3;                    // variance, lengthscales, noise_variance
constexpr int kFitMaxHalvings = 20;
constexpr int kFitMaxIterCap = 200;         // what an entry point accepts as max_iter: 1 .. kFitMaxIterCap
constexpr double kFitArmijo = 1e-4;
constexpr double kFitCurvature = 1e-10;
constexpr int kFitInfo = 8;                 // doubles of an info row of pgps_gp_panel_fit_*

enum FitStatus { kFitConverged = 0, kFitMaxIter = 1, kFitLineSearch = 2, kFitNotFinite = 3 };

PGPS_HD bool fit_max_iter_valid(int max_iter) { return max_iter >= 1 && max_iter <= kFitMaxIterCap; }
PGPS_HD bool fit_gtol_valid(double gtol) { return std::isfinite(gtol) && gtol >= 0.0; }
// the evaluations a search can make at most
PGPS_HD int fit_eval_cap(int max_iter) { return 1 + 2 * (kFitMaxHalvings + 1) * max_iter; }

PGPS_HD double fit_clip(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }
PGPS_HD bool fit_finite(double f, const double g[kFitP]) {
    return std::isfinite(f) && std::isfinite(g[0]) && std::isfinite(g[1]) && std::isfinite(g[2]);
}
PGPS_HD double fit_dot(const double a[kFitP], const double b[kFitP]) {
    double acc = a[0] * b[0];
    acc += a[1] * b[1];
    acc += a[2] * b[2];
    return acc;
}
// q and max |q|
PGPS_HD double fit_project(const double x[kFitP], const double g[kFitP], const double lo[kFitP], const double hi[kFitP],
                           double q[kFitP]) {
    double qmax = 0.0;
    for (int i = 0; i < kFitP; ++i) {
        const bool pinned = (x[i] <= lo[i] && g[i] > 0.0) || (x[i] >= hi[i] && g[i] < 0.0);
        q[i] = pinned ? 0.0 : g[i];
        const double a = std::fabs(q[i]);
        if (a > qmax) qmax = a;
    }
    return qmax;
}
PGPS_HD bool fit_accept(double f_t, const double g_t[kFitP], double f, double gs) {
    return fit_finite(f_t, g_t) && f_t <= f + kFitArmijo * gs;
}
PGPS_HD bool fit_curvature_ok(double sy, double ss, double yy) { return sy > kFitCurvature * (std::sqrt(ss) * std::sqrt(yy)); }

// what a search leaves: info row of pgps_gp_panel_fit_* is [-f n | -f0 n | iterations | evaluations | status | gnorm | n_obs | 0]
struct FitResult {
    double x[kFitP];        // the last accepted iterate
    double f, f0;           // f there, f at the (clipped) start
    double gnorm;           // max |q| there (NaN at status kFitNotFinite)
    int iterations, evaluations, status;
};

// Ops:  void eval(const double x[kFitP], double* f, double g[kFitP])
// free_[i] != 0: coordinate i is free.  On the device every lane of the workgroup runs this loop on the SAME numbers, so every
// branch is uniform.
template <typename Ops>
PGPS_HD void fit_search(Ops& o, const double x0[kFitP], const double lo[kFitP], const double hi[kFitP], const int free_[kFitP],
                        double gtol, int max_iter, FitResult& r) {
    double x[kFitP], g[kFitP], H[kFitP][kFitP];
    double f;
    for (int i = 0; i < kFitP; ++i) x[i] = fit_clip(x0[i], lo[i], hi[i]);
    o.eval(x, &f, g);
    r.evaluations = 1;
    r.iterations = 0;
    r.f0 = f;
    r.gnorm = NAN;
    bool fresh = true;
    for (int i = 0; i < kFitP; ++i)
        for (int j = 0; j < kFitP; ++j) H[i][j] = i == j ? 1.0 : 0.0;
    int status = fit_finite(f, g) ? -1 : (int)kFitNotFinite;
    // (one pass of this loop is one iteration; it runs at most max_iter + 1 times)
    for (int it = 0; it <= max_iter && status < 0; ++it) {
        double q[kFitP];
        const double qmax = fit_project(x, g, lo, hi, q);
        r.gnorm = qmax;
        if (qmax <= gtol) { status = kFitConverged; }
        else if (it == max_iter) { status = kFitMaxIter; }
        else {
            bool accepted = false;
            double xt[kFitP], gt[kFitP], s[kFitP], ft = 0.0;
            // (two rounds at most: the second from H = I after a failed search along -H q)
            for (int round = 0; round < 2 && !accepted && status < 0; ++round) {
                double p[kFitP], alpha;
                if (fresh) {
                    for (int i = 0; i < kFitP; ++i) p[i] = -q[i];
                    alpha = 1.0 / qmax;
                    if (alpha > 1.0) alpha = 1.0;
                } else {
                    for (int i = 0; i < kFitP; ++i) {
                        double acc = H[i][0] * q[0];
                        acc += H[i][1] * q[1];
                        acc += H[i][2] * q[2];
                        p[i] = -acc;
                    }
                    alpha = 1.0;
                }
                for (int trial = 0; trial <= kFitMaxHalvings && !accepted; ++trial) {
                    for (int i = 0; i < kFitP; ++i) {
                        xt[i] = fit_clip(x[i] + alpha * p[i], lo[i], hi[i]);
                        s[i] = xt[i] - x[i];
                    }
                    const double gs = fit_dot(g, s);
                    if (gs < 0.0) {
                        o.eval(xt, &ft, gt);
                        r.evaluations += 1;
                        accepted = fit_accept(ft, gt, f, gs);
                    }
                    alpha *= 0.5;
                }
                if (!accepted) {
                    if (fresh) status = kFitLineSearch;
                    else {
                        fresh = true;
                        for (int i = 0; i < kFitP; ++i)
                            for (int j = 0; j < kFitP; ++j) H[i][j] = i == j ? 1.0 : 0.0;
                    }
                }
            }
            if (accepted) {
                double y[kFitP];
                bool changed = false;               // the set of free coordinates on a bound
                for (int i = 0; i < kFitP; ++i) {
                    const bool was = free_[i] && (x[i] <= lo[i] || x[i] >= hi[i]);
                    const bool is = free_[i] && (xt[i] <= lo[i] || xt[i] >= hi[i]);
                    if (was != is) changed = true;
                    y[i] = (is && s[i] == 0.0) ? 0.0 : gt[i] - g[i];
                }
                const double sy = fit_dot(s, y), ss = fit_dot(s, s), yy = fit_dot(y, y);
                if (changed || !fit_curvature_ok(sy, ss, yy)) {
                    fresh = true;
                    for (int i = 0; i < kFitP; ++i)
                        for (int j = 0; j < kFitP; ++j) H[i][j] = i == j ? 1.0 : 0.0;
                } else {
                    if (fresh) {
                        const double scale = sy / yy;
                        for (int i = 0; i < kFitP; ++i)
                            for (int j = 0; j < kFitP; ++j) H[i][j] = i == j ? scale : 0.0;
                    }
                    // H += ((s.y + y.Hy) / (s.y)^2) s s^T - (Hy s^T + s Hy^T) / s.y
                    double Hy[kFitP];
                    for (int i = 0; i < kFitP; ++i) {
                        double acc = H[i][0] * y[0];
                        acc += H[i][1] * y[1];
                        acc += H[i][2] * y[2];
                        Hy[i] = acc;
                    }
                    const double yHy = fit_dot(y, Hy);
                    const double c1 = (sy + yHy) / (sy * sy), c2 = 1.0 / sy;
                    for (int i = 0; i < kFitP; ++i)
                        for (int j = 0; j < kFitP; ++j)
                            H[i][j] = (H[i][j] + c1 * (s[i] * s[j])) - c2 * (Hy[i] * s[j] + s[i] * Hy[j]);
                    fresh = false;
                }
                for (int i = 0; i < kFitP; ++i) { x[i] = xt[i]; g[i] = gt[i]; }
                f = ft;
                r.iterations = it + 1;
            }
        }
    }
    for (int i = 0; i < kFitP; ++i) r.x[i] = x[i];
    r.f = f;
    r.status = status;
}

}  // namespace pgps
