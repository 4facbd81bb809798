// pgps_newton.h -- the control rule of the damped Newton search of a Laplace approximation (DESIGN.md sections 4y, 4ab), in ONE
// place for the host and the device alike (the header also compiles as plain C++: tests/cpu_math/newton_ctl.cpp drives it over a
// scalar toy problem).  The rule is that of LaplaceStateSpaceGP._search:
//   accept      Psi_new finite and >= Psi - kNewtonPsiSlack |Psi|
//   halve       otherwise, at most kNewtonMaxHalvings times per step (the last proposal is then taken as it is)
//   converged   the PASS's move max |f - f_prev| is finite and <= tol (the undamped move: it is measured before any halving)
//   closing     after convergence ONE more pass from the accepted mode: its Gaussian log-likelihood of the sites and its
//               variances are the mode's
//   stop        unconverged after max_iter steps, keeping the last iterate (pass max_iter + 1 supplies its log-likelihood)
// newton_search runs the loop over four operations of a route; it ends after at most max_iter + 1 passes and
// kNewtonMaxHalvings max_iter damped updates whatever the sums are (NaN, infinite): every loop below counts.
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

constexpr int kNewtonMaxHalvings = 20;
constexpr double kNewtonPsiSlack = 1e-12;
constexpr int kNewtonMaxIterCap = 1000;         // what an entry point accepts as max_iter: 1 .. kNewtonMaxIterCap

PGPS_HD bool newton_max_iter_valid(int max_iter) { return max_iter >= 1 && max_iter <= kNewtonMaxIterCap; }
PGPS_HD bool newton_tol_valid(double tol) { return std::isfinite(tol) && tol >= 0.0; }

PGPS_HD bool newton_accept(double psi_new, double psi) {
    return std::isfinite(psi_new) && psi_new >= psi - kNewtonPsiSlack * std::fabs(psi);
}
PGPS_HD bool newton_halve_again(double psi_new, double psi, int halvings) {
    return !newton_accept(psi_new, psi) && halvings < kNewtonMaxHalvings;
}
PGPS_HD bool newton_converged(double move, double tol) { return std::isfinite(move) && move <= tol; }

// what a search leaves: info row of pgps_gp_panel_laplace_* in this order
struct NewtonResult {
    double ll_sites;        // Gaussian log-likelihood of the sites, from the last pass
    double corr;            // sum [lp - log N(z | f, s)] at the accepted iterate
    double psi;             // Psi at the accepted iterate
    double move;            // the last step's move (NaN before the first)
    double n_obs;           // observed rows
    int iterations, halvings, converged, passes;
};

// Ops:  void start(double s[3])   (lp, f alpha, corr) of the start, which becomes the iterate
//       void pass(double s[6])    one smoothing pass from the iterate into the proposal: [ll | lp | f alpha | corr | move | n_obs]
//       void halve(double s[3])   the proposal moved half way back to the iterate
//       void accept()             the proposal becomes the iterate
// On the device every lane of the workgroup runs this loop on the SAME sums, so every branch is uniform.
template <typename Ops>
PGPS_HD void newton_search(Ops& o, double tol, int max_iter, NewtonResult& r) {
    double s3[3], s6[6];
    o.start(s3);
    r.psi = s3[0] - 0.5 * s3[1];
    r.corr = s3[2];
    r.ll_sites = 0.0;
    r.move = NAN;
    r.n_obs = 0.0;
    r.iterations = 0; r.halvings = 0; r.converged = 0; r.passes = 0;
    for (int it = 0; it <= max_iter; ++it) {
        o.pass(s6);
        r.passes += 1;
        r.ll_sites = s6[0];
        r.n_obs = s6[5];
        if (r.converged || it == max_iter) break;       // the closing pass, or the pass after the last allowed step
        r.move = s6[4];
        double c_new = s6[3];
        double psi_new = s6[1] - 0.5 * s6[2];
        int halvings = 0;
        while (newton_halve_again(psi_new, r.psi, halvings)) {
            o.halve(s3);
            psi_new = s3[0] - 0.5 * s3[1];
            c_new = s3[2];
            halvings += 1;
        }
        o.accept();
        r.psi = psi_new;
        r.corr = c_new;
        r.iterations = it + 1;
        r.halvings += halvings;
        r.converged = newton_converged(r.move, tol) ? 1 : 0;
    }
}

}  // namespace pgps
