// pgps_fit_model.h -- what an evaluation of the per-series fit (pgps_fit.h, pgps_panel_fit.hip.h) does
// besides the three passes, for the host and the device alike (plain C++ too: tests/cpu_math/fit_ctl.cpp checks both parts
// against pssgp.forms.matern_closed_forms and pssgp.gradients.matern_contract):
//   fit_theta          x = log theta back to theta, exact at the start and on the bounds
//   fit_matern_model   the fused model (lam, N1, N2, Pinf, H) of a single Matern-1/2, -3/2 or -5/2 kernel (d = 1, 2, 3) at
//                      variance s2 and lengthscale ell -- matern_closed_forms restated
//   fit_contract       f = -ll / max(1, n_obs) and its gradient in x from the adjoints [Abar | Ubar | Hbar | Rbar] of the adjoint
//                      pass -- matern_contract restated, then the chain rule d theta / d x = theta
#pragma once

#include <cmath>

#include "pgps_fit.h"

namespace pgps {

// d x d blocks row-major at stride d in the first d d entries, as GpModel holds them
struct FitModel {
    double lam;
    double N1[9], N2[9], Pinf[9];
    double H[3];
};

// theta of a free coordinate at x.  x0 = log(theta0), xlo = log(lo), xhi = log(hi) are the values the search was given: an
// iterate that still equals one of them returns the theta it came from bit for bit (exp(log(t)) may differ from t in the
// last place: a start that never moved stays the start, and a fit that ends on a bound lies inside the box)
PGPS_HD double fit_theta(double x, double x0, double xlo, double xhi, double theta0, double lo, double hi) {
    if (x == x0) return fit_clip(theta0, lo, hi);
    if (x == xlo) return lo;
    if (x == xhi) return hi;
    return std::exp(x);
}

// `unit`: the Matern-5/2 SDE at lam = 1, s2 = 1 (balanced: F = lam F1, Pinf = s2 P1, H = H1); read at D = 3 only
template <int D>
PGPS_HD void fit_matern_model(double s2, double ell, const FitModel& unit, FitModel& m) {
    static_assert(D >= 1 && D <= 3, "Matern-1/2, -3/2, -5/2");
    for (int i = 0; i < 9; ++i) { m.N1[i] = 0.0; m.N2[i] = 0.0; m.Pinf[i] = 0.0; }
    for (int i = 0; i < 3; ++i) m.H[i] = 0.0;
    if (D == 1) {
        m.lam = 1.0 / ell;
        m.Pinf[0] = s2;
        m.H[0] = 1.0;
    } else if (D == 2) {
        const double lam = std::sqrt(3.0) / ell;
        m.lam = lam;
        m.N1[0] = lam;          m.N1[1] = 1.0;
        m.N1[2] = -lam * lam;   m.N1[3] = -lam;
        m.Pinf[0] = s2;         m.Pinf[3] = lam * lam * s2;
        m.H[0] = 1.0;
    } else {
        const double lam = std::sqrt(5.0) / ell;
        m.lam = lam;
        for (int i = 0; i < 9; ++i) {
            m.N1[i] = unit.N1[i] * lam;
            m.N2[i] = unit.N2[i] * (lam * lam);
            m.Pinf[i] = unit.Pinf[i] * s2;
        }
        for (int i = 0; i < 3; ++i) m.H[i] = unit.H[i];
    }
}

// d ll / d theta in the order (variance, lengthscales, noise_variance) from stats = [Abar (d d) | Ubar (d) | Hbar (d) | Rbar]:
//   d ll / d l = -<Abar, N1 - lam I> / l,   d ll / d s2 = Ubar . Pinf H^T / s2,   d ll / d R = Rbar
template <int D>
PGPS_HD void fit_grad_theta(const FitModel& m, double s2, double ell, const double* stats, double dll[kFitP]) {
    double aF = 0.0, uPH = 0.0;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) aF += stats[i * D + j] * (m.N1[i * D + j] - (i == j ? m.lam : 0.0));
    for (int i = 0; i < D; ++i) {
        double ph = 0.0;
        for (int j = 0; j < D; ++j) ph += m.Pinf[i * D + j] * m.H[j];
        uPH += stats[D * D + i] * ph;
    }
    dll[0] = uPH / s2;
    dll[1] = -aF / ell;
    dll[2] = stats[D * D + 2 * D];
}

// f = -ll / max(1, n_obs);  g_i = -theta_i d ll / d theta_i / max(1, n_obs) at a free coordinate, 0 elsewhere
template <int D>
PGPS_HD void fit_contract(const FitModel& m, const double theta[kFitP], const int free_[kFitP], double n_obs, double ll,
                          const double* stats, double* f, double g[kFitP]) {
    double dll[kFitP];
    fit_grad_theta<D>(m, theta[0], theta[1], stats, dll);
    const double scale = n_obs > 1.0 ? n_obs : 1.0;
    *f = -ll / scale;
    for (int i = 0; i < kFitP; ++i) g[i] = free_[i] ? -(theta[i] * dll[i]) / scale : 0.0;
}

}  // namespace pgps
