// pgps_lik.h -- observation likelihoods of the Laplace approximation: log p(y | f) and its first three
// derivatives in f, fp64, for the host and the device alike (the header also compiles as plain C++).
//
// All three are log-concave in f.  With lp = log p(y | f):  g = d lp / d f,  W = -d^2 lp / d f^2 >= 0 (floored at kLikWMin, so
// that the site variance 1 / W stays finite where the likelihood is flat),  d3 = d^3 lp / d f^3 (NOT floored).  A site formed at
// f is the Gaussian factor N(z | f, s) with  s = 1 / W,  z = f + g / W:  it has the gradient and the curvature of lp at f.
//   PGPS_LIK_GAUSSIAN         y ~ N(f, par)                      par = the noise variance
//   PGPS_LIK_BERNOULLI_LOGIT  y in {0, 1}, p(y = 1) = 1 / (1 + exp(-f))     par unused
//   PGPS_LIK_POISSON_EXP      y ~ Poisson(par exp(f))            par = the exposure; lp leaves out -lgamma(y + 1), which does not
//                                                                depend on f (the caller adds it once)
#pragma once

#include <cmath>

#include "../../include/pgps.h"

#ifndef PGPS_HD
#if defined(__HIPCC__)
#define PGPS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PGPS_HD inline
#endif
#endif

namespace pgps {

constexpr double kLikWMin = 1e-10;          // floor of W (the host twin and the tests' references use the same value)
constexpr double kLog2Pi = 1.8378770664093453;

PGPS_HD bool lik_known(int lik) {
    return lik == PGPS_LIK_GAUSSIAN || lik == PGPS_LIK_BERNOULLI_LOGIT || lik == PGPS_LIK_POISSON_EXP;
}

// (lp, g, W, d3) of one observation y at the latent value f
PGPS_HD void lik_eval(int lik, double par, double y, double f, double& lp, double& g, double& W, double& d3) {
    if (lik == PGPS_LIK_BERNOULLI_LOGIT) {
        // lp = -softplus(-(2 y - 1) f);  with e = exp(-|f|):  p = sigmoid(f),  W = p (1 - p) = e / (1 + e)^2,
        // 1 - 2 p = -sign(f) (1 - e) / (1 + e),  d3 = -W (1 - 2 p)
        const double a = (2.0 * y - 1.0) * f;
        const double e = std::exp(-std::fabs(f));
        const double r = 1.0 / (1.0 + e);
        lp = -((a < 0.0 ? -a : 0.0) + std::log1p(std::exp(-std::fabs(a))));
        const double p = f >= 0.0 ? r : e * r;
        g = y - p;
        W = e * r * r;
        d3 = W * (f >= 0.0 ? 1.0 : -1.0) * (1.0 - e) * r;
    } else if (lik == PGPS_LIK_POISSON_EXP) {
        const double rate = par * std::exp(f);
        lp = y * (f + std::log(par)) - rate;
        g = y - rate;
        W = rate;
        d3 = -rate;
    } else {
        const double r = y - f;
        g = r / par;
        lp = -0.5 * (kLog2Pi + std::log(par) + r * g);
        W = 1.0 / par;
        d3 = 0.0;
    }
    W = W > kLikWMin ? W : kLikWMin;
}

// what one step adds to the sums of a pass: the site (z, s) at f and lp - log N(z | f, s), the factor C_k of the evidence
// (log q = the Gaussian log-likelihood of the sites + the sum of these).  (z - f)^2 / s = g^2 / W.
struct LikSite {
    double lp, z, s, corr;
};
PGPS_HD LikSite lik_site(int lik, double par, double y, double f) {
    double lp, g, W, d3;
    lik_eval(lik, par, y, f, lp, g, W, d3);
    LikSite o;
    o.lp = lp;
    o.s = 1.0 / W;
    o.z = f + g * o.s;
    o.corr = lp + 0.5 * (kLog2Pi - std::log(W) + g * g * o.s);
    return o;
}

}  // namespace pgps
