// fit_ctl.cpp -- the control rule of the per-series fit on the host (tests/test_fit_ctl_host.py builds and runs this; no GPU):
// parallel-gps_amd/csrc/pgps_fit.h (fit_search, the loop k_gpp_fit runs per workgroup) and pgps_fit_model.h (the Matern closed
// forms and the contraction of the adjoints) compiled as plain C++.
//
//   fit_ctl                    drives fit_search over the toy problems below, checks status, result and the evaluation cap of
//                              every search, prints "fit ok"
//   fit_ctl trace NAME         prints every point fit_search evaluates on problem NAME ("eval x0 x1 x2 f g0 g1 g2") and the
//                              result ("result x0 x1 x2 f f0 gnorm iterations evaluations status"): the pytest runs
//                              pssgp.fitting.bfgs_box on the same function and holds both sequences together
//   fit_ctl forms U[30]        U = N1 (9) N2 (9) Pinf (9) H (3) of the Matern-5/2 unit form: prints, for d = 1, 2, 3 over a grid of
//                              (s2, ell), the model of fit_matern_model and f, g of fit_contract on printed adjoints
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pgps_fit.h"
#include "pgps_fit_model.h"

using namespace pgps;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            return 1;                                                            \
        }                                                                        \
    } while (0)

// ---- toy problems: polynomials only, written product by product (the pytest restates them in the same order) -------------------
struct Problem {
    const char* name;
    double x0[3], lo[3], hi[3];
    int free_[3];
    double gtol;
    int max_iter;
};

static void f_quad(const double* x, double* f, double* g) {
    static const double A[3][3] = {{3.0, 1.0, 0.0}, {1.0, 2.0, 0.5}, {0.0, 0.5, 1.0}};
    static const double b[3] = {1.0, -2.0, 0.5};
    double Ax[3];
    for (int i = 0; i < 3; ++i) Ax[i] = (A[i][0] * x[0] + A[i][1] * x[1]) + A[i][2] * x[2];
    *f = 0.5 * ((x[0] * Ax[0] + x[1] * Ax[1]) + x[2] * Ax[2]) - ((b[0] * x[0] + b[1] * x[1]) + b[2] * x[2]);
    for (int i = 0; i < 3; ++i) g[i] = Ax[i] - b[i];
}
static void f_valley(const double* x, double* f, double* g) {
    const double a = 1.0 - x[0], c = x[1] - x[0] * x[0], e = x[2] - 0.5;
    *f = (a * a + 10.0 * (c * c)) + e * e;
    g[0] = -2.0 * a - 40.0 * (c * x[0]);
    g[1] = 20.0 * c;
    g[2] = 2.0 * e;
}
static void f_outside(const double* x, double* f, double* g) {
    const double d0 = x[0] - 5.0, d1 = x[1] + 5.0, d2 = x[2] - 0.3;
    *f = (d0 * d0 + d1 * d1) + d2 * d2;
    g[0] = 2.0 * d0; g[1] = 2.0 * d1; g[2] = 2.0 * d2;
}
static void f_radius(const double* x, double* f, double* g) {
    const double r2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    const double d0 = x[0] - 0.5, d1 = x[1] - 0.2, d2 = x[2] + 0.1;
    *f = (d0 * d0 + 4.0 * (d1 * d1)) + 0.25 * (d2 * d2);
    g[0] = 2.0 * d0; g[1] = 8.0 * d1; g[2] = 0.5 * d2;
    if (r2 > 4.0) { *f = NAN; g[0] = g[1] = g[2] = NAN; }
}
static void f_nan(const double*, double* f, double* g) { *f = NAN; g[0] = g[1] = g[2] = NAN; }
static void f_liar(const double* x, double* f, double* g) {
    *f = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    g[0] = -2.0 * x[0]; g[1] = -2.0 * x[1]; g[2] = -2.0 * x[2];
}
static void f_inf_grad(const double* x, double* f, double* g) { *f = x[0]; g[0] = INFINITY; g[1] = 0.0; g[2] = 0.0; }
// finite at the first evaluation, NaN ever after
static int g_calls = 0;
static void f_once(const double* x, double* f, double* g) {
    f_quad(x, f, g);
    if (g_calls++ > 0) { *f = NAN; g[0] = g[1] = g[2] = NAN; }
}
// coordinate 1 is not free: its gradient reads 0
static void f_fixed(const double* x, double* f, double* g) {
    f_valley(x, f, g);
    g[1] = 0.0;
}

typedef void (*Fn)(const double*, double*, double*);
struct Entry { Problem p; Fn fn; };
static const Entry kProblems[] = {
    {{"quad", {0.0, 0.0, 0.0}, {-10.0, -10.0, -10.0}, {10.0, 10.0, 10.0}, {1, 1, 1}, 1e-10, 100}, f_quad},
    {{"valley", {-1.2, 1.0, 2.0}, {-3.0, -3.0, -3.0}, {3.0, 3.0, 3.0}, {1, 1, 1}, 1e-9, 200}, f_valley},
    {{"outside", {0.0, 0.0, 0.0}, {-1.0, -1.0, -1.0}, {1.0, 1.0, 1.0}, {1, 1, 1}, 1e-10, 100}, f_outside},
    {{"radius", {1.5, 1.0, 0.5}, {-3.0, -3.0, -3.0}, {3.0, 3.0, 3.0}, {1, 1, 1}, 1e-10, 100}, f_radius},
    {{"nan", {0.5, 0.5, 0.5}, {-1.0, -1.0, -1.0}, {1.0, 1.0, 1.0}, {1, 1, 1}, 1e-10, 100}, f_nan},
    {{"liar", {1.0, 1.0, 1.0}, {-10.0, -10.0, -10.0}, {10.0, 10.0, 10.0}, {1, 1, 1}, 1e-10, 100}, f_liar},
    {{"inf_grad", {0.5, 0.5, 0.5}, {-1.0, -1.0, -1.0}, {1.0, 1.0, 1.0}, {1, 1, 1}, 1e-10, 100}, f_inf_grad},
    {{"once", {0.3, 0.3, 0.3}, {-10.0, -10.0, -10.0}, {10.0, 10.0, 10.0}, {1, 1, 1}, 1e-10, 200}, f_once},
    {{"fixed", {-1.2, 0.7, 2.0}, {-3.0, 0.7, -3.0}, {3.0, 0.7, 3.0}, {1, 0, 1}, 1e-7, 100}, f_fixed},
    {{"one_step", {-1.2, 1.0, 2.0}, {-3.0, -3.0, -3.0}, {3.0, 3.0, 3.0}, {1, 1, 1}, 1e-9, 1}, f_valley},
    {{"start_clipped", {7.0, -7.0, 0.0}, {-1.0, -1.0, -1.0}, {1.0, 1.0, 1.0}, {1, 1, 1}, 1e-10, 100}, f_outside},
};

struct ToyOps {
    Fn fn;
    bool trace;
    int calls = 0;
    void eval(const double x[kFitP], double* f, double g[kFitP]) {
        fn(x, f, g);
        calls += 1;
        if (trace) std::printf("eval %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", x[0], x[1], x[2], *f, g[0], g[1], g[2]);
    }
};

static FitResult run(const Entry& e, bool trace, int* calls) {
    g_calls = 0;
    ToyOps o{e.fn, trace};
    FitResult r;
    fit_search(o, e.p.x0, e.p.lo, e.p.hi, e.p.free_, e.p.gtol, e.p.max_iter, r);
    *calls = o.calls;
    return r;
}

static const Entry* find(const char* name) {
    for (const Entry& e : kProblems)
        if (!std::strcmp(e.p.name, name)) return &e;
    return nullptr;
}

static int self_check() {
    CHECK(fit_max_iter_valid(1) && fit_max_iter_valid(kFitMaxIterCap) && !fit_max_iter_valid(0) && !fit_max_iter_valid(kFitMaxIterCap + 1));
    CHECK(fit_gtol_valid(0.0) && fit_gtol_valid(1e-6) && !fit_gtol_valid(-1.0) && !fit_gtol_valid(NAN) && !fit_gtol_valid(INFINITY));
    CHECK(fit_eval_cap(1) == 43 && fit_eval_cap(200) == 8401);
    for (const Entry& e : kProblems) {
        int calls;
        const FitResult r = run(e, false, &calls);
        std::printf("%-14s status %d iterations %3d evaluations %4d gnorm %.3e x %.12g %.12g %.12g\n", e.p.name, r.status,
                    r.iterations, r.evaluations, r.gnorm, r.x[0], r.x[1], r.x[2]);
        CHECK(calls == r.evaluations);
        CHECK(r.evaluations <= fit_eval_cap(e.p.max_iter));             // every search ends within the cap
        CHECK(r.iterations <= e.p.max_iter);
        CHECK(r.status >= 0 && r.status <= 3);
        for (int i = 0; i < 3; ++i) CHECK(r.x[i] >= e.p.lo[i] && r.x[i] <= e.p.hi[i]);
        if (r.status != kFitNotFinite) CHECK(r.f <= r.f0);
    }
    int calls;
    FitResult r = run(*find("quad"), false, &calls);
    CHECK(r.status == kFitConverged);
    CHECK(std::fabs(r.x[0] - 16.0 / 17.0) < 1e-9 && std::fabs(r.x[1] + 31.0 / 17.0) < 1e-9 && std::fabs(r.x[2] - 24.0 / 17.0) < 1e-9);
    r = run(*find("valley"), false, &calls);
    CHECK(r.status == kFitConverged);
    CHECK(std::fabs(r.x[0] - 1.0) < 1e-7 && std::fabs(r.x[1] - 1.0) < 1e-7 && std::fabs(r.x[2] - 0.5) < 1e-7);
    r = run(*find("outside"), false, &calls);                             // the minimum lies outside the box: on the bound, converged
    CHECK(r.status == kFitConverged && r.x[0] == 1.0 && r.x[1] == -1.0 && std::fabs(r.x[2] - 0.3) < 1e-9 && r.gnorm <= 1e-10);
    r = run(*find("start_clipped"), false, &calls);
    CHECK(r.status == kFitConverged && r.x[0] == 1.0 && r.x[1] == -1.0 && std::fabs(r.x[2] - 0.3) < 1e-9);
    r = run(*find("radius"), false, &calls);
    CHECK(r.status == kFitConverged);
    CHECK(std::fabs(r.x[0] - 0.5) < 1e-8 && std::fabs(r.x[1] - 0.2) < 1e-8 && std::fabs(r.x[2] + 0.1) < 1e-7);
    r = run(*find("nan"), false, &calls);
    CHECK(r.status == kFitNotFinite && r.evaluations == 1 && r.iterations == 0 && std::isnan(r.gnorm));
    r = run(*find("inf_grad"), false, &calls);
    CHECK(r.status == kFitNotFinite && r.evaluations == 1);
    r = run(*find("liar"), false, &calls);                                // every trial goes uphill: the line search fails at once
    CHECK(r.status == kFitLineSearch && r.iterations == 0 && r.evaluations == 1 + (kFitMaxHalvings + 1));
    CHECK(r.x[0] == 1.0 && r.x[1] == 1.0 && r.x[2] == 1.0);
    r = run(*find("once"), false, &calls);
    CHECK(r.status == kFitLineSearch && r.iterations == 0 && r.x[0] == 0.3);
    r = run(*find("fixed"), false, &calls);
    CHECK(r.status == kFitConverged && r.x[1] == 0.7);                    // bit for bit
    r = run(*find("one_step"), false, &calls);
    CHECK(r.status == kFitMaxIter && r.iterations == 1);

    // fit_theta: the start and the bounds come back bit for bit
    const double t0 = 0.3, lo = 0.3e-4, hi = 0.3e4;
    const double x0 = std::log(t0), xlo = std::log(lo), xhi = std::log(hi);
    CHECK(fit_theta(x0, x0, xlo, xhi, t0, lo, hi) == t0);
    CHECK(fit_theta(xlo, x0, xlo, xhi, t0, lo, hi) == lo);
    CHECK(fit_theta(xhi, x0, xlo, xhi, t0, lo, hi) == hi);
    CHECK(fit_theta(0.25, x0, xlo, xhi, t0, lo, hi) == std::exp(0.25));
    std::printf("fit ok\n");
    return 0;
}

template <int D>
static void forms_rows(const FitModel& unit) {
    constexpr int NST = D * D + 2 * D + 1;
    unsigned long long seed = 88172645463325252ull + D;
    auto next = [&]() {                 // xorshift: adjoints in (-1, 1)
        seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17;
        return (double)(seed >> 11) / 9007199254740992.0 * 2.0 - 1.0;
    };
    const double s2s[] = {0.37, 1.0, 12.5, 3e-3}, ells[] = {0.11, 1.0, 7.3, 250.0};
    for (double s2 : s2s)
        for (double ell : ells) {
            FitModel m;
            fit_matern_model<D>(s2, ell, unit, m);
            double stats[NST];
            for (double& v : stats) v = next();
            const double th[3] = {s2, ell, 0.05 + 0.5 * (next() + 1.0)};
            const int free_[3] = {1, 1, D == 2 ? 0 : 1};
            const double n_obs = D == 1 ? 0.0 : 37.0, ll = -12.25 + next();
            double f, g[3];
            fit_contract<D>(m, th, free_, n_obs, ll, stats, &f, g);
            std::printf("forms %d %.17g %.17g %.17g %.17g %.17g", D, s2, ell, th[2], n_obs, ll);
            std::printf(" %.17g", m.lam);
            for (int i = 0; i < D * D; ++i) std::printf(" %.17g", m.N1[i]);
            for (int i = 0; i < D * D; ++i) std::printf(" %.17g", m.N2[i]);
            for (int i = 0; i < D * D; ++i) std::printf(" %.17g", m.Pinf[i]);
            for (int i = 0; i < D; ++i) std::printf(" %.17g", m.H[i]);
            for (int i = 0; i < NST; ++i) std::printf(" %.17g", stats[i]);
            std::printf(" %.17g %.17g %.17g %.17g\n", f, g[0], g[1], g[2]);
        }
}

int main(int argc, char** argv) {
    if (argc == 1) return self_check();
    if (argc == 3 && !std::strcmp(argv[1], "trace")) {
        const Entry* e = find(argv[2]);
        if (!e) return 2;
        int calls;
        const FitResult r = run(*e, true, &calls);
        std::printf("result %.17g %.17g %.17g %.17g %.17g %.17g %d %d %d\n", r.x[0], r.x[1], r.x[2], r.f, r.f0, r.gnorm, r.iterations,
                    r.evaluations, r.status);
        return 0;
    }
    if (argc == 32 && !std::strcmp(argv[1], "forms")) {
        FitModel unit{};
        unit.lam = 1.0;
        for (int i = 0; i < 9; ++i) {
            unit.N1[i] = std::atof(argv[2 + i]);
            unit.N2[i] = std::atof(argv[11 + i]);
            unit.Pinf[i] = std::atof(argv[20 + i]);
        }
        for (int i = 0; i < 3; ++i) unit.H[i] = std::atof(argv[29 + i]);
        forms_rows<1>(unit);
        forms_rows<2>(unit);
        forms_rows<3>(unit);
        return 0;
    }
    std::printf("usage: fit_ctl | fit_ctl trace NAME | fit_ctl forms U[30]\n");
    return 2;
}
