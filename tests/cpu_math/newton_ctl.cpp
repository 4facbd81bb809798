// Host harness of parallel-gps_amd/csrc/pgps_newton.h and pgps_panel_site_lay.h (no GPU, no HIP header): the control rule of
// the mode search that k_gpp_newton runs inside the kernel, driven over scalar toy problems, and the scratch layout of
// pgps_gp_panel_laplace_*.  A stand-alone program: exit status 0 and a last line "newton ok" when every check held
// (tests/test_newton_ctl_host.py builds and runs it, once more under -fsanitize=address,undefined).
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "pgps_lik.h"
#include "pgps_newton.h"
#include "pgps_panel_site_lay.h"

using namespace pgps;

static long failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// ONE observation y under the prior f ~ N(0, k): the search of LaplaceStateSpaceGP in scalars.  A pass is the posterior mean of
// f under the site (z, s): f+ = k z / (k + s), alpha+ = (z - f+) / s.
struct Scalar {
    int lik;
    double par, y, k;
    double f = 0, a = 0, z = 0, s = 1;          // the iterate and its site
    double pf = 0, pa = 0, pz = 0, ps = 1;      // the proposal
    long passes = 0, halves = 0;
    void site(double f_, double& z_, double& s_, double& lp, double& corr) {
        const LikSite ls = lik_site(lik, par, y, f_);
        z_ = ls.z; s_ = ls.s; lp = ls.lp; corr = ls.corr;
    }
    void start(double o[3]) {
        f = 0; a = 0;
        double lp, corr;
        site(f, z, s, lp, corr);
        o[0] = lp; o[1] = f * a; o[2] = corr;
    }
    void pass(double o[6]) {
        ++passes;
        pf = k * z / (k + s);
        pa = (z - pf) / s;
        const double r = z, S = k + s;
        o[0] = -0.5 * (kLog2Pi + std::log(S) + r * r / S);
        double lp, corr;
        site(pf, pz, ps, lp, corr);
        o[1] = lp; o[2] = pf * pa; o[3] = corr; o[4] = std::fabs(pf - f); o[5] = 1.0;
    }
    void halve(double o[3]) {
        ++halves;
        pf = f + 0.5 * (pf - f);
        pa = a + 0.5 * (pa - a);
        double lp, corr;
        site(pf, pz, ps, lp, corr);
        o[0] = lp; o[1] = pf * pa; o[2] = corr;
    }
    void accept() { f = pf; a = pa; z = pz; s = ps; }
};

// sums chosen by the test: what the search does when Psi is NaN, infinite or falls for ever
struct Scripted {
    double psi_value, move;
    long passes = 0, halves = 0, accepts = 0;
    void start(double o[3]) { o[0] = -1.0; o[1] = 0.0; o[2] = 0.0; }
    void pass(double o[6]) { ++passes; o[0] = 0.0; o[1] = psi_value; o[2] = 0.0; o[3] = 0.0; o[4] = move; o[5] = 1.0; }
    void halve(double o[3]) { ++halves; o[0] = psi_value; o[1] = 0.0; o[2] = 0.0; }
    void accept() { ++accepts; }
};

static void rule() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(newton_accept(-1.0, -1.0) && newton_accept(-1.0 - 5e-13, -1.0) && !newton_accept(-1.0 - 2e-12, -1.0), "the slack is 1e-12 |Psi|");
    CHECK(!newton_accept(nan, -1.0) && !newton_accept(-inf, -1.0) && !newton_accept(inf, -1.0), "a non-finite Psi is never accepted");
    CHECK(newton_accept(0.0, 0.0) && !newton_accept(-1e-300, 0.0), "Psi = 0");
    CHECK(newton_converged(1e-8, 1e-8) && !newton_converged(1.0000001e-8, 1e-8) && !newton_converged(nan, 1e-8) && !newton_converged(inf, 1e-8),
          "converged: finite and <= tol");
    CHECK(newton_converged(0.0, 0.0), "tol = 0 accepts a zero move");
    CHECK(newton_halve_again(nan, -1.0, 19) && !newton_halve_again(nan, -1.0, 20), "20 halvings at the most");
    CHECK(!newton_max_iter_valid(0) && newton_max_iter_valid(1) && newton_max_iter_valid(1000) && !newton_max_iter_valid(1001), "the cap of max_iter");
    CHECK(newton_tol_valid(0.0) && newton_tol_valid(1e-8) && !newton_tol_valid(-1e-300) && !newton_tol_valid(nan) && !newton_tol_valid(inf), "tol");
}

static void scalar_problems() {
    // one Poisson count under a wide prior: the undamped Newton step from f = 0 lands at f = k (y - 1) / (k + 1), where exp(f)
    // overflows; the damped search halves and converges
    for (double y : {0.0, 3.0, 1000.0}) {
        Scalar p{PGPS_LIK_POISSON_EXP, 1.0, y, 1e4};
        NewtonResult r;
        newton_search(p, 1e-10, 50, r);
        // the mode solves f = k (y - exp(f))
        CHECK(r.converged == 1, "poisson y = %g: not converged after %d steps", y, r.iterations);
        CHECK(std::fabs(p.f - p.k * (y - std::exp(p.f))) <= 1e-6 * (1.0 + std::fabs(p.f)), "poisson y = %g: f = %.17g is no mode", y, p.f);
        if (y > 100.0) CHECK(r.halvings > 0, "poisson y = %g: the wide prior needs damping", y);
        CHECK(p.passes == r.passes && r.passes == r.iterations + 1 && p.halves == r.halvings, "poisson y = %g: counts", y);
        CHECK(r.passes <= 51 && r.halvings <= 20 * 50, "poisson y = %g: caps", y);
        std::printf("poisson y = %g k = 1e4: f = %.6f after %d steps, %d halvings\n", y, p.f, r.iterations, r.halvings);
    }
    for (double y : {0.0, 1.0}) {
        Scalar p{PGPS_LIK_BERNOULLI_LOGIT, 0.0, y, 25.0};
        NewtonResult r;
        newton_search(p, 1e-10, 50, r);
        const double g = y - 1.0 / (1.0 + std::exp(-p.f));
        CHECK(r.converged == 1 && std::fabs(p.f - p.k * g) <= 1e-8, "bernoulli y = %g: f = %.17g", y, p.f);
    }
    // max_iter = 1: one step, then the pass that supplies the log-likelihood; unconverged, the iterate kept
    Scalar p{PGPS_LIK_POISSON_EXP, 1.0, 5.0, 2.0};
    NewtonResult r;
    newton_search(p, 1e-12, 1, r);
    CHECK(r.converged == 0 && r.iterations == 1 && r.passes == 2, "max_iter = 1: %d steps, %d passes", r.iterations, r.passes);
}

static void termination() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int max_iter : {1, 7, 1000})
        for (double psi : {nan, -inf, inf})
            for (double move : {1.0, nan, inf}) {
                Scripted s{psi, move};
                NewtonResult r;
                newton_search(s, 1e-8, max_iter, r);
                CHECK(r.converged == 0 && r.iterations == max_iter && s.passes == max_iter + 1, "psi %g move %g: %d steps, %ld passes", psi, move,
                      r.iterations, s.passes);
                CHECK(s.halves == 20L * max_iter && r.halvings == 20 * max_iter && s.accepts == max_iter, "psi %g move %g: %ld halvings", psi, move, s.halves);
            }
    // a finite Psi that never falls: converges at the first step with a zero move, one closing pass
    Scripted s{-0.5, 0.0};
    NewtonResult r;
    newton_search(s, 1e-8, 50, r);
    CHECK(r.converged == 1 && r.iterations == 1 && s.passes == 2 && s.halves == 0, "a zero move converges at once");
}

static void layout() {
    std::mt19937_64 rng(20261020);
    long checked = 0;
    for (int q = 0; q < 2000; ++q) {
        const int d = 1 + (int)(rng() % 3);
        const bool grad = rng() & 1;
        const int chunk = (rng() % 4 == 0) ? (int)(1 + rng() % 8) : 0;
        const size_t S = 1 + rng() % 40;
        std::vector<long> len(S);
        for (auto& n : len) n = (rng() % 5 == 0) ? 1 + (long)(rng() % 3) : 1 + (long)(rng() % 2048);
        const size_t budget = (rng() % 3 == 0) ? ((size_t)1 << 18) : (rng() % 2 ? ((size_t)1 << 21) : ((size_t)64 << 20));
        std::vector<SiteGroup> groups(S);
        std::vector<SiteSlices> slices(S);
        std::vector<size_t> first(S);
        std::vector<int> lcs(S);
        size_t ng = 0;
        const size_t need = site_groups(S, d, grad, chunk, budget, [&](size_t s) { return len[s]; },
                                        [&](size_t s, size_t f, const SiteSlices& sl, int Lc) { slices[s] = sl; first[s] = f; lcs[s] = Lc; },
                                        groups.data(), &ng);
        const SiteRecLens rl = site_rec_lens(d);
        size_t covered = 0;
        for (size_t g = 0; g < ng; ++g) {
            const SiteGroup& G = groups[g];
            CHECK(G.first == covered && G.t.series >= 1 && G.t.series <= kGridYMax, "sequence %d: group %zu starts at %zu", q, g, G.first);
            covered += G.t.series;
            const size_t bytes = site_bytes(G.t, d);
            CHECK(bytes <= need, "sequence %d: group %zu needs %zu > %zu", q, g, bytes, need);
            CHECK(bytes <= budget || G.t.series == 1, "sequence %d: group %zu of %zu series exceeds the budget", q, g, G.t.series);
            Carver c(256);
            const SiteParts p = site_lay(c, G.t, d);
            size_t rows_end = 0, fm_end = 0, fP_end = 0, xs_end = 0;
            for (size_t s = G.first; s < G.first + G.t.series; ++s) {
                const SiteSlices& sl = slices[s];
                const size_t n = (size_t)len[s];
                CHECK(first[s] == G.first && sl.slot == s - G.first, "sequence %d: series %zu slot %zu", q, s, sl.slot);
                CHECK(lcs[s] >= 1 && (size_t)lcs[s] * kSiteLanes >= n && lcs[s] == site_steps_per_lane((int)n, chunk), "sequence %d: steps per lane", q);
                if (chunk == 0) CHECK((size_t)(lcs[s] - 1) * kSiteLanes < n, "sequence %d: the series' own steps per lane", q);
                CHECK(sl.o_rows % kSiteAlign == 0 && sl.o_fm % kSiteAlign == 0 && sl.o_fP % kSiteAlign == 0 && sl.o_xs % kSiteAlign == 0,
                      "sequence %d: series %zu: a slice off the alignment", q, s);
                if (grad) {
                    CHECK(sl.o_xs == xs_end, "sequence %d: series %zu: kept states overlap or leave a hole", q, s);
                    xs_end = sl.o_xs + site_pad((size_t)lcs[s] * rl.nx * kSiteLanes);
                } else {
                    CHECK(sl.o_rows == rows_end && sl.o_fm == fm_end && sl.o_fP == fP_end, "sequence %d: series %zu: slices overlap or leave a hole", q, s);
                    rows_end = sl.o_rows + kSiteRowArrays * site_pad(n);
                    fm_end = sl.o_fm + site_pad(n * d);
                    fP_end = sl.o_fP + site_pad(n * d * d);
                    CHECK((kSiteRowArrays - 1) * site_pad(n) + n <= rows_end - sl.o_rows, "sequence %d: the last row array ends inside the slice", q);
                }
                ++checked;
            }
            CHECK(rows_end == G.t.rows && fm_end == G.t.fm && fP_end == G.t.fP && xs_end == G.t.xs, "sequence %d: group %zu totals", q, g);
            // the parts are disjoint, in order, and the last one ends inside bytes()
            const size_t offs[] = {p.rows.off, p.fms.off, p.fPs.off, p.spine.off, p.lpre.off, p.sspine.off, p.lsuf.off, p.ll.off, p.part.off,
                                   p.xs.off, p.gpart.off};
            const size_t counts[] = {G.t.rows, G.t.fm, G.t.fP, G.t.series * rl.nfilt, G.t.series * kSiteLanes * rl.nfilt, G.t.series * rl.nsmth,
                                     G.t.series * kSiteLanes * rl.nsmth, G.t.series, G.t.series * kSitePartials, G.t.xs,
                                     G.t.xs ? G.t.series * rl.nst : 0};
            for (int i = 0; i < 11; ++i) {
                CHECK(offs[i] % 256 == 0, "sequence %d: part %d off the alignment", q, i);
                const size_t end = offs[i] + counts[i] * sizeof(double);
                CHECK(end <= (i + 1 < 11 ? offs[i + 1] : bytes), "sequence %d: part %d runs into its successor", q, i);
            }
        }
        CHECK(covered == S, "sequence %d: %zu of %zu series in groups", q, covered, S);
    }
    CHECK(site_rec_lens(1).nfilt == 5 && site_rec_lens(2).nfilt == 14 && site_rec_lens(3).nfilt == 27, "NFILT");
    CHECK(site_rec_lens(1).nsmth == 3 && site_rec_lens(2).nsmth == 9 && site_rec_lens(3).nsmth == 18, "NSMTH");
    CHECK(site_rec_lens(3).nx == 9 && site_rec_lens(3).nst == 16, "NX, NST");
    CHECK(site_steps_per_lane(2048, 0) == 8 && site_steps_per_lane(257, 0) == 2 && site_steps_per_lane(256, 0) == 1 && site_steps_per_lane(1, 0) == 1, "own steps");
    CHECK(site_steps_per_lane(700, 1) == 3 && site_steps_per_lane(700, 3) == 3 && site_steps_per_lane(700, 4) == 4 && site_steps_per_lane(700, 8) == 8, "pinned steps");
    std::printf("layout: 2000 panels, %ld series\n", checked);
}

int main() {
    rule();
    scalar_problems();
    termination();
    layout();
    if (failures) {
        std::printf("%ld check(s) FAILED\n", failures);
        return 1;
    }
    std::printf("newton ok\n");
    return 0;
}
