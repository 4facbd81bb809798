// Host harness for tests/test_gpu_resident_aggregate.py: the lane's smoothing aggregate of the resident launch
// (pgps_resident.hip.h, res_agg_fold) folded left to right with smth_combine of parallel-gps_amd/csrc/pgps_math.h, once
// started at the identity element and once started AT the first element.  The kernel does the second; it must be the first
// bit for bit.
#include "pgps_math.h"

using namespace pgps;

// x: n chains of lc elements in SmthElem<double, 2>'s packed layout; out: 2 n elements -- the chain from the identity, then
// the chain from its first element
extern "C" int res_aggregate_chain_f64_d2(const double* x, long n, int lc, double* out) {
    using E = SmthElem<double, 2>;
    static_assert(sizeof(E) % sizeof(double) == 0, "packed doubles");
    constexpr long W = sizeof(E) / sizeof(double);
    for (long i = 0; i < n; ++i) {
        E a, b, e, r;
        smth_identity(a);
        for (int j = 0; j < lc; ++j) {
            __builtin_memcpy(&e, x + (i * lc + j) * W, sizeof(E));
            smth_combine(a, e, r);
            a = r;
            if (j == 0) {
                b = e;
            } else {
                smth_combine(b, e, r);
                b = r;
            }
        }
        __builtin_memcpy(out + (2 * i) * W, &a, sizeof(E));
        __builtin_memcpy(out + (2 * i + 1) * W, &b, sizeof(E));
    }
    return (int)W;
}
