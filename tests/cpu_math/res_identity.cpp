// Host harness for tests/test_res_identity.py: filt_combine / smth_combine of parallel-gps_amd/csrc/pgps_math.h with the
// identity element on either side.  The resident launch's workgroup scans (pgps_resident.hip.h) let every lane combine at
// the row levels -- with the identity where the DPP shift has no source -- so this must return the other operand bit for bit.
#include "pgps_math.h"

using namespace pgps;

namespace {
template <typename E>
void put(const double* v, E& e) { static_assert(sizeof(E) % sizeof(double) == 0, "packed doubles"); __builtin_memcpy(&e, v, sizeof(E)); }
template <typename E>
void get(const E& e, double* v) { __builtin_memcpy(v, &e, sizeof(E)); }
}  // namespace

// x: n elements of the type's packed layout; out: 2 n -- combine(I, x_i), then combine(x_i, I)
extern "C" int res_identity_filt_f64_d2(const double* x, long n, double* out) {
    using E = FiltElem<double, 2>;
    constexpr long W = sizeof(E) / sizeof(double);
    for (long i = 0; i < n; ++i) {
        E a, id, r;
        put(x + i * W, a);
        filt_identity(id);
        filt_combine(id, a, r);
        get(r, out + (2 * i) * W);
        filt_combine(a, id, r);
        get(r, out + (2 * i + 1) * W);
    }
    return (int)W;
}
extern "C" int res_identity_smth_f64_d2(const double* x, long n, double* out) {
    using E = SmthElem<double, 2>;
    constexpr long W = sizeof(E) / sizeof(double);
    for (long i = 0; i < n; ++i) {
        E a, id, r;
        put(x + i * W, a);
        smth_identity(id);
        smth_combine(id, a, r);
        get(r, out + (2 * i) * W);
        smth_combine(a, id, r);
        get(r, out + (2 * i + 1) * W);
    }
    return (int)W;
}
