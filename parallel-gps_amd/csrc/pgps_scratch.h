// pgps_scratch.h -- how a launch function lays out the device scratch it needs: a bump carver (parts named and typed
// once, the total derived from them), the ONE function that turns a carver into memory, and the rule by which B items
// run in groups that fit a scratch budget.  The arithmetic compiles on the host without any HIP header
// (tests/cpu_math/scratch.cpp); commit() and the budgets of the context exist under hipcc only.
#pragma once

#include <cstddef>

namespace pgps {

// a part of a carved buffer: its offset from the base, typed.  It becomes a pointer only through a Scratch (below)
template <typename T>
struct Part {
    size_t off = 0;
};

inline size_t align_up(size_t x, size_t align) { return (x + align - 1) & ~(align - 1); }      // align: a power of two

// Bump carver: part<T>(count) reserves count elements at the next aligned offset.  Every offset is a multiple of `align`
// (a power of two), a part of 0 elements occupies nothing (it shares its successor's offset), and bytes() -- the aligned
// end of the last part -- is what the buffer must hold.
class Carver {
public:
    explicit Carver(size_t align) : align_(align) {}
    template <typename T>
    Part<T> part(size_t count) {
        const Part<T> p{off_};
        off_ = align_up(off_ + count * sizeof(T), align_);
        return p;
    }
    size_t bytes() const { return off_; }

private:
    size_t align_, off_ = 0;
};

// the base of a committed carver: s(part) is the part's address
struct Scratch {
    char* base = nullptr;
    template <typename T>
    T* operator()(Part<T> p) const { return reinterpret_cast<T*>(base + p.off); }
};

// B items over one series run in groups that fit a scratch budget: max(1, min(items, 65535, (budget - fixed) / per_item)),
// 0 for the quotient where the fixed part alone exceeds the budget.  One item is the least a launch can hold, and a group
// is one launch's grid.y
constexpr size_t kGridYMax = 65535;
inline size_t batch_group(size_t budget, size_t fixed_bytes, size_t per_item_bytes, size_t items) {
    size_t group = budget > fixed_bytes ? (budget - fixed_bytes) / per_item_bytes : 0;
    if (group > items) group = items;
    if (group > kGridYMax) group = kGridYMax;
    return group < 1 ? 1 : group;
}

// Steps per lane of a launch that gives a series of m steps ONE workgroup of kPanelLanes lanes (the panel kernels, their Gram,
// site and fit launches): the series' own, max(1, ceil(m / lanes)); the pinned chunk (pgps_set_chunk) where it covers the
// series (ctx->chunk * kBlock >= m).  THE rule: every planner and pgps_get_panel_chunk call it
constexpr int kPanelLanes = 256;        // == kBlock (pgps_panel_inst.hip asserts it)
inline int panel_steps_per_lane(long m, int chunk) {
    if (chunk > 0 && (long)chunk * kPanelLanes >= m) return chunk;
    const long own = (m + kPanelLanes - 1) / kPanelLanes;
    return own < 1 ? 1 : (int)own;
}

// The budgets when pgps_set_batch_scratch has not set one.
// Fused path (d <= 3): the smallest budget beyond which the measured time per model no longer improves (B = 1000,
// N + K = 5000, d = 2: 3.79, 2.83, 2.35, 2.19 ms at 8, 16, 32, 64 MiB, 2.2 .. 2.7 ms at 256 MiB and 1 GiB)
constexpr size_t kBatchScratchDefault = (size_t)64 << 20;
// General-LTI path (a model is ~3 (N + K) d^2 doubles, 12.6 MB at d = 11, N + K = 4216): d = 11, B = 64 measured 34.7, 23.4,
// 16.6, 13.6, 12.6 ms at 8, 32, 64, 256 MiB and 1 GiB -- still improving at the largest budget measured, where the whole
// batch is one group
constexpr size_t kBatchScratchDefaultLti = (size_t)1 << 30;

}  // namespace pgps

#if defined(__HIPCC__)
#include "pgps_internal.h"

namespace pgps {

// ensure() of the carver's total, then the base its parts resolve against: no pointer exists before the buffer has its
// final address, and none reaches past what was ensured
inline int commit(pgps_ctx* ctx, DevBuf& b, const Carver& c, Scratch* s) {
    const int rc = ensure(ctx, b, c.bytes());
    s->base = rc ? nullptr : (char*)b.p;
    return rc;
}

inline size_t batch_budget_fused(const pgps_ctx* ctx) { return ctx->batch_scratch ? ctx->batch_scratch : kBatchScratchDefault; }
inline size_t batch_budget_lti(const pgps_ctx* ctx) { return ctx->batch_scratch ? ctx->batch_scratch : kBatchScratchDefaultLti; }

}  // namespace pgps
#endif
