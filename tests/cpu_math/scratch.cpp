// Host harness of parallel-gps_amd/csrc/pgps_scratch.h (no GPU, no HIP header): the bump carver over seeded random
// sequences of parts, and batch_group against the literal formula on a table of edges.  A stand-alone program: exit
// status 0 and a last line "scratch ok" when every check held (tests/test_scratch_host.py builds and runs it, once more
// under -fsanitize=address,undefined).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "pgps_scratch.h"

using namespace pgps;

struct alignas(16) Sixteen { double a, b; };
static_assert(sizeof(Sixteen) == 16, "the 16-byte element");

static long failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Seen { size_t off, count, esize; };

static int carver_sequences(int nseq) {
    std::mt19937_64 rng(20261019);
    long parts_total = 0, zero_parts = 0;
    for (int q = 0; q < nseq; ++q) {
        const size_t align = (rng() & 1) ? 128 : 256;
        const int nparts = 1 + (int)(rng() % 12);
        Carver c(align);
        std::vector<Seen> seen;
        size_t hand = 0;                                    // the hand-written form the launch functions used
        for (int i = 0; i < nparts; ++i) {
            const int kind = (int)(rng() % 3);
            size_t count = 0;                               // a quarter of the parts are empty; sizes straddle the alignment
            switch (rng() % 4) {
                case 0: count = 0; break;
                case 1: count = 1 + rng() % 70; break;
                case 2: count = (align / 4) * (1 + rng() % 8) + (rng() % 3) - 1; break;
                default: count = 1 + rng() % 100000; break;
            }
            const size_t esize = kind == 0 ? 4 : kind == 1 ? 8 : 16;
            const size_t off = kind == 0 ? c.part<float>(count).off : kind == 1 ? c.part<double>(count).off : c.part<Sixteen>(count).off;
            CHECK(off == hand, "sequence %d part %d: offset %zu, by hand %zu", q, i, off, hand);
            hand = (hand + count * esize + align - 1) / align * align;
            CHECK(c.bytes() == hand, "sequence %d part %d: bytes() %zu, by hand %zu", q, i, c.bytes(), hand);
            seen.push_back({off, count, esize});
            ++parts_total;
            zero_parts += count == 0;
        }
        for (size_t i = 0; i < seen.size(); ++i) {
            const Seen& a = seen[i];
            CHECK(a.off % align == 0, "sequence %d part %zu: offset %zu not a multiple of %zu", q, i, a.off, align);
            if (i + 1 < seen.size()) {
                if (a.count == 0) CHECK(a.off == seen[i + 1].off, "sequence %d: empty part %zu at %zu, successor at %zu", q, i, a.off, seen[i + 1].off);
                else CHECK(a.off + a.count * a.esize <= seen[i + 1].off, "sequence %d: part %zu runs into part %zu", q, i, i + 1);
            }
            for (size_t j = i + 1; j < seen.size(); ++j) {
                const Seen& b = seen[j];
                const bool overlap = a.count && b.count && a.off < b.off + b.count * b.esize && b.off < a.off + a.count * a.esize;
                CHECK(!overlap, "sequence %d: parts %zu and %zu overlap", q, i, j);
            }
        }
        const Seen& last = seen.back();
        CHECK(last.off + last.count * last.esize <= c.bytes(), "sequence %d: the last part ends at %zu, bytes() = %zu", q,
              last.off + last.count * last.esize, c.bytes());
        CHECK(c.bytes() % align == 0, "sequence %d: bytes() %zu not a multiple of %zu", q, c.bytes(), align);
    }
    std::printf("carver: %d sequences, %ld parts (%ld empty)\n", nseq, parts_total, zero_parts);
    // a handle resolves against the base it is given, and only there
    alignas(256) static char buf[1024];
    Carver c(256);
    const Part<float> a = c.part<float>(3);
    const Part<double> b = c.part<double>(5);
    Scratch s;
    s.base = buf;
    CHECK((char*)s(a) == buf && (char*)s(b) == buf + 256 && c.bytes() == 512, "resolution against the base");
    return 0;
}

// the formula as the issue states it
static size_t group_literal(size_t budget, size_t fixed, size_t per_item, size_t items) {
    const size_t fit = budget > fixed ? (budget - fixed) / per_item : 0;
    return std::max<size_t>(1, std::min({items, (size_t)65535, fit}));
}

static void group_table() {
    const size_t big = (size_t)1 << 40;
    const size_t fixeds[] = {0, 1, 256, 4096 + 768, (size_t)3 << 30};
    const size_t pers[] = {1, 8, 2304, 1000003, big - 1, big, big + 12345};
    const size_t itemss[] = {1, 2, 5, 1000, 65535, 65536, 100000, (size_t)1 << 31};
    long rows = 0;
    auto row = [&](size_t budget, size_t fixed, size_t per, size_t items, size_t want_or_0) {
        const size_t got = batch_group(budget, fixed, per, items), want = group_literal(budget, fixed, per, items);
        CHECK(got == want, "batch_group(%zu, %zu, %zu, %zu) = %zu, the formula gives %zu", budget, fixed, per, items, got, want);
        if (want_or_0) CHECK(got == want_or_0, "batch_group(%zu, %zu, %zu, %zu) = %zu, expected %zu", budget, fixed, per, items, got, want_or_0);
        CHECK(got >= 1 && got <= 65535 && (got <= items || items == 0), "batch_group(%zu, %zu, %zu, %zu) = %zu out of range", budget, fixed, per, items, got);
        ++rows;
    };
    for (size_t fixed : fixeds)
        for (size_t per : pers)
            for (size_t items : itemss) {
                row(1, fixed, per, items, 1);                                               // budget 1: one item whatever else
                row(fixed, fixed, per, items, 1);                                           // budget = fixed
                if (fixed) row(fixed - 1, fixed, per, items, 1);                            // budget < fixed
                row(fixed + per - 1, fixed, per, items, 1);                                 // one byte short of one item
                row(fixed + per, fixed, per, items, 1);                                     // exactly one item
                for (size_t k : {(size_t)2, (size_t)3, (size_t)7, (size_t)65535, (size_t)65536, (size_t)70000}) {
                    if (per > ((size_t)-1 - fixed) / k) continue;                           // (the test's own product must fit size_t)
                    row(fixed + k * per, fixed, per, items, std::min({k, items, (size_t)65535}));
                    row(fixed + k * per - 1, fixed, per, items, std::min({k - 1, items, (size_t)65535}));
                    row(fixed + k * per + per - 1, fixed, per, items, std::min({k, items, (size_t)65535}));
                }
                row((size_t)-1, fixed, per, items, 0);                                      // the largest budget there is
            }
    // items beyond grid.y with a budget that would hold them all
    row((size_t)1 << 40, 0, 8, 100000, 65535);
    row((size_t)1 << 40, 4096, 8, 65536, 65535);
    // per_item near 2^40: seven items fit 2^43 - 1 bytes, eight fit 2^43
    row(((size_t)1 << 43) - 1, 0, big, 100, 7);
    row((size_t)1 << 43, 0, big, 100, 8);
    row(((size_t)1 << 43) + 4096, 4096, big, 100, 8);
    row(((size_t)1 << 43) + 4095, 4096, big, 100, 7);
    // the two defaults
    CHECK(kBatchScratchDefault == (size_t)64 * 1024 * 1024 && kBatchScratchDefaultLti == (size_t)1024 * 1024 * 1024, "default budgets");
    std::printf("batch_group: %ld rows\n", rows);
}

int main() {
    carver_sequences(10000);
    group_table();
    if (failures) { std::printf("scratch: %ld checks FAILED\n", failures); return 1; }
    std::printf("scratch ok\n");
    return 0;
}
