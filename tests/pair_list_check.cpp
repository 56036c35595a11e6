// pair_list_check.cpp — the unit cut of a pair list (csrc/pair_list.hpp)
// without a device: the plan kernels' steps run in a loop over the sorted
// positions (count the units of the chunk heads, exclusive scan, write the
// units), on arrays of exactly the size the library allocates so that a read
// or a write past them is the sanitizers' to report.
//
// A chunk a unit (gdist_sketch_pairs), for every list: every sorted position
// lies in exactly one unit, no unit holds more than kPairUnit pairs or more
// than one row, no unit is empty, a unit never stops short of the cap inside a
// run, and the units and groups are the numbers gdist_ctx_pairs_info reports:
// sum over the rows of ceil(run / kPairUnit), and the distinct rows.
//
// The kmer cut (gdist_pairs, sorted path), for the same lists with synthetic
// set sizes, the budget and the cap of the units array by the header's own
// formulas: every chunk gets 1 .. nseg units, their segment ranges are
// non-empty, ascend and tile [0, nseg) exactly, the units written are the
// scanned total, and that total never exceeds the cap the units kernel relies
// on; with every set empty a chunk is one unit.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <utility>
#include <vector>

#include "pair_list.hpp"

using namespace gdist;

static int failures = 0, lists = 0, cuts = 0;
static std::mt19937_64 size_rng(777);   // the set sizes' own stream: the lists stay the ones they were

#define EXPECT(cond, ...)                                \
    do {                                                 \
        if (!(cond)) {                                   \
            if (failures < 20) {                         \
                std::printf("FAIL %s: ", #cond);         \
                std::printf(__VA_ARGS__);                \
                std::printf("\n");                       \
            }                                            \
            failures++;                                  \
        }                                                \
    } while (0)

using Runs = std::vector<std::pair<uint64_t, int64_t>>;   // (row, pairs of the row), rows strictly ascending

// the sizes of a list's sets: a row's, and the column's of every sorted position
struct Sizes {
    std::vector<int64_t> row, col;   // [groups], [n]
};

enum SizeKind { ALL_ZERO, ALL_ONE, SMALL, ONE_HUGE, UNDER, ON, OVER, SIZE_KINDS };

// UNDER / ON / OVER: the first chunk holds kUnitCodesMin - 1 / + 0 / + 1 codes and nothing else holds
// any, so the budget is kUnitCodesMin for any number of CUs
static Sizes make_sizes(const Runs& runs, int64_t n, int kind) {
    auto& rng = size_rng;
    Sizes s;
    s.row.assign(runs.size(), kind == ALL_ONE ? 1 : 0);
    s.col.assign(n, kind == ALL_ONE ? 1 : 0);
    if (kind == SMALL || kind == ONE_HUGE) {
        for (auto& v : s.row) v = (int64_t)(rng() % 3000);
        for (auto& v : s.col) v = (int64_t)(rng() % 3000);
    }
    if (kind == ONE_HUGE) (rng() & 1 ? s.row[rng() % s.row.size()] : s.col[rng() % n]) = int64_t(1) << 22;
    if (kind >= UNDER) s.col[0] = kUnitCodesMin + (kind - ON);
    return s;
}

// pl_plan_kernel, the scan and pl_units_kernel with the segment cut
static void check_cut(const uint64_t* keys, int64_t n, const Runs& runs, const Sizes& sz, int kind, int nseg, int cus,
                      const char* what) {
    cuts++;
    std::vector<int64_t> group_of(n);
    int64_t at = 0;
    for (size_t g = 0; g < runs.size(); g++)
        for (int64_t t = 0; t < runs[g].second; t++) group_of[at++] = (int64_t)g;
    // the host's half (pairs() in pairs.hip): the list's codes over its pairs, both sets
    double codes = 0;
    for (int64_t k = 0; k < n; k++) codes += (double)(sz.row[group_of[k]] + sz.col[k]);
    const int64_t budget = pl_budget(codes, cus), ucap = pl_unit_cap(n, codes, budget);
    EXPECT(budget >= kUnitCodesMin && budget <= kUnitCodesMax, "%s budget %lld", what, (long long)budget);
    if (kind >= UNDER) EXPECT(budget == kUnitCodesMin, "%s budget %lld", what, (long long)budget);
    std::vector<int32_t> ucount(n);
    int64_t chunks = 0;
    for (int64_t k = 0; k < n; k++) {
        int32_t u = 0;
        if (pl_unit_head(keys, k)) {
            const int c = pl_unit_pairs(keys, n, k);
            int64_t cc = sz.row[group_of[k]];
            for (int t = 0; t < c; t++) cc += sz.col[k + t];
            u = pl_chunk_units(cc, budget, nseg);
            chunks++;
            EXPECT(u >= 1 && u <= nseg, "%s chunk at %lld: %d units of %d segments", what, (long long)k, u, nseg);
            if (kind == ALL_ZERO) EXPECT(u == 1, "%s empty chunk at %lld: %d units", what, (long long)k, u);
            if (kind >= UNDER && k == 0)
                EXPECT(u == std::min(nseg, kind == OVER ? 2 : 1), "%s first chunk %d units", what, u);
        }
        ucount[k] = u;
    }
    std::vector<int64_t> ubase(n);
    int64_t acc = 0;
    for (int64_t k = 0; k < n; k++) {
        ubase[k] = acc;
        acc += ucount[k];
    }
    const int64_t total = ubase[n - 1] + ucount[n - 1];
    EXPECT(total <= ucap, "%s %lld units past the cap %lld", what, (long long)total, (long long)ucap);
    EXPECT(total >= chunks, "%s %lld units of %lld chunks", what, (long long)total, (long long)chunks);
    if (total > ucap) return;
    struct Unit { int64_t k; int c, s0, s1; };
    std::unique_ptr<Unit[]> units(new Unit[ucap]);        // exactly the cap, unchecked as in the kernel
    int64_t written = 0;
    for (int64_t k = 0; k < n; k++) {
        const int u = ucount[k];
        if (!u) continue;
        const int c = pl_unit_pairs(keys, n, k);
        for (int t = 0; t < u; t++, written++)
            units[ubase[k] + t] = Unit{k, c, pl_unit_seg(nseg, t, u), pl_unit_seg(nseg, t + 1, u)};
    }
    EXPECT(written == total, "%s %lld units written of %lld", what, (long long)written, (long long)total);
    for (int64_t u = 0; u < total; u++) {
        const Unit& un = units[u];
        const bool first = u == 0 || units[u - 1].k != un.k, last = u + 1 == total || units[u + 1].k != un.k;
        EXPECT(un.s0 < un.s1, "%s unit %lld: empty range %d .. %d", what, (long long)u, un.s0, un.s1);
        EXPECT(un.s0 == (first ? 0 : units[u - 1].s1), "%s unit %lld starts at %d", what, (long long)u, un.s0);
        if (last) EXPECT(un.s1 == nseg, "%s unit %lld ends at %d of %d", what, (long long)u, un.s1, nseg);
        EXPECT(first || units[u - 1].c == un.c, "%s unit %lld: %d pairs", what, (long long)u, un.c);
    }
}

// every SizeKind x nseg x CUs (all), or one of each drawn at random plus the empty sets
static void check_list(const Runs& runs, const char* what, bool all) {
    lists++;
    int64_t n = 0, want_units = 0;
    for (auto& r : runs) {
        n += r.second;
        want_units += (r.second + kPairUnit - 1) / kPairUnit;
    }
    if (n == 0) return;                                   // the library plans no empty list
    std::unique_ptr<uint64_t[]> keys(new uint64_t[n]);    // exactly n: no slack behind the list
    int64_t at = 0;
    for (auto& r : runs)
        for (int64_t t = 0; t < r.second; t++) keys[at++] = r.first;
    // pl_plan_kernel, a chunk a unit
    std::vector<int32_t> uhead(n);
    int64_t groups = 0;
    for (int64_t k = 0; k < n; k++) {
        groups += pl_group_head(keys.get(), k) ? 1 : 0;
        uhead[k] = pl_unit_head(keys.get(), k) ? 1 : 0;
        EXPECT(pl_run_begin(keys.get(), k) <= k && keys[pl_run_begin(keys.get(), k)] == keys[k], "%s k=%lld", what,
               (long long)k);
    }
    // the scan
    std::vector<int64_t> ubase(n);
    int64_t acc = 0;
    for (int64_t k = 0; k < n; k++) {
        ubase[k] = acc;
        acc += uhead[k];
    }
    const int64_t nunits = ubase[n - 1] + uhead[n - 1];
    // pl_units_kernel
    std::vector<std::pair<int64_t, int>> units(nunits, {-1, 0});
    for (int64_t k = 0; k < n; k++)
        if (uhead[k]) units[ubase[k]] = {k, pl_unit_pairs(keys.get(), n, k)};
    EXPECT(groups == (int64_t)runs.size(), "%s groups %lld want %zu", what, (long long)groups, runs.size());
    EXPECT(nunits == want_units, "%s units %lld want %lld", what, (long long)nunits, (long long)want_units);
    EXPECT(nunits <= n, "%s units %lld of %lld pairs", what, (long long)nunits, (long long)n);
    std::vector<int> seen(n, 0);
    for (int64_t u = 0; u < nunits; u++) {
        const int64_t k0 = units[u].first;
        const int c = units[u].second;
        EXPECT(k0 >= 0 && c >= 1 && c <= kPairUnit && k0 + c <= n, "%s unit %lld: k0 %lld pairs %d", what,
               (long long)u, (long long)k0, c);
        if (k0 < 0 || k0 + c > n) continue;
        for (int t = 0; t < c; t++) {
            seen[k0 + t]++;
            EXPECT(keys[k0 + t] == keys[k0], "%s unit %lld holds two rows", what, (long long)u);
        }
        // short of the cap only where the run ends
        if (c < kPairUnit) EXPECT(k0 + c == n || keys[k0 + c] != keys[k0], "%s unit %lld stops early", what, (long long)u);
    }
    for (int64_t k = 0; k < n; k++) EXPECT(seen[k] == 1, "%s position %lld in %d units", what, (long long)k, seen[k]);
    // the kmer cut
    const int nsegs[4] = {1, 2, 64, 1024}, cus[2] = {1, 256};
    const int drawn = (int)(1 + size_rng() % (SIZE_KINDS - 1));
    for (int kind = 0; kind < SIZE_KINDS; kind++) {
        if (!all && kind != ALL_ZERO && kind != drawn) continue;
        const Sizes sz = make_sizes(runs, n, kind);
        const int pick = (int)(size_rng() % 8);
        for (int q = 0; q < 8; q++)
            if (all || q == pick) check_cut(keys.get(), n, runs, sz, kind, nsegs[q & 3], cus[q >> 2], what);
    }
}

int main() {
    // one run of every length around the cap and its multiples
    for (int64_t len : {1, 2, 63, 64, 65, 127, 128, 129, 200, 640, 641, 4097})
        check_list({{7, len}}, "one run", true);
    // the largest and the smallest row, runs that end on, before and past the cap, side by side
    check_list({{0, 64}, {1, 1}, {2, 65}, {3, 63}, {UINT64_MAX >> 1, 128}, {UINT64_MAX, 129}}, "edges", true);
    check_list({{0, 1}, {1, 1}, {2, 1}, {3, 1}}, "singles", true);
    check_list({{5, 200}, {6, 1}}, "long then single", true);
    check_list({{5, 1}, {6, 200}}, "single then long", true);
    check_list({}, "empty", true);
    std::mt19937_64 rng(12345);
    for (int it = 0; it < 400; it++) {
        Runs runs;
        const int nr = 1 + (int)(rng() % 40);
        uint64_t row = rng() % 5;
        for (int r = 0; r < nr; r++) {
            const int kind = (int)(rng() % 4);
            const int64_t len = kind == 0 ? 1 : kind == 1 ? 1 + (int64_t)(rng() % 8)
                              : kind == 2 ? 60 + (int64_t)(rng() % 10) : 1 + (int64_t)(rng() % 400);
            runs.push_back({row, len});
            row += 1 + rng() % 1000;
        }
        check_list(runs, "random", false);
    }
    std::printf("%d lists, %d cuts, %d failures\n", lists, cuts, failures);
    return failures ? 1 : 0;
}
