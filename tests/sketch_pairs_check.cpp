// sketch_pairs_check.cpp — the unit cut of the sketch pair list
// (csrc/sketch_pairs_plan.hpp) without a device: the plan kernels' steps run in
// a loop over the sorted positions (mark the unit heads, exclusive scan, write
// the units), on key arrays of exactly n elements so that a read at or past n
// is the sanitizers' to report. Checked for every list: every sorted position
// lies in exactly one unit, no unit holds more than kSkpUnitPairs pairs or more
// than one row, no unit is empty, a unit never stops short of the cap inside a
// run, and the units and groups are the numbers gdist_ctx_pairs_info reports:
// sum over the rows of ceil(run / kSkpUnitPairs), and the distinct rows.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <utility>
#include <vector>

#include "sketch_pairs_plan.hpp"

using namespace gdist;

static int failures = 0, lists = 0;

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

// runs: (row, pairs of the row), rows strictly ascending
static void check_list(const std::vector<std::pair<uint64_t, int64_t>>& runs, const char* what) {
    lists++;
    int64_t n = 0, want_units = 0;
    for (auto& r : runs) {
        n += r.second;
        want_units += (r.second + kSkpUnitPairs - 1) / kSkpUnitPairs;
    }
    if (n == 0) return;                                   // the library plans no empty list
    std::unique_ptr<uint64_t[]> keys(new uint64_t[n]);    // exactly n: no slack behind the list
    int64_t at = 0;
    for (auto& r : runs)
        for (int64_t t = 0; t < r.second; t++) keys[at++] = r.first;
    // skp_plan_kernel
    std::vector<int32_t> uhead(n);
    int64_t groups = 0;
    for (int64_t k = 0; k < n; k++) {
        groups += skp_group_head(keys.get(), k) ? 1 : 0;
        uhead[k] = skp_unit_head(keys.get(), k) ? 1 : 0;
        EXPECT(skp_run_begin(keys.get(), k) <= k && keys[skp_run_begin(keys.get(), k)] == keys[k], "%s k=%lld", what,
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
    // skp_units_kernel
    std::vector<std::pair<int64_t, int>> units(nunits, {-1, 0});
    for (int64_t k = 0; k < n; k++)
        if (uhead[k]) units[ubase[k]] = {k, skp_unit_pairs(keys.get(), n, k)};
    EXPECT(groups == (int64_t)runs.size(), "%s groups %lld want %zu", what, (long long)groups, runs.size());
    EXPECT(nunits == want_units, "%s units %lld want %lld", what, (long long)nunits, (long long)want_units);
    std::vector<int> seen(n, 0);
    for (int64_t u = 0; u < nunits; u++) {
        const int64_t k0 = units[u].first;
        const int c = units[u].second;
        EXPECT(k0 >= 0 && c >= 1 && c <= kSkpUnitPairs && k0 + c <= n, "%s unit %lld: k0 %lld pairs %d", what,
               (long long)u, (long long)k0, c);
        if (k0 < 0 || k0 + c > n) continue;
        for (int t = 0; t < c; t++) {
            seen[k0 + t]++;
            EXPECT(keys[k0 + t] == keys[k0], "%s unit %lld holds two rows", what, (long long)u);
        }
        // short of the cap only where the run ends
        if (c < kSkpUnitPairs) EXPECT(k0 + c == n || keys[k0 + c] != keys[k0], "%s unit %lld stops early", what, (long long)u);
    }
    for (int64_t k = 0; k < n; k++) EXPECT(seen[k] == 1, "%s position %lld in %d units", what, (long long)k, seen[k]);
}

int main() {
    // one run of every length around the cap and its multiples
    for (int64_t len : {1, 2, 63, 64, 65, 127, 128, 129, 200, 640, 641, 4097})
        check_list({{7, len}}, "one run");
    // the largest and the smallest row, runs that end on, before and past the cap, side by side
    check_list({{0, 64}, {1, 1}, {2, 65}, {3, 63}, {UINT64_MAX >> 1, 128}, {UINT64_MAX, 129}}, "edges");
    check_list({{0, 1}, {1, 1}, {2, 1}, {3, 1}}, "singles");
    check_list({{5, 200}, {6, 1}}, "long then single");
    check_list({{5, 1}, {6, 200}}, "single then long");
    check_list({}, "empty");
    std::mt19937_64 rng(12345);
    for (int it = 0; it < 400; it++) {
        std::vector<std::pair<uint64_t, int64_t>> runs;
        const int nr = 1 + (int)(rng() % 40);
        uint64_t row = rng() % 5;
        for (int r = 0; r < nr; r++) {
            const int kind = (int)(rng() % 4);
            const int64_t len = kind == 0 ? 1 : kind == 1 ? 1 + (int64_t)(rng() % 8)
                              : kind == 2 ? 60 + (int64_t)(rng() % 10) : 1 + (int64_t)(rng() % 400);
            runs.push_back({row, len});
            row += 1 + rng() % 1000;
        }
        check_list(runs, "random");
    }
    std::printf("%d lists, %d failures\n", lists, failures);
    return failures ? 1 : 0;
}
