// Stand-alone check of csrc/cross_plan.hpp (the work units of the
// cross-collection join): built by tests/test_cross_plan.py with the host
// compiler under AddressSanitizer + UBSan, no device.
//
// For a set of regions it verifies that every (non-empty row, column block,
// segment) is covered by exactly one unit, that a (row, block) is cut into
// clamp(ceil(codes / budget), 1, nseg) even ranges, that the order is column
// block major (within a block: rows cut alike together, range by range), that
// the budget is clamped at both ends, and that
// cross_unit_walk hands every unit to exactly one workgroup.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cross_plan.hpp"

using gdist::CrossUnit;

static int checks = 0, failures = 0;

#define CHECK(cond, ...)                         \
    do {                                         \
        checks++;                                \
        if (!(cond)) {                           \
            failures++;                          \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);            \
            std::printf("\n");                   \
        }                                        \
    } while (0)

static std::vector<int64_t> offsets(const std::vector<int64_t>& sizes) {
    std::vector<int64_t> off(sizes.size() + 1, 0);
    for (size_t i = 0; i < sizes.size(); i++) off[i + 1] = off[i] + sizes[i];
    return off;
}

// deterministic sizes in [lo, hi]
static std::vector<int64_t> sizes_of(int n, int64_t lo, int64_t hi, uint64_t seed) {
    std::vector<int64_t> v(n);
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
    for (int i = 0; i < n; i++) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        v[i] = lo + (int64_t)(x % (uint64_t)(hi - lo + 1));
    }
    return v;
}

static void check_region(const char* name, const std::vector<int64_t>& qs, int64_t q0, int64_t q1,
                         const std::vector<int64_t>& ss, int64_t c0, int64_t c1, int nseg, int64_t budget) {
    const std::vector<int64_t> qoff = offsets(qs), soff = offsets(ss);
    std::vector<CrossUnit> units;
    gdist::cross_plan(qoff.data(), q0, q1, soff.data(), c0, c1, nseg, budget, units);
    const int64_t nr = q1 > q0 ? q1 - q0 : 0, nc = c1 > c0 ? c1 - c0 : 0;
    const int64_t ncb = (nc + gdist::kCrossCols - 1) / gdist::kCrossCols;
    // cover[(row, block)][segment]
    std::vector<int> cover((size_t)(nr * ncb * nseg), 0), cuts((size_t)(nr * ncb), 0);
    bool in_range = true, ordered = true, even = true;
    for (const CrossUnit& u : units) {
        if (u.row < 0 || u.row >= nr || u.cb < 0 || u.cb >= ncb || u.p0 < 0 || u.p0 >= u.p1 || u.p1 > nseg) {
            in_range = false;
            continue;
        }
        cuts[(size_t)(u.row * ncb + u.cb)]++;
        for (int p = u.p0; p < u.p1; p++) cover[(size_t)((u.row * ncb + u.cb) * nseg + p)]++;
    }
    // order: column block, then the (row, block)'s cut count, then the range,
    // then the row; a (row, block)'s t-th unit holds the range nseg t / u
    {
        std::vector<int> seen((size_t)(nr * ncb), 0);
        int64_t prev[4] = {-1, -1, -1, -1};
        for (const CrossUnit& x : units) {
            if (x.row < 0 || x.row >= nr || x.cb < 0 || x.cb >= ncb) continue;
            const int u = cuts[(size_t)(x.row * ncb + x.cb)];
            const int t = seen[(size_t)(x.row * ncb + x.cb)]++;
            if (x.p0 != (int64_t)nseg * t / u || x.p1 != (int64_t)nseg * (t + 1) / u) even = false;
            const int64_t key[4] = {x.cb, u, t, x.row};
            bool less = false;
            for (int k = 0; k < 4; k++) {
                if (prev[k] != key[k]) {
                    less = prev[k] < key[k];
                    break;
                }
            }
            if (!less) ordered = false;
            for (int k = 0; k < 4; k++) prev[k] = key[k];
        }
    }
    CHECK(in_range, "%s: a unit outside the region", name);
    CHECK(ordered, "%s: units are not ordered by (column block, cuts, range, row)", name);
    bool exact = true, cut_ok = true;
    for (int64_t a = 0; a < nr; a++) {
        const int64_t na = qs[(size_t)(q0 + a)];
        for (int64_t cb = 0; cb < ncb; cb++) {
            const int64_t cs = c0 + cb * gdist::kCrossCols, ce = cs + gdist::kCrossCols < c1 ? cs + gdist::kCrossCols : c1;
            const int64_t codes = na + (soff[(size_t)ce] - soff[(size_t)cs]);
            int64_t want = (codes + budget - 1) / budget;
            want = want < 1 ? 1 : (want > nseg ? nseg : want);
            const int got = cuts[(size_t)(a * ncb + cb)];
            if (na == 0) {
                if (got != 0) cut_ok = false;
            } else if (got != want) {
                cut_ok = false;
            }
            for (int p = 0; p < nseg; p++)
                if (cover[(size_t)((a * ncb + cb) * nseg + p)] != (na == 0 ? 0 : 1)) exact = false;
        }
    }
    CHECK(exact, "%s: a (row, block, segment) is not covered exactly once", name);
    CHECK(cut_ok, "%s: a (row, block) is not cut into clamp(ceil(codes / budget), 1, nseg) units", name);
    CHECK(even, "%s: ranges are not nseg t / u", name);

    // every unit walked by exactly one workgroup
    const int64_t nu = (int64_t)units.size();
    for (int64_t G : {int64_t(1), int64_t(3), int64_t(8), int64_t(13), int64_t(512)}) {
        const int64_t g = G < nu ? G : nu;
        if (g < (nu < 8 ? nu : 8)) continue;                   // the launch keeps G >= min(nunits, 8)
        std::vector<int> seen((size_t)nu, 0);
        bool inside = true, contiguous = true;
        for (int64_t b = 0; b < g; b++) {
            int64_t first, end, stride;
            gdist::cross_unit_walk(g, b, nu, &first, &end, &stride);
            if (stride < 1) { inside = false; continue; }
            const int64_t per = (nu + 7) / 8;
            for (int64_t u = first; u < end; u += stride) {
                if (u < 0 || u >= nu) { inside = false; break; }
                if (u / per != (b & 7)) contiguous = false;   // XCD x owns the run [x per, (x + 1) per)
                seen[(size_t)u]++;
            }
        }
        bool once = true;
        for (int64_t u = 0; u < nu; u++) once = once && seen[(size_t)u] == 1;
        CHECK(inside, "%s: G = %lld walks outside the units", name, (long long)g);
        CHECK(once, "%s: G = %lld does not walk every unit exactly once", name, (long long)g);
        CHECK(contiguous, "%s: G = %lld: an XCD walks outside its run", name, (long long)g);
    }
}

int main() {
    const std::vector<int64_t> q52 = sizes_of(52, 1, 6000, 1), s143 = sizes_of(143, 0, 6000, 2);
    std::vector<int64_t> qe = q52;
    qe[0] = qe[17] = qe[51] = 0;                               // empty rows: first, middle, last

    check_region("fixture shape", qe, 0, 52, s143, 0, 143, 3, 20000);
    check_region("nseg 1", qe, 0, 52, s143, 0, 143, 1, 20000);
    check_region("ragged last block", qe, 0, 52, s143, 60, 143, 3, 20000);
    check_region("sub-rows", qe, 5, 37, s143, 60, 143, 3, 20000);
    check_region("one row", qe, 3, 4, s143, 0, 143, 3, 20000);
    check_region("one empty row", qe, 17, 18, s143, 0, 143, 3, 20000);
    check_region("zero columns", qe, 0, 52, s143, 70, 70, 3, 20000);
    check_region("zero rows", qe, 9, 9, s143, 0, 143, 3, 20000);
    check_region("one column", qe, 0, 52, s143, 142, 143, 3, 20000);
    check_region("exactly one block", qe, 0, 52, s143, 0, 64, 3, 20000);
    check_region("block plus one", qe, 0, 52, s143, 0, 65, 3, 20000);
    check_region("budget 1 (u = nseg)", qe, 0, 52, s143, 0, 143, 7, 1);
    check_region("huge budget (u = 1)", qe, 0, 52, s143, 0, 143, 7, int64_t(1) << 40);
    check_region("lower clamp", qe, 0, 52, s143, 0, 143, 64, gdist::kCrossCodesMin);
    check_region("upper clamp", qe, 0, 52, s143, 0, 143, 64, gdist::kCrossCodesMax);
    // one query of 40,000 codes against 4,096 subjects of the same size
    {
        const std::vector<int64_t> q1{40000}, s4k(4096, 40000);
        const std::vector<int64_t> qoff = offsets(q1), soff = offsets(s4k);
        const double codes = gdist::cross_region_codes(qoff.data(), 0, 1, soff.data(), 0, 4096);
        CHECK(codes == 64.0 * 40000 + 4096.0 * 40000, "region codes %.0f", codes);
        const int64_t budget = gdist::cross_budget(codes, 256);
        CHECK(budget == (int64_t)(codes / 2048.0), "budget %lld", (long long)budget);
        check_region("one query, 4,096 subjects", q1, 0, 1, s4k, 0, 4096, 20, budget);
        std::vector<CrossUnit> units;
        gdist::cross_plan(qoff.data(), 0, 1, soff.data(), 0, 4096, 20, budget, units);
        CHECK(units.size() == 64u * 20u, "one query against 4,096 subjects: %zu units", units.size());
    }

    // the budget: the region's codes over 8 units a CU, clamped at both ends
    CHECK(gdist::cross_budget(0.0, 256) == gdist::kCrossCodesMin, "empty region budget");
    CHECK(gdist::cross_budget(1e6, 256) == gdist::kCrossCodesMin, "small region budget");
    CHECK(gdist::cross_budget(2048.0 * 100000, 256) == 100000, "mid region budget");
    CHECK(gdist::cross_budget(1e15, 256) == gdist::kCrossCodesMax, "large region budget");
    CHECK(gdist::cross_budget(1e9, 0) == gdist::kCrossCodesMax, "no CU count");
    CHECK(gdist::kCrossCodesMin == 1 << 14 && gdist::kCrossCodesMax == 1 << 18 && gdist::kCrossUnitsPerCU == 8 &&
              gdist::kCrossCols == 64, "constants of pairs.hip");
    CHECK(gdist::cross_cuts(0, 100, 5) == 1 && gdist::cross_cuts(100, 100, 5) == 1 &&
              gdist::cross_cuts(101, 100, 5) == 2 && gdist::cross_cuts(100000, 100, 5) == 5, "cross_cuts");
    // empty rows do not count their block's codes
    {
        const std::vector<int64_t> q{0, 10, 0}, s{5, 7};
        const std::vector<int64_t> qoff = offsets(q), soff = offsets(s);
        CHECK(gdist::cross_region_codes(qoff.data(), 0, 3, soff.data(), 0, 2) == 10.0 + 12.0, "region codes");
        CHECK(gdist::cross_region_codes(qoff.data(), 0, 1, soff.data(), 0, 2) == 0.0, "empty row region");
        CHECK(gdist::cross_region_codes(qoff.data(), 0, 3, soff.data(), 1, 1) == 0.0, "no columns region");
    }
    CHECK(sizeof(CrossUnit) == 16, "16-byte unit records");

    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
