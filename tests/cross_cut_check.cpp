// cross_cut_check.cpp — where a query row is cut by the subjects' splitters
// (csrc/cross_cut.hpp) without a device: the search the join kernel of
// gdist_cross_pairs runs per work unit, on arrays of exactly the sizes the
// library holds (a row of n codes, nseg - 1 splitters, the kCrossCutMax cut
// points the kernel reserves in LDS) so that a read or a write past them is
// the sanitizers' to report.
//
// For rows that are empty, entirely below the first splitter, entirely above
// the last, entirely inside one segment, holding codes equal to splitters, and
// random, with nseg 1 .. 4,096: the cut points of [0, nseg] start at 0, end at
// n and never descend, so the segments tile the row; every code of segment t
// lies in [split[t - 1], split[t]) (a code equal to a splitter opens its
// segment, as in the subjects' own index); a workgroup's 512 threads write
// what one worker writes; and the units of a chunk (pl_unit_seg), each
// searching its own range only into an array of exactly that many entries,
// agree where they meet, so their sub-runs tile the row too.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "cross_cut.hpp"
#include "pair_list.hpp"

using namespace gdist;

static int failures = 0, rows_checked = 0;

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

// exactly n elements on the heap: no slack behind them
template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

static void check_row(std::vector<uint64_t> codes, const std::vector<uint64_t>& splitv, const char* what) {
    rows_checked++;
    std::sort(codes.begin(), codes.end());
    codes.erase(std::unique(codes.begin(), codes.end()), codes.end());
    const int64_t n = (int64_t)codes.size();
    const int nseg = (int)splitv.size() + 1;
    auto row = exact(codes);
    auto split = exact(splitv);
    // the whole row, into what the kernel reserves
    std::unique_ptr<uint32_t[]> cut(new uint32_t[kCrossCutMax]);
    std::fill(cut.get(), cut.get() + kCrossCutMax, 0xDEADBEEFu);
    xc_cuts(row.get(), n, split.get(), nseg, 0, nseg, cut.get(), 0, 1);
    EXPECT(cut[0] == 0, "%s nseg %d: first cut %u", what, nseg, cut[0]);
    EXPECT(cut[nseg] == (uint32_t)n, "%s nseg %d: last cut %u of %lld", what, nseg, cut[nseg], (long long)n);
    for (int t = nseg + 1; t < kCrossCutMax; t++)
        EXPECT(cut[t] == 0xDEADBEEFu, "%s nseg %d: slot %d past the range written", what, nseg, t);
    for (int t = 0; t < nseg; t++) {
        EXPECT(cut[t] <= cut[t + 1], "%s nseg %d: cut %d descends (%u > %u)", what, nseg, t, cut[t], cut[t + 1]);
        if (cut[t] > cut[t + 1] || cut[t + 1] > (uint32_t)n) continue;
        for (uint32_t e = cut[t]; e < cut[t + 1]; e++) {
            if (t > 0) EXPECT(row[e] >= split[t - 1], "%s nseg %d: code %u below segment %d", what, nseg, e, t);
            if (t + 1 < nseg) EXPECT(row[e] < split[t], "%s nseg %d: code %u above segment %d", what, nseg, e, t);
        }
    }
    // a workgroup's threads, a cut point each in turn
    std::unique_ptr<uint32_t[]> wg(new uint32_t[kCrossCutMax]);
    for (int me = 0; me < 512; me++) xc_cuts(row.get(), n, split.get(), nseg, 0, nseg, wg.get(), me, 512);
    for (int t = 0; t <= nseg; t++) EXPECT(wg[t] == cut[t], "%s nseg %d: thread's cut %d", what, nseg, t);
    // the units of a chunk, each its own range
    for (int u : {1, 2, 3, 7, nseg}) {
        if (u > nseg) continue;
        uint32_t at = 0;
        for (int t = 0; t < u; t++) {
            const int first = pl_unit_seg(nseg, t, u), end = pl_unit_seg(nseg, t + 1, u);
            EXPECT(first < end && end <= nseg, "%s nseg %d: unit %d of %d is %d .. %d", what, nseg, t, u, first, end);
            if (first >= end || end > nseg) continue;
            std::unique_ptr<uint32_t[]> own(new uint32_t[end - first + 1]);
            for (int me = 0; me < 512; me++) xc_cuts(row.get(), n, split.get(), nseg, first, end, own.get(), me, 512);
            EXPECT(own[0] == at, "%s nseg %d: unit %d of %d starts at %u, the one before ended at %u", what, nseg, t,
                   u, own[0], at);
            for (int k = 0; k <= end - first; k++)
                EXPECT(own[k] == cut[first + k], "%s nseg %d: unit %d of %d cut %d", what, nseg, t, u, k);
            at = own[end - first];
        }
        EXPECT(at == (uint32_t)n, "%s nseg %d: %d units end at %u of %lld", what, nseg, u, at, (long long)n);
    }
}

int main() {
    std::mt19937_64 rng(20261021);
    for (int nseg : {1, 2, 3, 4, 5, 64, 1000, 4095, 4096}) {
        // strictly ascending splitters away from both ends of the code space
        std::vector<uint64_t> split;
        const uint64_t lo = uint64_t(1) << 40, step = (UINT64_MAX - (uint64_t(1) << 41)) / (uint64_t)nseg;
        for (int t = 1; t < nseg; t++) split.push_back(lo + step * (uint64_t)t + rng() % (step / 2));
        const uint64_t first = nseg > 1 ? split.front() : lo, last = nseg > 1 ? split.back() : lo;
        check_row({}, split, "empty");
        check_row({0}, split, "code 0");
        check_row({UINT64_MAX}, split, "all ones");
        std::vector<uint64_t> v;
        for (int e = 0; e < 5000; e++) v.push_back(rng() % first);
        v.push_back(0);
        check_row(v, split, "below the first splitter");
        v.clear();
        for (int e = 0; e < 5000; e++) v.push_back(last + 1 + rng() % (UINT64_MAX - last - 1));
        v.push_back(UINT64_MAX);
        check_row(v, split, "above the last splitter");
        // inside one segment: a window of 2^30 codes behind a splitter (or behind lo)
        for (int pick = 0; pick < 3; pick++) {
            const uint64_t base = nseg > 1 ? split[rng() % split.size()] : lo;
            v.clear();
            for (int e = 0; e < 20000; e++) v.push_back(base + 1 + rng() % (uint64_t(1) << 30));
            check_row(v, split, "inside one segment");
        }
        // codes equal to splitters: every splitter, then every other one with its neighbours
        v = split;
        check_row(v, split, "the splitters themselves");
        v.clear();
        for (size_t t = 0; t < split.size(); t += 2) {
            v.push_back(split[t] - 1);
            v.push_back(split[t]);
            v.push_back(split[t] + 1);
        }
        check_row(v, split, "around splitters");
        v = split;
        v.push_back(0);
        v.push_back(UINT64_MAX);
        for (int e = 0; e < 3000; e++) v.push_back(rng());
        check_row(v, split, "splitters and random codes");
        v.clear();
        for (int e = 0; e < 30000; e++) v.push_back(rng());
        check_row(v, split, "random");
    }
    // splitters at the ends of the code space and next to each other
    check_row({0, 1, 2, 3, UINT64_MAX - 1, UINT64_MAX}, {0, 1, 2, UINT64_MAX}, "extreme splitters");
    check_row({}, {0, UINT64_MAX}, "extreme splitters, empty row");
    check_row({5}, {5}, "one code on the one splitter");
    std::printf("%d rows, %d failures\n", rows_checked, failures);
    return failures ? 1 : 0;
}
