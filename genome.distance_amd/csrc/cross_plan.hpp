// cross_plan.hpp — the work units of a cross-collection join (cross.hip), pure
// host code (tests/cross_plan_check.cpp runs it under the sanitizers without a
// device).
//
// A region is query rows [q0, q1) against subject columns [c0, c1). The
// columns are cut into blocks of kCrossCols from c0; a unit is (query row,
// column block, segment range [p0, p1) of the subjects' segment index). A
// (row, block) whose codes |Q_i| + sum |S_j| exceed the budget is cut into
// u = clamp(ceil(codes / budget), 1, nseg) even ranges nseg t / u, as
// pl_unit_seg (pair_list.hpp) cuts a chunk of a pair list; the units of one
// (row, block) add their integer counts into the same cells, which is exact.
// A row whose set is empty gets no unit: its cells stay zero.
//
// Order: column block major; within a block the rows that are cut alike stand
// together (fewest cuts first) and go range by range, rows ascending within a
// range. Consecutive units then read the same segments of the same 64 subject
// sets (a row's own ranges side by side would read 64 whole sets between
// them). cross_unit_walk hands each XCD (workgroup b runs on XCD b mod 8) a
// contiguous run of that order.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define GDIST_CROSS_HD __host__ __device__
#else
#define GDIST_CROSS_HD
#endif

namespace gdist {

constexpr int kCrossCols = 64;                // subject columns a unit holds at most
// pairs.hip's constants: the region's codes over kCrossUnitsPerCU units a CU,
// within [kCrossCodesMin, kCrossCodesMax]
constexpr int64_t kCrossCodesMin = 1 << 14, kCrossCodesMax = 1 << 18;
constexpr int kCrossUnitsPerCU = 8;

// 16 bytes: row and cb are relative to the region (row q0 + row, columns from
// c0 + cb * kCrossCols)
struct CrossUnit {
    int32_t row, cb, p0, p1;
};

// codes of sets [a, b) from an offsets mirror
inline int64_t cross_codes(const int64_t* off, int64_t a, int64_t b) { return off[b] - off[a]; }

// the region's codes: every (non-empty row, block) reads its row and its block
inline double cross_region_codes(const int64_t* qoff, int64_t q0, int64_t q1, const int64_t* soff, int64_t c0,
                                 int64_t c1) {
    if (q1 <= q0 || c1 <= c0) return 0.0;
    int64_t rows = 0;
    for (int64_t i = q0; i < q1; i++) rows += qoff[i + 1] > qoff[i];
    const int64_t ncb = (c1 - c0 + kCrossCols - 1) / kCrossCols;
    return (double)ncb * (double)cross_codes(qoff, q0, q1) + (double)rows * (double)cross_codes(soff, c0, c1);
}

inline int64_t cross_budget(double region_codes, int cus) {
    const double per = region_codes / ((double)std::max(cus, 1) * kCrossUnitsPerCU);
    if (!(per > (double)kCrossCodesMin)) return kCrossCodesMin;
    if (per > (double)kCrossCodesMax) return kCrossCodesMax;
    return (int64_t)per;
}

// ranges a (row, block) of `codes` codes is cut into
inline int cross_cuts(int64_t codes, int64_t budget, int nseg) {
    const int64_t want = (codes + budget - 1) / budget;
    return (int)(want < 1 ? 1 : (want > nseg ? nseg : want));
}

// appends the region's units to `units` (not cleared); nseg >= 1, budget >= 1,
// q1 - q0 and the block count within int32
inline void cross_plan(const int64_t* qoff, int64_t q0, int64_t q1, const int64_t* soff, int64_t c0, int64_t c1,
                       int nseg, int64_t budget, std::vector<CrossUnit>& units) {
    if (q1 <= q0 || c1 <= c0) return;
    const int64_t ncb = (c1 - c0 + kCrossCols - 1) / kCrossCols;
    std::vector<std::pair<int32_t, int32_t>> rows;   // (cuts, row) of the block's non-empty rows
    for (int64_t cb = 0; cb < ncb; cb++) {
        const int64_t cs = c0 + cb * kCrossCols, ce = std::min<int64_t>(c1, cs + kCrossCols);
        const int64_t bcodes = cross_codes(soff, cs, ce);
        rows.clear();
        for (int64_t i = q0; i < q1; i++) {
            const int64_t na = qoff[i + 1] - qoff[i];
            if (na) rows.emplace_back(cross_cuts(na + bcodes, budget, nseg), (int32_t)(i - q0));
        }
        std::sort(rows.begin(), rows.end());
        // rows cut alike, range by range
        for (size_t g0 = 0; g0 < rows.size();) {
            const int u = rows[g0].first;
            size_t g1 = g0;
            while (g1 < rows.size() && rows[g1].first == u) g1++;
            for (int t = 0; t < u; t++)
                for (size_t g = g0; g < g1; g++)
                    units.push_back(CrossUnit{rows[g].second, (int32_t)cb, (int32_t)((int64_t)nseg * t / u),
                                              (int32_t)((int64_t)nseg * (t + 1) / u)});
            g0 = g1;
        }
    }
}

// The units workgroup b of G walks: first, first + stride, ... below end.
// XCD x = b mod 8 owns the run [x per, (x + 1) per) of the plan's order,
// per = ceil(nunits / 8), shared by the workgroups of that XCD. Every unit is
// walked by exactly one workgroup when G >= min(nunits, 8).
GDIST_CROSS_HD inline void cross_unit_walk(int64_t G, int64_t b, int64_t nunits, int64_t* first, int64_t* end,
                                           int64_t* stride) {
    const int64_t x = b & 7, slot = b >> 3;
    const int64_t per = (nunits + 7) >> 3;
    const int64_t lo = x * per, hi = lo + per < nunits ? lo + per : nunits;
    *stride = (G - x + 7) >> 3;                 // workgroups of this XCD
    *first = lo + slot;
    *end = hi;
}

}  // namespace gdist
