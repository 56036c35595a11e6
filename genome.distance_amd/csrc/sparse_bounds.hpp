// sparse_bounds.hpp — chunk bounds of the sparse words at equal modelled cost.
//
// Host only, no HIP: the plan of sparse.hip calls it, and a stand-alone test
// program compiles it with the host compiler alone.
//
// The sparse words of a tile are walked in chunks, one workgroup each. A word
// with z holders costs z (z - 1) / 2 products, and the locus order puts the
// expensive words last, so chunks of equal word count differ in cost by more
// than a factor of two. The costs are kept per granule of kCostGranule words
// (sparse_granule_costs); balanced_bounds cuts [0, Ws) where the cumulative
// cost crosses k / n of the total, at granule boundaries.
//
// Exactness (16-bit counters): a chunk of at most `cap` words is always
// exact. A longer one is exact only if the caller's predicate says so for
// (first word, end word, chunk index); the index matters because the first
// `slabs` chunks also fold a dense-word slab. A chunk that fails is split
// until it passes, so the result may hold more chunks than asked.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gdist {

constexpr int kCostGranule = 16;          // sparse words per entry of the cost profile

// products z (z - 1) / 2 of the sparse words, summed per granule
inline std::vector<double> sparse_granule_costs(const int32_t* z, int64_t Ws) {
    std::vector<double> c((size_t)((Ws + kCostGranule - 1) / kCostGranule), 0.0);
    for (int64_t k = 0; k < Ws; k++) c[(size_t)(k / kCostGranule)] += 0.5 * (double)z[k] * ((double)z[k] - 1.0);
    return c;
}

// chunk bounds at equal word counts (n chunks)
inline std::vector<int32_t> equal_count_bounds(int64_t Ws, int64_t n) {
    std::vector<int32_t> b;
    for (int64_t c = 0; c <= n; c++) b.push_back((int32_t)(Ws * c / n));
    return b;
}

// cost of the words [b0, b1): whole granules, and a granule the range cuts by
// its share of words
inline double range_cost(const std::vector<double>& cost, int64_t Ws, int64_t b0, int64_t b1) {
    double t = 0.0;
    for (int64_t g = b0 / kCostGranule; g * kCostGranule < b1; g++) {
        const int64_t g0 = g * kCostGranule, g1 = std::min<int64_t>(g0 + kCostGranule, Ws);
        const int64_t lo = std::max(b0, g0), hi = std::min(b1, g1);
        if (hi > lo) t += cost[(size_t)g] * (double)(hi - lo) / (double)(g1 - g0);
    }
    return t;
}

// n chunks (at least `slabs`) of equal cumulative cost to within one granule:
// bound k is the granule boundary nearest the point at which the cumulative
// cost reaches k / n of the total, kept strictly increasing. With `weight`
// (n relative chunk costs) chunk k gets weight[k] / sum of the total instead
// of 1 / n. Then every chunk longer than `cap` words that
// `exact(b0, b1, index)` refuses is halved (by cost, at a granule boundary
// where one lies inside; else by words) until it is accepted or no longer
// than cap.
template <class Exact>
std::vector<int32_t> balanced_bounds(const std::vector<double>& cost, int64_t Ws, int64_t n, int64_t slabs,
                                     int64_t cap, Exact exact, const std::vector<double>& weight = {}) {
    n = std::max<int64_t>(std::max<int64_t>(n, slabs), 1);
    if (n > Ws) return equal_count_bounds(Ws, n);          // more chunks than words: some stay empty
    std::vector<double> share((size_t)n + 1, 0.0);         // cumulative share of the total before chunk k
    {
        const bool weighted = (int64_t)weight.size() == n;
        for (int64_t k = 0; k < n; k++) share[(size_t)k + 1] = share[(size_t)k] + (weighted ? weight[(size_t)k] : 1.0);
        for (int64_t k = 0; k <= n; k++) share[(size_t)k] /= share[(size_t)n];
    }
    const int64_t G = (int64_t)cost.size();
    std::vector<double> cum((size_t)G + 1, 0.0);
    for (int64_t g = 0; g < G; g++) cum[(size_t)g + 1] = cum[(size_t)g] + cost[(size_t)g];
    const double total = cum[(size_t)G];
    std::vector<int32_t> b{0};
    int64_t g = 0;
    for (int64_t k = 1; k < n; k++) {
        const double want = total * share[(size_t)k];
        // the boundary nearest the crossing: after granule g while that leaves the cumulative cost closer
        while (g < G && cum[(size_t)g + 1] - want <= want - cum[(size_t)g]) g++;
        int64_t w = std::min<int64_t>(g * kCostGranule, Ws);
        // strictly increasing, and room for a word in each chunk still to come
        w = std::max<int64_t>(w, (int64_t)b.back() + 1);
        w = std::min<int64_t>(w, Ws - (n - k));
        b.push_back((int32_t)w);
    }
    b.push_back((int32_t)Ws);
    if (total <= 0.0) b = equal_count_bounds(Ws, n);        // nothing to balance
    for (size_t c = 0; c + 1 < b.size();) {
        const int64_t b0 = b[c], b1 = b[c + 1];
        if (b1 - b0 <= cap || b1 - b0 < 2 || exact(b0, b1, (int64_t)c)) { c++; continue; }
        // the granule boundary inside (b0, b1) nearest half the chunk's cost
        const double half = 0.5 * range_cost(cost, Ws, b0, b1);
        int64_t mid = -1;
        double acc = 0.0, best = -1.0;
        for (int64_t q = b0 / kCostGranule; q * kCostGranule < b1; q++) {
            const int64_t e = std::min<int64_t>((q + 1) * kCostGranule, Ws);
            acc += range_cost(cost, Ws, std::max<int64_t>(b0, q * kCostGranule), std::min(e, b1));
            if (e <= b0 || e >= b1) continue;
            const double d = acc > half ? acc - half : half - acc;
            if (best < 0.0 || d < best) { best = d; mid = e; }
        }
        // by words instead where the cut by cost is lopsided: a long cheap
        // run would otherwise take many rounds to come under the cap
        if (mid < 0 || std::max(mid - b0, b1 - mid) > (b1 - b0) * 3 / 4) mid = b0 + (b1 - b0) / 2;
        b.insert(b.begin() + (std::ptrdiff_t)c + 1, (int32_t)mid);
    }
    return b;
}

}  // namespace gdist
