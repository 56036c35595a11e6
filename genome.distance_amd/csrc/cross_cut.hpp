// cross_cut.hpp — where a query row is cut by the subjects' splitters
// (cross_pairs.hip; gdist_cross_pairs). Host and device code over plain
// pointers: tests/cross_cut_check.cpp runs the search under the sanitizers
// without a device; the join kernel calls these same functions, a thread a cut
// point.
//
// The subjects' segment index (sorted.hip build_segments) cuts every subject
// set by nseg - 1 strictly ascending splitters: segment t holds the codes v
// with split[t - 1] <= v < split[t]. Segment t of a query can only meet
// segment t of a subject, so a query row (sorted distinct codes) is cut at the
// same values: cut[0] = 0, cut[nseg] = n and, between them, cut[t] = the first
// position whose code is >= split[t - 1], the lower bound segoff_kernel takes.
// The cut points are not cached anywhere: a work unit finds those of its own
// segment range [first, end], end - first + 1 <= kCrossCutMax of them, 32-bit
// relative to the row's start.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GDIST_XC_HD __host__ __device__ __forceinline__
#else
#define GDIST_XC_HD inline
#endif

namespace gdist {

constexpr int kCrossSegMax = 4096;                // the most segments an index has (sorted.hip build_segments)
constexpr int kCrossCutMax = kCrossSegMax + 1;    // cut points of a whole row: what the kernel reserves

// cut point t in [0, nseg] of a row of n sorted codes; split: nseg - 1
// splitters, not read for t == 0 or t == nseg
GDIST_XC_HD uint32_t xc_cut(const uint64_t* row, int64_t n, const uint64_t* split, int nseg, int t) {
    if (t <= 0) return 0;
    if (t >= nseg) return (uint32_t)n;
    const uint64_t v = split[t - 1];
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (row[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return (uint32_t)lo;
}

// out[t - first] = cut point t for t in [first, end], the share of worker
// `me` of `workers` (a thread of the workgroup; 0 of 1 on the host):
// 0 <= first < end <= nseg, out holds end - first + 1 entries
GDIST_XC_HD void xc_cuts(const uint64_t* row, int64_t n, const uint64_t* split, int nseg, int first, int end,
                         uint32_t* out, int me, int workers) {
    for (int t = first + me; t <= end; t += workers) out[t - first] = xc_cut(row, n, split, nseg, t);
}

}  // namespace gdist
