// width_sweep.hpp — the lane-level arithmetic of gdist_width_sweep
// (width_sweep.hip): one walk of a sketch pair's merged union that yields the
// pair's common count at EVERY sketch size of a list. Host and device code
// over plain pointers, as sketch_cross_merge.hpp: tests/width_sweep_check.cpp
// runs the 64 lanes of a pair in a loop under the sanitizers without a device;
// the kernel runs them as the lanes of a wave and calls these same functions.
//
// Two facts carry it ("Sketch error at every width").
//  Prefix: the bottom-s signature of a set is the first s hashes of its
//  bottom-S signature for any S >= s, so one collection built at the largest
//  size holds every smaller one.
//  Threshold: give a common element of the two full signatures the threshold
//    Mash     t = its 1-based rank in the union of the two signatures,
//    Jaccard  t = max(its index in a, its index in b) + 1;
//  then the pair of size-s sketches has common(s) = #{t <= s}, with
//  taken(s) = min(s, |a u b|) (Mash) or the lengths min(na, s), min(nb, s)
//  (Jaccard). The walk adds 1 to counter[first k with sizes[k] >= t] per
//  common element (t past the last size: dropped); the inclusive prefix sum of
//  the counters over k is common(sizes[k]).
//
// The lanes partition the pair as sketch_cross_merge.hpp describes (skx_chunk,
// skx_a_range, skx_b_begin): every element of lane t lies below every element
// of lane t + 1. Jaccard needs nothing more: a lane knows its elements'
// indices. Mash needs `before`, the union elements of the lanes below (the
// exclusive prefix sum of the lanes' unions), so a lane first merges its
// segments for their common count and the mask of its first 64 union steps
// (skx_merge); with `before` known it reads the ranks off the mask, and walks
// again only where its segment's union is longer than the mask.
//
// Nothing here uses a sentinel value: INT_MIN and INT_MAX are real hashes.
#pragma once

#include "sketch_cross_merge.hpp"

namespace gdist {

// counter[k] += 1 for the first k with sizes[k] >= t; none: dropped. The
// kernel's counters are shared by the lanes of a wave (LDS)
GDIST_SKX_HD void wsw_count(const int32_t* sizes, int nsizes, int32_t* counter, int t) {
    const int k = skx_lb(sizes, nsizes, t);
    if (k >= nsizes) return;
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(&counter[k], 1);
#else
    counter[k]++;
#endif
}

// Jaccard: the thresholds of the common elements of A[a0, a1) and B[b0, b1),
// positions within the whole signatures
GDIST_SKX_HD void wsw_walk_jaccard(const int32_t* A, int a0, int a1, const int32_t* B, int b0, int b1,
                                   const int32_t* sizes, int nsizes, int32_t* counter) {
    int ia = a0, ib = b0;
    while (ia < a1 && ib < b1) {
        const int32_t va = A[ia], vb = B[ib];
        if (va == vb) wsw_count(sizes, nsizes, counter, (ia > ib ? ia : ib) + 1);
        ia += va <= vb;
        ib += vb <= va;
    }
}

// Mash: the ranks of the segments' common elements. before: union elements of
// the lanes below; uni / mask: this segment's union and skx_merge's mask
GDIST_SKX_HD void wsw_walk_mash(const int32_t* A, int a0, int a1, const int32_t* B, int b0, int b1, int before,
                                int uni, uint64_t mask, const int32_t* sizes, int nsizes, int32_t* counter) {
    if (nsizes == 0 || before >= sizes[nsizes - 1]) return;   // every rank here is past the last size
    if (uni <= 64) {
        // the merge took at most `uni` steps: the mask holds all of them
        while (mask) {
            wsw_count(sizes, nsizes, counter, before + __builtin_ctzll(mask) + 1);
            mask &= mask - 1;
        }
        return;
    }
    int ia = a0, ib = b0, steps = 0;
    while (ia < a1 && ib < b1) {
        const int32_t va = A[ia], vb = B[ib];
        steps++;
        if (va == vb) wsw_count(sizes, nsizes, counter, before + steps);
        ia += va <= vb;
        ib += vb <= va;
    }
}

// The sketch distance at one size from the prefix-summed counter. na / nb: the
// signatures' lengths; uni_total: their union (Mash only)
GDIST_SKX_HD double wsw_distance(int common, int size, int na, int nb, int uni_total, int jaccard) {
    if (jaccard) return skx_distance(common, 0, na < size ? na : size, nb < size ? nb : size, 1, 0);
    return skx_distance(common, skx_taken(uni_total, size, 0), 0, 0, 0, 0);
}

}  // namespace gdist
