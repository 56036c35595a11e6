// sketch_cross_merge.hpp — the wave-per-pair segmented merge of two sketch
// signatures (sketch_cross.hip). Host and device code over plain pointers:
// tests/sketch_cross_check.cpp runs the 64 lanes of a pair in a loop under the
// sanitizers without a device; the kernel runs them as the lanes of a wave and
// calls these same functions.
//
// Signatures are strictly increasing signed int32; INT_MIN and INT_MAX are
// real hashes, so nothing here uses a sentinel value.
//
// A is the longer signature (na >= nb). Lane t of kSkxLanes owns the A
// positions [t ca, (t + 1) ca) clamped to na and the B positions
// [skx_b_begin(t), skx_b_begin(t + 1)): the B elements >= its first A element
// and < the next lane's first. Lane 0 also takes the B elements below A[0];
// the lane whose A range ends at na takes B to its end; a lane without A
// elements owns nothing. Every element of lane t (of A or B) is below every
// element of lane t + 1, so the sorted union of the pair is the lanes' unions
// one after the other, and a common element is common within one lane.
//
// ca = skx_chunk(na) is ceil(na / 64) made odd. Any ca >= ceil(na / 64) gives
// the same result; an odd one puts the 64 lanes' positions t ca + r (one r)
// into 64 different LDS banks, where the even 16 of a 1,000-wide signature
// would put them into 4.
//
// Jaccard (GDIST_SKETCH_JACCARD): common = sum of the lanes' skx_merge.
// Mash: the first T = min(width, sum of the lanes' unions) union elements
// count. With `before` the exclusive prefix sum of the unions, a lane whose
// segment ends within T gives its common, one that starts at or past T gives
// nothing, and the one lane that straddles T counts the common elements among
// the T - before union elements it may still take (skx_lane_common): from the
// bit mask its merge left for its first 64 union elements, or, past them (a
// signature of more than ~2,000 hashes), by merging again with a cap.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GDIST_SKX_HD __host__ __device__ __forceinline__
#else
#define GDIST_SKX_HD inline
#endif

namespace gdist {

constexpr int kSkxLanes = 64;

// A positions a lane owns
GDIST_SKX_HD int skx_chunk(int na) { return ((na + kSkxLanes - 1) / kSkxLanes) | 1; }

// first position of B[0, n) whose value is >= v
GDIST_SKX_HD int skx_lb(const int32_t* B, int n, int32_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (B[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// where lane t's B range starts; lane t's range ends where lane t + 1's starts
// (t = kSkxLanes: nb)
GDIST_SKX_HD int skx_b_begin(const int32_t* A, int na, const int32_t* B, int nb, int ca, int t) {
    if (t == 0) return 0;
    const int64_t a0 = (int64_t)t * ca;
    if (a0 >= na) return nb;
    return skx_lb(B, nb, A[a0]);
}

// lane t's A range
GDIST_SKX_HD void skx_a_range(int na, int ca, int t, int* a0, int* a1) {
    const int64_t s = (int64_t)t * ca, e = s + ca;
    *a0 = (int)(s < na ? s : na);
    *a1 = (int)(e < na ? e : na);
}

// common elements among the first `cap` union elements of A[a0, a1) and B[b0, b1)
GDIST_SKX_HD int skx_merge_capped(const int32_t* A, int a0, int a1, const int32_t* B, int b0, int b1, int cap) {
    int ia = a0, ib = b0, steps = 0;
    while (ia < a1 && ib < b1 && steps < cap) {
        const int32_t va = A[ia], vb = B[ib];
        ia += va <= vb;
        ib += vb <= va;
        steps++;
    }
    // a step over a common element advanced both sides; what one side has
    // left once the other is exhausted holds no common element
    return (ia - a0) + (ib - b0) - steps;
}

// common elements of the two segments; their union is (a1 - a0) + (b1 - b0) - common.
// *mask: bit k set when the segment's k-th union element (k < 64) is a common
// one, so the common elements among its first cap <= 64 are a popcount
GDIST_SKX_HD int skx_merge(const int32_t* A, int a0, int a1, const int32_t* B, int b0, int b1, uint64_t* mask) {
    int ia = a0, ib = b0, steps = 0;
    uint64_t m = 0;
    while (ia < a1 && ib < b1) {
        const int32_t va = A[ia], vb = B[ib];
        if (steps < 64) m |= (uint64_t)(va == vb) << steps;
        ia += va <= vb;
        ib += vb <= va;
        steps++;
    }
    *mask = m;
    return (ia - a0) + (ib - b0) - steps;
}

// Mash: what a lane adds to the pair's common. before: union elements of the
// lanes below it; uni / common / mask: its own segment's (skx_merge); T: union
// elements that count. Only a lane that straddles T past its 64th union
// element merges again
GDIST_SKX_HD int skx_lane_common(const int32_t* A, int a0, int a1, const int32_t* B, int b0, int b1, int before,
                                 int uni, int common, uint64_t mask, int T) {
    if (before + uni <= T) return common;
    if (before >= T) return 0;
    const int cap = T - before;   // 1 .. uni - 1
    if (cap <= 64) return (int)__builtin_popcountll(cap == 64 ? mask : mask & ((uint64_t(1) << cap) - 1));
    return skx_merge_capped(A, a0, a1, B, b0, b1, cap);
}

// union elements that count: Mash min(width, union), Jaccard all of them
GDIST_SKX_HD int skx_taken(int uni_total, int width, int jaccard) {
    return (jaccard || uni_total < width) ? uni_total : width;
}

// The distance of sketch_tile_kernel (sketch.hip), fp64, no contraction (there
// is no multiply to contract): Jaccard from (common, na, nb) by the header's
// Java expression, Mash from (common, taken)
GDIST_SKX_HD double skx_distance(int common, int taken, int na, int nb, int jaccard, int empty_nan) {
    if (jaccard) {
        const int64_t la = na, lb = nb;
        if (common > 0) return 1.0 - (double)common / (double)(la + lb - common);
        return (empty_nan && la + lb == 0) ? __builtin_nan("") : 1.0;
    }
    if (common > 0) return 1.0 - (double)common / (double)taken;
    return (empty_nan && taken == 0) ? __builtin_nan("") : 1.0;
}

}  // namespace gdist
