// sketch_pairs_plan.hpp — the unit cut of a sketch pair list (sketch_pairs.hip).
// Host and device code over plain pointers: tests/sketch_pairs_check.cpp walks
// sorted lists through it under the sanitizers without a device; the plan
// kernels call these same functions, a thread a sorted position.
//
// keys[0, n) are the list's rows in ascending order (the stable sort of the
// pair positions by row). A run of equal keys is a group; a group is cut into
// units of at most kSkpUnitPairs consecutive sorted positions, so a unit holds
// one row, no unit is empty and every position lies in exactly one unit:
// units = sum over the groups of ceil(run / kSkpUnitPairs).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GDIST_SKP_HD __host__ __device__ __forceinline__
#else
#define GDIST_SKP_HD inline
#endif

namespace gdist {

constexpr int kSkpUnitPairs = 64;   // the cap gdist_pairs documents

// first position of the run that holds sorted position k
GDIST_SKP_HD int64_t skp_run_begin(const uint64_t* keys, int64_t k) {
    const uint64_t key = keys[k];
    int64_t lo = 0, hi = k;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// sorted position k is the first of a group
GDIST_SKP_HD bool skp_group_head(const uint64_t* keys, int64_t k) { return k == 0 || keys[k - 1] != keys[k]; }

// sorted position k is the first of a unit
GDIST_SKP_HD bool skp_unit_head(const uint64_t* keys, int64_t k) {
    return ((k - skp_run_begin(keys, k)) % kSkpUnitPairs) == 0;
}

// pairs of the unit that starts at sorted position k: what is left of its run,
// at most kSkpUnitPairs; never reads at or past n
GDIST_SKP_HD int skp_unit_pairs(const uint64_t* keys, int64_t n, int64_t k) {
    const uint64_t key = keys[k];
    int c = 1;
    while (c < kSkpUnitPairs && k + c < n && keys[k + c] == key) c++;
    return c;
}

}  // namespace gdist
