// pair_list.hpp — the cut of a pair list into units (pair_list.hip; gdist_pairs
// and gdist_sketch_pairs). Host and device code over plain pointers:
// tests/pair_list_check.cpp walks sorted lists through it under the sanitizers
// without a device; the plan kernels call these same functions, a thread a
// sorted position.
//
// keys[0, n) are the list's rows in ascending order (the stable sort of the
// pair positions by row). A run of equal keys is a group; a group is cut into
// chunks of at most kPairUnit consecutive sorted positions, so a chunk holds
// one row, no chunk is empty and every position lies in exactly one chunk:
// chunks = sum over the groups of ceil(run / kPairUnit). A sketch chunk is one
// unit. A kmer chunk of the sorted path whose codes (its row's set plus its
// columns' sets) exceed the call's budget is cut into several units, each a
// range of the segment index (sorted.hip build_segments).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GDIST_PL_HD __host__ __device__ __forceinline__
#else
#define GDIST_PL_HD inline
#endif

namespace gdist {

constexpr int kPairUnit = 64;   // pairs of one row a unit holds at most: the cap gdist_pairs documents

// first position of the run that holds sorted position k
GDIST_PL_HD int64_t pl_run_begin(const uint64_t* keys, int64_t k) {
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
GDIST_PL_HD bool pl_group_head(const uint64_t* keys, int64_t k) { return k == 0 || keys[k - 1] != keys[k]; }

// sorted position k is the first of a chunk
GDIST_PL_HD bool pl_unit_head(const uint64_t* keys, int64_t k) {
    return ((k - pl_run_begin(keys, k)) % kPairUnit) == 0;
}

// pairs of the chunk that starts at sorted position k: what is left of its run,
// at most kPairUnit; never reads at or past n
GDIST_PL_HD int pl_unit_pairs(const uint64_t* keys, int64_t n, int64_t k) {
    const uint64_t key = keys[k];
    int c = 1;
    while (c < kPairUnit && k + c < n && keys[k + c] == key) c++;
    return c;
}

// The code budget of the sorted kmer path: the list's codes (over its pairs,
// both sets) over kUnitsPerCu units a CU, within [kUnitCodesMin,
// kUnitCodesMax]: a short list is cut finer, a few pairs of huge sets still
// fill the chip.
constexpr int64_t kUnitCodesMin = 1 << 14, kUnitCodesMax = 1 << 18;
constexpr int kUnitsPerCu = 8;

inline int64_t pl_budget(double codes, int cus) {
    const int64_t b = (int64_t)(codes / ((double)cus * kUnitsPerCu));
    return b < kUnitCodesMin ? kUnitCodesMin : (b > kUnitCodesMax ? kUnitCodesMax : b);
}

// the most units the plan makes of n pairs with that budget: a chunk a pair,
// and a cut per budget of the chunks' codes (a chunk counts its row once, the
// list's codes once a pair). The units kernel writes within this bound unchecked.
inline int64_t pl_unit_cap(int64_t n, double codes, int64_t budget) {
    return n + (int64_t)(codes / (double)budget) + 1;
}

// units of a chunk of `codes` codes: 1 .. nseg
GDIST_PL_HD int pl_chunk_units(int64_t codes, int64_t budget, int nseg) {
    const int64_t want = (codes + budget - 1) / budget;
    return (int)(want < 1 ? 1 : (want > nseg ? nseg : want));
}

// first segment of unit t of a chunk's u: unit t takes [pl_unit_seg(t), pl_unit_seg(t + 1)) of [0, nseg)
GDIST_PL_HD int pl_unit_seg(int nseg, int t, int u) { return (int)((int64_t)nseg * t / u); }

}  // namespace gdist
