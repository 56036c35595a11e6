// reps_resolve.hpp — the host side of greedy representative selection on a
// row block: what is left once the device has said which rows an earlier
// block's representative covers and has filled the block's own tile.
// Pure host code, no HIP include: tests/reps_resolve_check.cpp compiles it
// with the host compiler under sanitizers against a brute-force loop.
//
// The rules are gdist_greedy_reps's (include/gdist.h): sets in index order;
// a set becomes a representative unless an earlier representative lies within
// t, a plain fp64 d <= t (so NaN never covers, and d == 1.0 covers when
// t >= 1.0).
#pragma once
#include <cstddef>
#include <cstdint>

namespace gdist {

// Pass 1, rows [b0, b0 + nb): cov[k] != 0 when a representative of an earlier
// block covers row k; tile is [nb][nb], its upper triangle filled:
// tile[j * nb + k] = d(b0 + j, b0 + k) for j < k, which is d(b0 + k, b0 + j)
// (the distance is symmetric bit for bit); nothing else of it is read.
// Writes is_rep[b0 .. b0 + nb) (is_rep indexes the
// whole collection) and appends the new representatives' set indices, in
// order, to new_reps (room for nb); returns their number.
inline int64_t reps_resolve_block(int64_t b0, int64_t nb, const int32_t* cov, const double* tile, double t,
                                  int32_t* is_rep, int64_t* new_reps) {
    // is_rep[b0 + k] starts as "not covered yet"; when the walk reaches row j
    // every earlier representative has swept it, so an uncovered j is one, and
    // sweeps its own row of the tile (contiguous) over the rows after it
    int64_t count = 0;
    for (int64_t k = 0; k < nb; k++) is_rep[b0 + k] = cov[k] != 0 ? 0 : 1;
    for (int64_t j = 0; j < nb; j++) {
        if (!is_rep[b0 + j]) continue;
        new_reps[count++] = b0 + j;
        const double* row = tile + (size_t)j * nb;
        for (int64_t k = j + 1; k < nb; k++)
            if (row[k] <= t) is_rep[b0 + k] = 0;
    }
    return count;
}

// Pass 2, rows [b0, b0 + nb): best[k] / best_d[k] are the device's closest
// representative of row k (set index, -1 / 1.0 when none). A representative
// maps to itself at 0.0 whatever the device found. Either output may be null.
inline void reps_assign_block(int64_t b0, int64_t nb, const int32_t* is_rep, const int64_t* best,
                              const double* best_d, int64_t* rep_of, double* rep_dist) {
    for (int64_t k = 0; k < nb; k++) {
        const int64_t g = b0 + k;
        const bool self = is_rep[g] != 0;
        if (rep_of) rep_of[g] = self ? g : best[k];
        if (rep_dist) rep_dist[g] = self ? 0.0 : (best[k] < 0 ? 1.0 : best_d[k]);
    }
}

}  // namespace gdist
