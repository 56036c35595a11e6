// sketch_wave_merge.hpp — one sketch pair by the 64 lanes of a wave: the
// device side of sketch_cross_merge.hpp, shared by the kernels that give a
// wave a pair (sketch_cross.hip: the pairs of a rectangle; sketch_pairs.hip:
// the pairs of a list). The signatures may lie in LDS or in global memory.
#pragma once

#include <hip/hip_runtime.h>

#include "sketch_cross_merge.hpp"

namespace gdist {

__device__ __forceinline__ int skx_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int skx_wave_scan(int v, int lane) {   // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

// one pair by the 64 lanes of a wave; every lane returns the pair's result
__device__ __forceinline__ void skx_pair_merge(const int32_t* Q, int nq, const int32_t* S, int ns, int width,
                                               int jaccard, int empty_nan, int lane, int* common_out,
                                               double* d_out) {
    const bool qa = nq >= ns;
    const int32_t* A = qa ? Q : S;
    const int32_t* B = qa ? S : Q;
    const int na = qa ? nq : ns, nb = qa ? ns : nq;
    const int ca = skx_chunk(na);
    int a0, a1;
    skx_a_range(na, ca, lane, &a0, &a1);
    const int b0 = skx_b_begin(A, na, B, nb, ca, lane);
    int b1 = __shfl_down(b0, 1, 64);
    if (lane == kSkxLanes - 1) b1 = nb;
    uint64_t mask;
    const int c = skx_merge(A, a0, a1, B, b0, b1, &mask);
    int common, taken;
    if (jaccard) {
        common = skx_wave_sum(c);
        taken = na + nb - common;
    } else {
        const int uni = (a1 - a0) + (b1 - b0) - c;
        const int incl = skx_wave_scan(uni, lane);
        taken = skx_taken(__shfl(incl, kSkxLanes - 1, 64), width, 0);
        common = skx_wave_sum(skx_lane_common(A, a0, a1, B, b0, b1, incl - uni, uni, c, mask, taken));
    }
    *common_out = common;
    *d_out = skx_distance(common, taken, na, nb, jaccard, empty_nan);
}

}  // namespace gdist
