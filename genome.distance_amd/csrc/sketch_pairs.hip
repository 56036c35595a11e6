// sketch_pairs.hip — the sketch distances of an arbitrary (row, column) pair
// list in one call (gdist_sketch_pairs).
//
// The lists of the reference that name their pairs: the methods table
// (MethodTableProcessor.java:258-276), one genome against a column list, and
// the chosen pairs the width comparison sets beside the exact distance
// (WidthProcessor.java:183-192). The rectangle kernels do not fit: 10^5
// scattered pairs among 50,000 sketches are 4e-5 of their bounding rectangle.
//
// Plan (PairList, pair_list.hip: one upload, no host round trip): the pair
// positions sorted by row and cut into units of at most kPairUnit consecutive
// pairs of one row. A signature is at most `width` hashes, so there is no code
// budget and a pair is never split. The merge kernel reads the number of units
// from device memory and strides over them.
//
// sketch_pairs_kernel: a workgroup of 16 waves takes units in a grid-stride
// loop, up to kRows consecutive ones a step: a scattered list's units hold
// ~20 pairs, and 16 waves on one such unit leave the second round a quarter
// full; the pairs of a step's units go to the waves in turn as one run. A
// short list is not batched (every workgroup keeps kStepsPerWg steps).
//   LDS variant: a unit's row signature is staged once (one flat coalesced
//   copy by the whole workgroup); each wave then copies its pair's column
//   signature into its own LDS slice (64 lanes, coalesced, at most `width`
//   dwords) and merges the two with the wave-per-pair merge of the cross kernel
//   (skx_pair_merge). The merge is a chain of dependent reads at data-dependent
//   addresses: ~2 width / 64 short steps from LDS, an HBM / L2 latency each
//   from global memory; the gather stays one wide load a signature. Rows and
//   slices are sw = width | 1 dwords apart, so they start on different banks.
//   (1 + 16) sw dwords a unit, 68 KB at width 1000; with kRows = 4 rows 80 KB,
//   still two workgroups in a CU's 160 KiB: what hides the merge latency is
//   waves. Fewer rows a step where only fewer fit (widths 1,024 .. 1,203).
//   Global variant (a row and the slices past kLdsBytes): the same walk,
//   searching and merging straight from global memory. Width 20,000 runs here.
// Lane 0 stores the pair's common count and / or distance at the pair's
// original position: every position is in exactly one unit, so nothing is
// zeroed and nothing at or past npairs is touched.
#include "gdist_internal.hpp"
#include "sketch_wave_merge.hpp"

namespace gdist {
namespace {

constexpr int kNT = 1024, kNW = kNT / 64;   // threads, waves of a workgroup
constexpr int kLdsBytes = 80 * 1024;        // a workgroup's signatures: two workgroups in a CU's 160 KiB
constexpr int kWgPerCu = 2;                 // 16-wave workgroups a CU holds
constexpr int kRows = 4;                    // units a workgroup holds at a time, at most
constexpr int kStepsPerWg = 4;              // steps a workgroup keeps before units are batched

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Rows index (asig, aoff), columns (bsig, boff). A workgroup holds up to
// `nrows` (<= kRows) consecutive units at a time; LDS: sm holds (nrows + kNW) sw
// dwords, the units' row signatures first, then a slice a wave.
// 8 waves a SIMD are two workgroups a CU: the registers are held to that
template <bool LDS>
__global__ __launch_bounds__(kNT) __attribute__((amdgpu_waves_per_eu(8, 8))) void sketch_pairs_kernel(
    const int32_t* __restrict__ asig, const int64_t* __restrict__ aoff, const int32_t* __restrict__ bsig,
    const int64_t* __restrict__ boff, int width, int sw, int nrows, const uint64_t* __restrict__ keys,
    const int32_t* __restrict__ vals, const int64_t* __restrict__ cols, const int2* __restrict__ units,
    const unsigned long long* __restrict__ counts, int jaccard, int empty_nan, int32_t* __restrict__ common_out,
    double* __restrict__ D) {
    extern __shared__ int32_t sm[];
    __shared__ int64_t s_k0[kRows], s_rb[kRows];
    __shared__ int s_la[kRows], s_np[kRows];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nunits = (int64_t)counts[1];
    // units a step: as many as fit while every workgroup still gets a few steps
    const int64_t share = nunits / ((int64_t)kStepsPerWg * gridDim.x);
    const int R = (int)(share < 1 ? 1 : (share > nrows ? nrows : share));
    int32_t* mine = sm + (nrows + wave) * sw;
    for (int64_t u0 = (int64_t)blockIdx.x * R; u0 < nunits; u0 += (int64_t)gridDim.x * R) {
        const int nu = (int)(nunits - u0 < R ? nunits - u0 : R);
        __syncthreads();   // the previous step's pairs are done with the rows and their table
        if ((int)threadIdx.x < nu) {
            const int2 un = units[u0 + threadIdx.x];
            const int64_t i = (int64_t)keys[un.x];
            const int64_t rb = aoff[i], rl = aoff[i + 1] - rb;
            s_k0[threadIdx.x] = un.x;
            s_np[threadIdx.x] = un.y;                           // 1 .. kPairUnit
            s_rb[threadIdx.x] = rb;
            s_la[threadIdx.x] = (int)(rl < width ? rl : width);   // no signature is longer than the width
        }
        __syncthreads();
        if (LDS) {
            for (int r = 0; r < nu; r++) {
                const int32_t* src = asig + s_rb[r];
                const int la = s_la[r];
                for (int e = threadIdx.x; e < la; e += kNT) sm[r * sw + e] = src[e];
            }
            __syncthreads();
        }
        int total = 0;
        for (int r = 0; r < nu; r++) total += s_np[r];
        // the step's pairs, unit after unit, to the waves in turn
        for (int t = wave; t < total; t += kNW) {
            int r = 0, first = 0;
            while (r + 1 < nu && t >= first + s_np[r]) first += s_np[r++];
            const int32_t pos = vals[s_k0[r] + (t - first)];
            const int64_t j = cols[pos];
            const int64_t cb = boff[j], cl = boff[j + 1] - cb;
            const int la = s_la[r], lb = (int)(cl < width ? cl : width);
            const int32_t *Q = asig + s_rb[r], *S = bsig + cb;
            if (LDS) {
                const int32_t* src = bsig + cb;
                wave_sync();   // the wave's previous pair is done with the slice
                constexpr int U = 4;   // loads in flight a lane
                for (int e0 = lane; e0 < lb; e0 += 64 * U) {
                    int32_t v[U];
#pragma unroll
                    for (int q = 0; q < U; q++) v[q] = e0 + q * 64 < lb ? src[e0 + q * 64] : 0;
#pragma unroll
                    for (int q = 0; q < U; q++)
                        if (e0 + q * 64 < lb) mine[e0 + q * 64] = v[q];
                }
                wave_sync();
                Q = sm + r * sw;
                S = mine;
            }
            int common;
            double d;
            skx_pair_merge(Q, la, S, lb, width, jaccard, empty_nan, lane, &common, &d);
            if (lane == 0) {
                if (common_out) common_out[pos] = common;
                if (D) D[pos] = d;
            }
        }
    }
}

}  // namespace

// every argument checked by the caller, n > 0; rows / cols / common_out / D_out:
// host, n entries, either output may be null
void sketch_pairs(gdist_ctx* ctx, const gdist_sets* a, const gdist_sets* b, unsigned flags, int64_t n,
                  const int64_t* rows, const int64_t* cols, int32_t* common_out, double* D_out) {
    hipStream_t st = ctx->stream;
    PairList pl(ctx, a->nsets, n, rows, cols, common_out, D_out, false);   // every position is stored once
    pl.plan_units();

    const int width = std::max(1, a->width), sw = width | 1;
    // rows a step: what fits beside the 16 slices, at most kRows; none: the global variant
    const int fit = kLdsBytes / 4 / sw - kNW;
    const int nrows = fit >= 1 ? std::min(kRows, fit) : kRows;
    const int jaccard = (flags & GDIST_SKETCH_JACCARD) ? 1 : 0, empty_nan = (flags & GDIST_EMPTY_NAN) ? 1 : 0;
    const unsigned grid = (unsigned)std::min<int64_t>(n, (int64_t)std::max(ctx->cus, 1) * kWgPerCu);
    if (fit >= 1) {
        const size_t bytes = (size_t)(nrows + kNW) * sw * 4;   // <= kLdsBytes
        auto kern = &sketch_pairs_kernel<true>;
        GD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kLdsBytes));
        kern<<<grid, kNT, bytes, st>>>(a->codes.as<int32_t>(), a->off.as<int64_t>(), b->codes.as<int32_t>(),
                                       b->off.as<int64_t>(), width, sw, nrows, pl.keys, pl.vals, pl.cols,
                                       pl.units.as<int2>(), pl.counts, jaccard, empty_nan, pl.I, pl.D);
    } else {
        sketch_pairs_kernel<false><<<grid, kNT, 0, st>>>(
            a->codes.as<int32_t>(), a->off.as<int64_t>(), b->codes.as<int32_t>(), b->off.as<int64_t>(), width, sw,
            nrows, pl.keys, pl.vals, pl.cols, pl.units.as<int2>(), pl.counts, jaccard, empty_nan, pl.I, pl.D);
    }
    GD_HIP(hipGetLastError());
    pl.finish();
}

}  // namespace gdist
