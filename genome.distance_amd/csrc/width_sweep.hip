// width_sweep.hip — the error of the sketch distance at every sketch size of
// a list, in one walk of the pairs (gdist_width_sweep): the per-size loop of
// WidthProcessor.ProcessGroup (WidthProcessor.java:153-208) without a sketch
// build, an all-pairs launch and a table download per size.
//
// The driver walks row blocks x column chunks of the KMER collection as
// closest() does (SelfSource, counts, upper triangle); per step the matrix
// kernels leave the block's intersection counts I in device memory and
// width_sweep_kernel meets them with the SKETCH collection built at the
// largest size: for every cell (i, j), j > i, a wave merges the two
// signatures once (width_sweep.hpp), which gives the common count at every
// size, forms the exact distance r from I and the set sizes and the sketch
// distance s_k per size, and where they differ adds the relative error
// e = |r - s_k| * 2 / (r + s_k) to size k's accumulators.
//
// width_sweep_kernel: a workgroup of 8 waves owns a run of `st` consecutive
// columns and a slab of the step's rows (grid.y).
//   LDS variant: the run's signatures are staged once as they lie in the
//   collection's CSR, then the slab's rows pass through in tiles of kQT,
//   staged the same way, and the waves take the tile's (row, column) pairs
//   with column > row in turn: a row's signature is staged once for all its
//   pairs of the run. The merge is a chain of dependent LDS reads; what hides
//   its latency is waves.
//   Global variant (a run of kMinRun signatures and the row tile past the LDS
//   budget): the same walk, searching and merging straight from global memory.
//
// Exactness (the precedent is group.hip). Per size the kernel keeps the count
// of differing pairs, the maximum of bits(e) (e > 0: the unsigned pattern
// orders it) and the sum of E = rint(e * 2^62) (e <= 2, so E <= 2^63) as two
// 32-bit digits, each added into its own 64-bit slot (carry-save): integer
// arithmetic only, so the result depends on neither the order of the pairs
// nor the block sizes, the method or the run. A workgroup accumulates in LDS
// (64-bit LDS atomics; the lanes of a wave own different sizes) and adds its
// non-zero slots to the call's accumulators with 64-bit global atomics when
// it ends. With fewer than 2^31 pairs a digit slot stays below 2^63. The host
// joins the digits.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "gdist_internal.hpp"
#include "sketch_wave_merge.hpp"
#include "width_sweep.hpp"

namespace gdist {
namespace {

constexpr int kNT = 512, kNW = kNT / 64;   // threads, waves of a workgroup
constexpr int kQT = 4;                     // rows staged at a time
constexpr int kMinRun = 4, kMaxRun = 32;   // columns a workgroup holds
constexpr int kLdsBytes = 60 * 1024;       // everything a workgroup holds: two workgroups a CU
constexpr int kSlots = 4;                  // per size: differing, max bits(e), low and high digit of sum E

// what a workgroup holds beside the signatures: the accumulators (kSlots a
// size and the pairs count), the size list, a counter a size for every wave
constexpr size_t fixed_bytes(int nsizes) { return (size_t)8 * (kSlots * nsizes + 1) + (size_t)4 * nsizes * (1 + kNW); }

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// stage_sets of sketch_cross.hip for this workgroup size: sets
// [first, first + n) of a CSR collection into LDS as they lie (at most cap
// dwords), rel[0 .. n] their bounds relative to off[first], clamped to cap.
// Called by the whole workgroup; the caller's barrier publishes both.
__device__ __forceinline__ void stage_sets(const int32_t* __restrict__ sig, const int64_t* __restrict__ off,
                                           int64_t first, int n, int cap, int32_t* dst, int32_t* rel) {
    const int64_t base = off[first];
    if ((int)threadIdx.x <= n) {
        const int64_t r = off[first + threadIdx.x] - base;
        rel[threadIdx.x] = (int32_t)(r < cap ? r : cap);
    }
    const int64_t all = off[first + n] - base;
    const int total = (int)(all < cap ? all : cap);
    const int32_t* src = sig + base;
    constexpr int U = 4;   // loads in flight a thread
    for (int i0 = threadIdx.x; i0 < total; i0 += kNT * U) {
        int32_t v[U];
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = i0 + u * kNT < total ? src[i0 + u * kNT] : 0;
#pragma unroll
        for (int u = 0; u < U; u++)
            if (i0 + u * kNT < total) dst[i0 + u * kNT] = v[u];
    }
}

// Rows [b0, b0 + nb) x columns [k0, k0 + nk) of the step: I is the block's
// intersection counts (row a / column b at I[a * nk + b]), koff the kmer
// sets' offsets, (sig, soff) the sketch collection. Workgroup (x, y) owns
// columns [k0 + x st, k0 + (x + 1) st) and rows [b0 + y rs, b0 + (y + 1) rs),
// st <= kMaxRun, rs a multiple of kQT. sizes: nsizes strictly increasing
// sketch sizes, the last one smax. acc: kSlots nsizes + 1 slots.
// LDS (dynamic): the accumulators, the size list, the waves' counters, then
// (LDS variant) (st + kQT) sw dwords of signatures, the columns' first.
template <bool LDS>
__global__ __launch_bounds__(kNT) void width_sweep_kernel(
    const int32_t* __restrict__ I, const int64_t* __restrict__ koff, const int32_t* __restrict__ sig,
    const int64_t* __restrict__ soff, int sw, int st, int64_t rs, int64_t b0, int64_t nb, int64_t k0, int64_t nk,
    int jaccard, const int32_t* __restrict__ sizes, int nsizes, unsigned long long* __restrict__ acc) {
#pragma clang fp contract(off)
    extern __shared__ unsigned long long wsw_lds[];
    __shared__ int32_t s_rel[kMaxRun + 1], q_rel[kQT + 1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nslots = kSlots * nsizes + 1;
    unsigned long long* lacc = wsw_lds;
    int32_t* sz = reinterpret_cast<int32_t*>(wsw_lds + nslots);
    int32_t* cnt = sz + nsizes + wave * nsizes;   // this wave's counters
    int32_t* sm = sz + nsizes * (1 + kNW);
    int32_t* qm = sm + st * sw;

    const int64_t j0 = (int64_t)blockIdx.x * st;   // relative to k0
    if (j0 >= nk) return;
    const int run = (int)(nk - j0 < st ? nk - j0 : st);   // <= kMaxRun
    // rows of the slab that have a column of the run to their right
    const int64_t t_begin = (int64_t)blockIdx.y * rs;
    const int64_t t_end = std::min(std::min(nb, t_begin + rs), k0 + j0 + run - 1 - b0);
    if (t_begin >= t_end) return;   // the whole workgroup: no barrier is left waiting

    for (int i = threadIdx.x; i < nslots; i += kNT) lacc[i] = 0ull;
    for (int i = threadIdx.x; i < nsizes; i += kNT) sz[i] = sizes[i];
    for (int i = threadIdx.x; i < nsizes * kNW; i += kNT) sz[nsizes + i] = 0;
    if (LDS) stage_sets(sig, soff, k0 + j0, run, st * sw, sm, s_rel);
    __syncthreads();
    const int smax = sz[nsizes - 1];

    const int64_t tile = LDS ? kQT : t_end - t_begin;
    for (int64_t t0 = t_begin; t0 < t_end; t0 += tile) {
        const int nq = (int)(t_end - t0 < tile ? t_end - t0 : tile);
        if (LDS) {
            __syncthreads();   // the previous tile's pairs are done with the rows
            stage_sets(sig, soff, b0 + t0, nq, kQT * sw, qm, q_rel);
            __syncthreads();
        }
        const int64_t npairs = (int64_t)nq * run;
        for (int64_t p = wave; p < npairs; p += kNW) {
            const int64_t r = p / run;
            const int s = (int)(p - r * run);
            const int64_t q = b0 + t0 + r, j = k0 + j0 + s;
            if (j <= q) continue;   // on or left of the diagonal (wave-uniform)
            const int32_t *Q, *S;
            int lq, ls;
            if (LDS) {
                Q = qm + q_rel[r];
                S = sm + s_rel[s];
                lq = q_rel[r + 1] - q_rel[r];
                ls = s_rel[s + 1] - s_rel[s];
            } else {
                const int64_t qb = soff[q], sb = soff[j];
                Q = sig + qb;
                S = sig + sb;
                lq = (int)(soff[q + 1] - qb);
                ls = (int)(soff[j + 1] - sb);
            }
            // no size reads past the first smax hashes of a signature
            lq = lq < smax ? lq : smax;
            ls = ls < smax ? ls : smax;

            // the merge: a threshold per common element into the wave's counters
            const bool qa = lq >= ls;
            const int32_t* A = qa ? Q : S;
            const int32_t* B = qa ? S : Q;
            const int na = qa ? lq : ls, nbb = qa ? ls : lq;
            const int ca = skx_chunk(na);
            int a0, a1;
            skx_a_range(na, ca, lane, &a0, &a1);
            const int bb0 = skx_b_begin(A, na, B, nbb, ca, lane);
            int bb1 = __shfl_down(bb0, 1, 64);
            if (lane == kSkxLanes - 1) bb1 = nbb;
            int uni_total = 0;
            if (jaccard) {
                wsw_walk_jaccard(A, a0, a1, B, bb0, bb1, sz, nsizes, cnt);
            } else {
                uint64_t mask;
                const int c = skx_merge(A, a0, a1, B, bb0, bb1, &mask);
                const int uni = (a1 - a0) + (bb1 - bb0) - c;
                const int incl = skx_wave_scan(uni, lane);
                uni_total = __shfl(incl, kSkxLanes - 1, 64);
                wsw_walk_mash(A, a0, a1, B, bb0, bb1, incl - uni, uni, mask, sz, nsizes, cnt);
            }
            wave_sync();   // every lane's counts are in

            // the exact distance: the Java expression of epilogue_kernel
            // (matrix_step.hip) and the other consumers, fp64, no contraction
            const int64_t inter = I[(t0 + r) * nk + j0 + s];
            const int64_t ka = koff[q + 1] - koff[q], kb = koff[j + 1] - koff[j];
            double real = 1.0;
            if (inter > 0) real = 1.0 - (double)inter / (double)(ka + kb - inter);
            if (lane == 0 && real < 1.0) atomicAdd(&lacc[nslots - 1], 1ull);

            // lane k, k + 64, ... takes size k: the counters' inclusive prefix
            // sum is the common count at that size
            int carry = 0;
            for (int base = 0; base < nsizes; base += 64) {
                const int k = base + lane;
                int v = 0;
                if (k < nsizes) {
                    v = cnt[k];
                    cnt[k] = 0;   // for the wave's next pair
                }
                const int common = skx_wave_scan(v, lane) + carry;
                carry = __shfl(common, 63, 64);
                if (k < nsizes) {
                    const double d = wsw_distance(common, sz[k], lq, ls, uni_total, jaccard);
                    if (real != d) {
                        const double e = fabs(real - d) * 2.0 / (real + d);
                        // exact: a scale by a power of two, then one rounding (ties to even)
                        const unsigned long long E = __double2ull_rn(e * 4611686018427387904.0);
                        unsigned long long* a = lacc + (size_t)kSlots * k;
                        atomicAdd(a, 1ull);
                        atomicMax(a + 1, (unsigned long long)__double_as_longlong(e));
                        atomicAdd(a + 2, E & 0xffffffffull);
                        atomicAdd(a + 3, E >> 32);
                    }
                }
            }
            wave_sync();   // the counters are zero before the next pair adds
        }
    }

    __syncthreads();
    for (int i = threadIdx.x; i < nslots; i += kNT) {
        const unsigned long long v = lacc[i];
        if (!v) continue;
        if (i < nslots - 1 && i % kSlots == 1) atomicMax(acc + i, v);
        else atomicAdd(acc + i, v);
    }
}

}  // namespace

// Every argument checked by the caller; n >= 2 sets, nsizes >= 1. method:
// SORTED or BITSET, resolved by the caller. rows: nsizes entries with size
// and dwarves set by the caller; the rest written here.
void width_sweep(gdist_ctx* ctx, gdist_sets* sets, const gdist_sets* sk, int nsizes, const int32_t* sizes,
                 int method, unsigned flags, gdist_width_row* rows, int64_t* pairs) {
    hipStream_t st = ctx->stream;
    const int64_t n = sets->nsets;
    const int jaccard = (flags & GDIST_SKETCH_JACCARD) ? 1 : 0;
    SelfSource src(ctx, sets, method, GDIST_UPPER_TRIANGLE);
    int64_t R, W;
    closest_blocks(ctx, n, n, src.elem(), &R, &W);
    Walk walk(ctx, src, R, W);

    const size_t nslots = (size_t)kSlots * nsizes + 1;
    DevBuf acc(nslots * 8, st), dsz((size_t)nsizes * 4, st);
    GD_HIP(hipMemsetAsync(acc.p, 0, nslots * 8, st));
    h2d(dsz.p, sizes, (size_t)nsizes * 4, st);

    // no signature is longer than the width (uploads are validated, built
    // sketches are cut), so a run of `run` columns fits run sw dwords as it lies
    const int sw = std::max(1, sk->width);
    const size_t fixed = fixed_bytes(nsizes);
    const int64_t fit = ((int64_t)kLdsBytes - (int64_t)fixed) / 4 / sw - kQT;
    const bool lds = fit >= kMinRun;
    const int run = (int)(lds ? std::min<int64_t>(fit, kMaxRun) : kMinRun);
    const size_t bytes = fixed + (lds ? (size_t)(run + kQT) * sw * 4 : 0);
    const auto kernel = lds ? width_sweep_kernel<true> : width_sweep_kernel<false>;

    walk.run(0, n, 0, n, false, [&](const WalkStep& t) {
        // enough workgroups for four a CU: the rows in slabs of whole tiles
        const int64_t gx = ceil_div(t.nk, run);
        const int64_t want = ceil_div((int64_t)4 * std::max(ctx->cus, 1), gx);
        const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(want, ceil_div(t.nb, kQT)));
        const int64_t rs = ceil_div(ceil_div(t.nb, gy), kQT) * kQT;
        kernel<<<dim3((unsigned)gx, (unsigned)ceil_div(t.nb, rs)), kNT, bytes, st>>>(
            walk.blk.as<int32_t>(), sets->off.as<int64_t>(), sk->codes.as<int32_t>(), sk->off.as<int64_t>(), sw, run,
            rs, t.b0, t.nb, t.k0, t.nk, jaccard, dsz.as<int32_t>(), nsizes, acc.as<unsigned long long>());
        GD_HIP(hipGetLastError());
    }, [](const WalkStep&) {});

    std::vector<unsigned long long> h(nslots, 0ull);
    d2h(h.data(), acc.p, nslots * 8, st);
    *pairs = (int64_t)h[nslots - 1];
    for (int k = 0; k < nsizes; k++) {
        const unsigned long long* a = h.data() + (size_t)kSlots * k;
        gdist_width_row& o = rows[k];
        o.differing = (int64_t)a[0];
        std::memcpy(&o.max_err, &a[1], 8);
        // the digits joined: low + high * 2^32, 128 bits
        const unsigned __int128 sum = (unsigned __int128)a[2] + ((unsigned __int128)a[3] << 32);
        o.sum[0] = (uint64_t)sum;
        o.sum[1] = (uint64_t)(sum >> 64);
        // one rounding (to nearest, ties to even), then an exact scale
        o.total = std::ldexp((double)sum, -62);
        o.mean = *pairs ? o.total / (double)*pairs : 0.0;
    }
}

}  // namespace gdist
