// group.hip — in-group / out-group distance summary on the device
// (gdist_group_stats): the distCheck report of DistanceCheckProcessor.java:149-223
// without the distance table leaving HBM.
//
// The driver walks row blocks x column chunks as closest() does; per step the
// matrix kernels leave the block's intersection counts I (kmer sets) or
// distances D (sketches) in device memory and group_reduce_kernel folds them
// into the call's accumulators. Pairs are classified per grouping as
// GroupTypeSpec.java:77-95 classifies them: a label < 0 on either side is a
// bad pair; equal labels are in-group, others out-group; within a side
// d == 1.0 is counted in `ones`, NaN in `nans`, any other d is summarised.
//
// Exactness. Every summarised d has the form 1.0 - (double)a / (double)b with
// 0 < a <= b and is therefore an integer multiple of 2^-53 in [0, 1)
// (DESIGN.md §4): m = d * 2^53 is an integer <= 2^53. The kernel accumulates
// n, sum m and sum m^2 in integer arithmetic only, so the result does not
// depend on the order of the pairs, the block sizes or the method, and no
// floating-point atomic appears anywhere in the path.
//
// Registers. One pass over the block per grouping (grid.y = grouping): a lane
// holds the in and out accumulators of one grouping only (2 x {n, ones, nans,
// 96-bit sum, 128-bit sum of squares, min, max} and the bad count), not 8 x 2
// of them. I is 4 bytes a pair and the re-reads hit the cache.
//
// Accumulators (device, zeroed per call), per grouping kTypeSlots uint64
// slots: per side {n, ones, nans, 4 digits of sum m, 6 digits of sum m^2,
// max of ~bits(d) (the minimum), max of bits(d)}, then the bad count. A
// workgroup adds its partial as 32-bit digits, each into its own 64-bit slot
// (carry-save): a slot overflows only past 2^32 workgroup flushes. The host
// propagates the carries (group_stats_host.hpp).
#include <algorithm>
#include <cstring>

#include "gdist_internal.hpp"
#include "group_stats_host.hpp"

namespace gdist {
namespace {

constexpr int kSideSlots = 15;                   // n, ones, nans, S[4], Q[6], ~min, max
constexpr int kTypeSlots = 2 * kSideSlots + 1;   // in, out, bad
constexpr int kSegCols = 4096;                   // columns of a work item: 64 a lane
constexpr int64_t kMaxItemsPerWave = 1 << 14;    // x 64 pairs a lane = 2^20 pairs a lane and launch

struct LaneSide {
    uint32_t n = 0, ones = 0, nans = 0;
    unsigned long long s0 = 0;       // sum m, bits 0..63
    uint32_t s1 = 0;                 //        bits 64..95
    unsigned long long q0 = 0, q1 = 0;   // sum m^2, 128 bits
    unsigned long long mn = 0;       // max of ~bits(d): 0 = none
    unsigned long long mx = 0;       // max of bits(d)
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// Rows [q0, q0 + nrows) against the chunk's columns [c0, c0 + nc), grouping
// blockIdx.y. A work item is (row, segment of kSegCols columns); wave w of
// the launch takes the items w, w + waves, ...
//  FromCounts: src is I (int32, row a / column b at src[a * ld + b]) and d is
//  the Java expression of epilogue_kernel (matrix_step.hip) and
//  closest_select_kernel, fp64, no contraction; else src is D (double).
//  The row's size and label come from roff / rlabels ([.][nrsets]), the
//  column's from coff / clabels ([.][ncsets]): one collection passes the same
//  pointers twice, the cross calls (cross.hip) the queries' and the subjects'.
template <bool FromCounts>
__global__ __launch_bounds__(256) void group_reduce_kernel(
    const void* __restrict__ src, int64_t ld, const int64_t* __restrict__ roff, const int64_t* __restrict__ coff,
    int empty_nan, int64_t q0, int64_t nrows, int64_t c0, int64_t nc, int upper,
    const int32_t* __restrict__ rlabels, int64_t nrsets, const int32_t* __restrict__ clabels, int64_t ncsets,
    int64_t nitems, int64_t nseg, unsigned long long* __restrict__ acc) {
#pragma clang fp contract(off)
    __shared__ unsigned long long red[4][kTypeSlots];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int type = blockIdx.y;
    const int32_t* rlab = rlabels + (int64_t)type * nrsets;
    const int32_t* clab = clabels + (int64_t)type * ncsets;
    const int64_t nwaves = (int64_t)gridDim.x * 4;

    LaneSide sd[2];
    uint32_t bad = 0;
    // Overflow bound: the host launches enough waves that a wave takes at
    // most kMaxItemsPerWave = 2^14 items, an item is at most 64 pairs a lane:
    // a lane adds at most 2^20 pairs. m <= 2^53 and m^2 <= 2^106, so its
    // sums stay below 2^73 (96 bits held) and 2^126 (128 bits held), and
    // its 32-bit counts below 2^20.
    for (int64_t it = (int64_t)blockIdx.x * 4 + wave; it < nitems; it += nwaves) {
        const int64_t a = it / nseg, b0 = (it - a * nseg) * kSegCols;
        const int64_t bend = min(nc, b0 + (int64_t)kSegCols);
        const int64_t q = q0 + a;
        if (upper && c0 + bend - 1 <= q) continue;   // wholly on or left of the diagonal (wave-uniform)
        const int32_t la = rlab[q];
        int64_t na = 0;
        if (FromCounts) na = roff[q + 1] - roff[q];
        const int32_t* Ir = static_cast<const int32_t*>(src) + a * ld;
        const double* Dr = static_cast<const double*>(src) + a * ld;
        for (int64_t b = b0 + lane; b < bend; b += 64) {
            const int64_t j = c0 + b;
            if (upper && j <= q) continue;
            const int32_t lb = clab[j];
            if ((la | lb) < 0) {
                bad++;
                continue;
            }
            double d;
            if (FromCounts) {
                const int64_t inter = Ir[b];
                const int64_t nb = coff[j + 1] - coff[j];
                if (inter > 0) {
                    const double uni = (double)(na + nb - inter);
                    d = 1.0 - (double)inter / uni;
                } else {
                    d = (empty_nan && na + nb == 0) ? __builtin_nan("") : 1.0;
                }
            } else {
                d = Dr[b];
            }
            const bool isnan = d != d, one = d == 1.0, num = !isnan && !one;
            // exact: a scale by a power of two, then an integer <= 2^53
            const unsigned long long m = num ? (unsigned long long)(d * 9007199254740992.0) : 0ull;
            const unsigned long long db = (unsigned long long)__double_as_longlong(d);
            const unsigned long long m2lo = m * m, m2hi = __umul64hi(m, m);   // 64 x 64 -> 128
            const bool same = la == lb;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const bool sel = same == (k == 0);
                LaneSide& s = sd[k];
                s.ones += (sel && one) ? 1u : 0u;
                s.nans += (sel && isnan) ? 1u : 0u;
                const bool add = sel && num;
                s.n += add ? 1u : 0u;
                const unsigned long long mm = add ? m : 0ull;
                s.s0 += mm;
                s.s1 += s.s0 < mm ? 1u : 0u;
                const unsigned long long lo = add ? m2lo : 0ull, hi = add ? m2hi : 0ull;
                s.q0 += lo;
                s.q1 += hi + (s.q0 < lo ? 1ull : 0ull);
                if (add) {
                    s.mn = ~db > s.mn ? ~db : s.mn;   // d >= 0 and not NaN: the unsigned pattern orders it
                    s.mx = db > s.mx ? db : s.mx;
                }
            }
        }
    }

    // wave reduction of the 32-bit digits (64 lanes x 2^32 < 2^38: no carry is lost)
    unsigned long long v[kTypeSlots];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const LaneSide& s = sd[k];
        unsigned long long* w = v + k * kSideSlots;
        w[0] = s.n;
        w[1] = s.ones;
        w[2] = s.nans;
        w[3] = s.s0 & 0xffffffffull;
        w[4] = s.s0 >> 32;
        w[5] = s.s1;
        w[6] = 0;
        w[7] = s.q0 & 0xffffffffull;
        w[8] = s.q0 >> 32;
        w[9] = s.q1 & 0xffffffffull;
        w[10] = s.q1 >> 32;
        w[11] = 0;
        w[12] = 0;
        w[13] = s.mn;
        w[14] = s.mx;
    }
    v[2 * kSideSlots] = bad;
#pragma unroll
    for (int i = 0; i < kTypeSlots; i++) {
        const int f = i < 2 * kSideSlots ? i % kSideSlots : 0;
        if (f == 6 || f == 11 || f == 12) continue;   // digits only carries reach
        v[i] = f >= 13 ? wave_max(v[i]) : wave_sum(v[i]);
        if (lane == 0) red[wave][i] = v[i];
    }
    __syncthreads();
    // one thread a side: the four waves' digit sums, carries propagated so
    // that every global add is below 2^32, then the atomics
    unsigned long long* g = acc + (size_t)type * kTypeSlots;
    if (threadIdx.x < 2) {
        const int base = threadIdx.x * kSideSlots;
        for (int f = 0; f < 3; f++) {
            const unsigned long long t = red[0][base + f] + red[1][base + f] + red[2][base + f] + red[3][base + f];
            if (t) atomicAdd(g + base + f, t);
        }
        unsigned long long carry = 0;
        for (int f = 3; f < 7; f++) {   // sum m: digits 0..2 held, digit 3 from the carry
            unsigned long long t = carry;
            if (f < 6) t += red[0][base + f] + red[1][base + f] + red[2][base + f] + red[3][base + f];
            if (t & 0xffffffffull) atomicAdd(g + base + f, t & 0xffffffffull);
            carry = t >> 32;
        }
        carry = 0;
        for (int f = 7; f < 13; f++) {  // sum m^2: digits 0..3 held, 4..5 from the carries
            unsigned long long t = carry;
            if (f < 11) t += red[0][base + f] + red[1][base + f] + red[2][base + f] + red[3][base + f];
            if (t & 0xffffffffull) atomicAdd(g + base + f, t & 0xffffffffull);
            carry = t >> 32;
        }
        for (int f = 13; f < 15; f++) {
            unsigned long long t = red[0][base + f];
            for (int w = 1; w < 4; w++) t = red[w][base + f] > t ? red[w][base + f] : t;
            if (t) atomicMax(g + base + f, t);
        }
    } else if (threadIdx.x == 2) {
        const int f = 2 * kSideSlots;
        const unsigned long long t = red[0][f] + red[1][f] + red[2][f] + red[3][f];
        if (t) atomicAdd(g + f, t);
    }
}

// enough waves for ~4 a SIMD, and never more than kMaxItemsPerWave items a
// wave (the kernel's overflow bound)
dim3 group_grid(const gdist_ctx* ctx, int64_t nrows, int64_t nc, int ntypes) {
    const int64_t nitems = nrows * ceil_div(nc, kSegCols);
    const int64_t waves =
        std::max(std::min<int64_t>(nitems, (int64_t)ctx->cus * 16), ceil_div(nitems, kMaxItemsPerWave));
    return dim3((unsigned)ceil_div(waves, 4), (unsigned)ntypes);
}

}  // namespace

// carries of the digit slots, min / max from their patterns, mean and sdev
static void group_finish(const unsigned long long* h, int ntypes, gdist_group_side* out, int64_t* bad) {
    for (int t = 0; t < ntypes; t++) {
        const unsigned long long* g = h + (size_t)t * kTypeSlots;
        for (int k = 0; k < 2; k++) {
            const unsigned long long* w = g + k * kSideSlots;
            gdist_group_side o;
            std::memset(&o, 0, sizeof(o));
            o.n = (int64_t)w[0];
            o.ones = (int64_t)w[1];
            o.nans = (int64_t)w[2];
            gstats::U256 S, Q;
            for (int d = 0; d < 4; d++) gstats::add_digit(S, w[3 + d], d);
            for (int d = 0; d < 6; d++) gstats::add_digit(Q, w[7 + d], d);
            if (S.w[2] | S.w[3] | Q.w[3]) throw Error(GDIST_EDEVICE, "group statistics: a sum exceeds its limbs");
            o.sum[0] = S.w[0];
            o.sum[1] = S.w[1];
            for (int i = 0; i < 3; i++) o.sumsq[i] = Q.w[i];
            const unsigned long long mn = ~w[13], mx = w[14];
            std::memcpy(&o.min, &mn, 8);
            std::memcpy(&o.max, &mx, 8);
            gstats::finish(&o);
            out[2 * t + k] = o;
        }
        bad[t] = (int64_t)g[2 * kSideSlots];
    }
}

// Any order of the steps: the sums do not depend on it.
void group_reduce(gdist_ctx* ctx, WalkSource& src, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int ntypes,
                  const int32_t* rlabels, const int32_t* clabels, gdist_group_side* out, int64_t* bad) {
    hipStream_t st = ctx->stream;
    const size_t nslots = (size_t)ntypes * kTypeSlots;
    std::vector<unsigned long long> h(nslots, 0ull);
    if (r1 > r0 && c1 > c0) {
        int64_t R, W;
        closest_blocks(ctx, r1 - r0, c1 - c0, src.elem(), &R, &W);
        Walk walk(ctx, src, R, W);
        const WalkLabels lab(src, ntypes, rlabels, clabels, st);
        DevBuf acc(nslots * 8, st);
        GD_HIP(hipMemsetAsync(acc.p, 0, nslots * 8, st));
        const auto kernel = src.from_counts ? group_reduce_kernel<true> : group_reduce_kernel<false>;
        walk.run(r0, r1, c0, c1, false, [&](const WalkStep& t) {
            const int64_t nseg = ceil_div(t.nk, kSegCols);
            kernel<<<group_grid(ctx, t.nb, t.nk, ntypes), 256, 0, st>>>(
                walk.blk.p, t.nk, src.roff, src.coff, src.empty_nan, t.b0, t.nb, t.k0, t.nk, src.upper, lab.rows,
                src.nrsets, lab.cols, src.ncsets, t.nb * nseg, nseg, acc.as<unsigned long long>());
            GD_HIP(hipGetLastError());
        }, [](const WalkStep&) {});
        d2h(h.data(), acc.p, nslots * 8, st);
    }
    group_finish(h.data(), ntypes, out, bad);
}

void group_stats(gdist_ctx* ctx, gdist_sets* s, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int method,
                 unsigned flags, int ntypes, const int32_t* labels, gdist_group_side* out, int64_t* bad) {
    SelfSource src(ctx, s, method, flags);
    ctx->group_matrix_ms = ctx->group_reduce_ms = -1.0;
    group_reduce(ctx, src, r0, r1, c0, c1, ntypes, labels, labels, out, bad);
    if (src.timed) {
        ctx->group_matrix_ms = src.fill_ms;
        ctx->group_reduce_ms = src.consume_ms;
    }
}

}  // namespace gdist
