// pairs.hip — the distances of an arbitrary (id1, id2) pair list in one call.
//
// getDistance over a pair list (MethodTableProcessor.java:258-276; the lists
// of BasicPairsProcessor.java:71-89 and PairCreateProcessor.java:29-32): P
// intersections, one upload, one download. The rectangle kernels do not fit:
// a list of many first genomes with a handful of partners each fills no tile.
//
// Plan (PairList, pair_list.hip: one upload, no host round trip): the pair
// positions sorted by row and cut into chunks of at most kPairUnit pairs of
// one row. Sorted path: a chunk whose codes (|A_i| plus its columns' sets)
// exceed the call's budget (pair_list.hpp) is cut into several ranges of the
// segment index (sorted.hip build_segments), the units. A unit adds its counts
// into a zeroed I with atomicAdd (integers: exact, order-free), so a few pairs
// of huge sets still fill the chip. The join kernel reads the number of units
// from device memory and strides over them. Bitset path: no units, the sorted
// positions.
//
// Sorted path (pairs_sorted_kernel): as sorted_join_kernel, a workgroup stages
// A_i's codes of the unit's next segments in LDS and its waves stream the same
// segments of each listed column (coalesced), but A's sorted run is staged as
// it is (as many whole segments as fit STAGE keys) and probed by a branch-free
// search for the last key <= v: nothing to clear or build per segment, which
// is what a unit of one or four columns cannot amortise. Keys are compared for
// equality only, so the all-ones code (the hash join's EMPTY marker) is a key
// like any other. A unit with fewer than 8 columns splits each column's run
// over its 8 waves.
//
// Bitset path (pairs_bitset_kernel): one wave per pair in row order. Dense
// tier: popc(bits[i] & bits[j]) over the W words (bits is kept whole). Rare
// tier: each record of the set with fewer records is searched for the other
// set in its posting list (ascending), a hit adds the record's weight.
// Variant tier (and the grouped rare tier in the same arrays): each entry of
// the set with fewer entries is searched for the other set in its word list
// (ascending), a hit adds popc(mask & mask). The three sums are what
// bitset_matrix counts; a self pair is |A_i| (the epilogue).
#include "gdist_internal.hpp"
#include "pair_list.hpp"
#include "sketch_wave_merge.hpp"

namespace gdist {
namespace {

constexpr int NTP = 512;                    // threads of a join workgroup (8 waves)
constexpr int STAGE = 4096;                 // keys of A staged at a time (32 KiB)

__global__ __launch_bounds__(NTP) void pairs_sorted_kernel(
    const uint64_t* __restrict__ codes, const int64_t* __restrict__ segoff, int nseg,
    const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, const int64_t* __restrict__ cols,
    const int4* __restrict__ units, const unsigned long long* __restrict__ counts, int32_t* __restrict__ I) {
    __shared__ unsigned long long sa[STAGE];
    __shared__ int32_t cnt[kPairUnit];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nunits = (int64_t)counts[1];
    const int64_t per = nseg + 1;
    for (int64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const int4 un = units[u];
        const int64_t k0 = un.x;
        const int ncol = un.y;
        const int64_t i = (int64_t)keys[k0];
        const int64_t* arow = segoff + i * per;
        if (tid < kPairUnit) cnt[tid] = 0;
        __syncthreads();
        // a unit of few columns: each column's run in S slices, a wave a slice
        const int S = ncol >= NTP / 64 ? 1 : (NTP / 64) / ncol;
        for (int p = un.z; p < un.w;) {
            const int64_t a0 = arow[p];
            int pe = p + 1;
            while (pe < un.w && arow[pe + 1] - a0 <= STAGE) pe++;
            const int64_t a1 = arow[pe];
            // more than one pass only for a single segment longer than STAGE
            // (exact: A's sub-runs are disjoint)
            for (int64_t sb = a0; sb < a1; sb += STAGE) {
                const int n = (int)(a1 - sb < STAGE ? a1 - sb : STAGE);
                for (int t = tid; t < n; t += NTP) sa[t] = codes[sb + t];
                __syncthreads();
                const uint64_t amin = sa[0], amax = sa[n - 1];
                for (int it = wave; it < ncol * S; it += NTP / 64) {
                    const int t = it % ncol, sl = it / ncol;
                    const int64_t j = cols[vals[k0 + t]];
                    const int64_t* brow = segoff + j * per;
                    const int64_t b0 = brow[p], blen = brow[pe] - b0;
                    const int64_t lo = b0 + blen * sl / S, hi = b0 + blen * (sl + 1) / S;
                    int c = 0;
                    for (int64_t e = lo + lane; e < hi; e += 64) {
                        const uint64_t v = codes[e];
                        if (v < amin || v > amax) continue;
                        int base = 0, len = n;   // the last key <= v is in [base, base + len)
                        while (len > 1) {
                            const int half = len >> 1;
                            base = sa[base + half] <= v ? base + half : base;
                            len -= half;
                        }
                        c += sa[base] == v;
                    }
                    c = skx_wave_sum(c);
                    if (lane == 0 && c) atomicAdd(&cnt[t], c);
                }
                __syncthreads();
            }
            p = pe;
        }
        if (tid < ncol) {
            const int c = cnt[tid];
            if (c) atomicAdd(I + vals[k0 + tid], c);
        }
        __syncthreads();
    }
}

// first position of [b, e) holding a value >= t (e when none)
__device__ __forceinline__ int64_t lower_u32(const uint32_t* __restrict__ a, int64_t b, int64_t e, uint32_t t) {
    while (b < e) {
        const int64_t mid = (b + e) >> 1;
        if (a[mid] < t) b = mid + 1; else e = mid;
    }
    return b;
}

__global__ __launch_bounds__(256) void pairs_bitset_kernel(
    const unsigned long long* __restrict__ bits, int64_t W, const int64_t* __restrict__ roff,
    const uint64_t* __restrict__ rent, const uint32_t* __restrict__ rw, const uint32_t* __restrict__ psets,
    const int64_t* __restrict__ voff, const uint32_t* __restrict__ vent, const uint32_t* __restrict__ vset,
    const unsigned long long* __restrict__ vmask, const uint32_t* __restrict__ vbeg,
    const uint32_t* __restrict__ vend, const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals,
    const int64_t* __restrict__ cols, int64_t n, int32_t* __restrict__ I) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t k = wave; k < n; k += waves) {
        const int32_t p = vals[k];
        const int64_t i = (int64_t)keys[k], j = cols[p];
        if (i == j) continue;               // the epilogue takes |A_i|
        int acc = 0;
        const unsigned long long* a = bits + i * W;
        const unsigned long long* b = bits + j * W;
        for (int64_t w = lane; w < W; w += 64) acc += __popcll(a[w] & b[w]);
        if (roff) {
            const bool sw = roff[j + 1] - roff[j] < roff[i + 1] - roff[i];
            const int64_t x = sw ? j : i;
            const uint32_t y = (uint32_t)(sw ? i : j);
            for (int64_t r = roff[x] + lane; r < roff[x + 1]; r += 64) {
                const uint64_t ent = rent[r];
                const int64_t lb = (int64_t)(ent >> 24), le = lb + (int64_t)(ent & 0xFFFFFFu);
                const int64_t f = lower_u32(psets, lb, le, y);
                if (f < le && psets[f] == y) acc += (int)rw[r];
            }
        }
        if (voff) {
            const bool sw = voff[j + 1] - voff[j] < voff[i + 1] - voff[i];
            const int64_t x = sw ? j : i;
            const uint32_t y = (uint32_t)(sw ? i : j);
            for (int64_t r = voff[x] + lane; r < voff[x + 1]; r += 64) {
                const uint32_t e = vent[r];
                const unsigned long long m = vmask[e];
                const int64_t le = (int64_t)vend[e];
                for (int64_t f = lower_u32(vset, (int64_t)vbeg[e], le, y); f < le && vset[f] == y; f++)
                    acc += __popcll(m & vmask[f]);
            }
        }
        acc = skx_wave_sum(acc);
        if (lane == 0) I[p] = acc;
    }
}

// I of a self pair and D: the expression of row_epilogue_kernel
__global__ void pairs_epilogue_kernel(const int64_t* __restrict__ off, const int64_t* __restrict__ rows,
                                      const int64_t* __restrict__ cols, int64_t n, int empty_nan,
                                      int32_t* __restrict__ I, double* __restrict__ D) {
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t i = rows[p], j = cols[p];
    const int64_t na = off[i + 1] - off[i], nb = off[j + 1] - off[j];
    const int64_t inter = (j == i) ? na : I[p];
    if (j == i) I[p] = (int32_t)na;
    if (!D) return;
    double d;
    if (inter > 0) {
        const double uni = (double)(na + nb - inter);
        d = 1.0 - (double)inter / uni;
    } else {
        d = (empty_nan && na + nb == 0) ? __builtin_nan("") : 1.0;
    }
    D[p] = d;
}

}  // namespace

// method: SORTED or BITSET (resolved by the caller, which checked every
// argument); I_out / D_out: host, either may be null
void pairs(gdist_ctx* ctx, const gdist_sets* s, int method, unsigned flags, int64_t n, const int64_t* rows,
           const int64_t* cols, int32_t* I_out, double* D_out) {
    hipStream_t st = ctx->stream;
    PairList pl(ctx, s->nsets, n, rows, cols, I_out, D_out, true);   // the join adds into I, the epilogue reads it
    if (method == GDIST_METHOD_SORTED) {
        double codes = 0;
        for (int64_t p = 0; p < n; p++)
            codes += (double)(s->h_off[rows[p] + 1] - s->h_off[rows[p]] + s->h_off[cols[p] + 1] - s->h_off[cols[p]]);
        pl.plan_segment_units(s, s, codes);
        const unsigned grid = (unsigned)std::min<int64_t>(pl.ucap, (int64_t)ctx->cus * 8);
        pairs_sorted_kernel<<<grid, NTP, 0, st>>>(s->codes.as<uint64_t>(), s->segoff.as<int64_t>(), s->nseg, pl.keys,
                                                  pl.vals, pl.cols, pl.units.as<int4>(), pl.counts, pl.I);
    } else {
        pl.plan_groups();
        const bool rare = s->n_rare > 0;
        const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n, 4), (int64_t)ctx->cus * 16);
        pairs_bitset_kernel<<<grid, 256, 0, st>>>(
            s->bits.as<unsigned long long>(), s->W, rare ? s->srare_off.as<int64_t>() : nullptr,
            s->srare_ent.as<uint64_t>(), s->srare_w.as<uint32_t>(), s->post_sets.as<uint32_t>(),
            s->variant ? s->vs_off.as<int64_t>() : nullptr, s->vs_ent.as<uint32_t>(), s->vw_set.as<uint32_t>(),
            s->vw_mask.as<unsigned long long>(), s->vw_beg.as<uint32_t>(), s->vw_end.as<uint32_t>(), pl.keys, pl.vals,
            pl.cols, n, pl.I);
    }
    GD_HIP(hipGetLastError());
    pairs_epilogue_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(s->off.as<int64_t>(), pl.rows, pl.cols, n,
                                                                      (flags & GDIST_EMPTY_NAN) ? 1 : 0, pl.I, pl.D);
    GD_HIP(hipGetLastError());
    pl.finish();
}

}  // namespace gdist
