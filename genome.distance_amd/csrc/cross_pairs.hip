// cross_pairs.hip — a pair list across two collections (gdist_cross_pairs).
//
// getDistance over an (id1, id2) list (MethodTableProcessor.java:258-276; the
// lists of BasicPairsProcessor.java:71-89 and PairCreateProcessor.java:29-32)
// whose first genomes are new and whose second genomes live in the resident
// database: rows index the queries, columns the subjects. The subjects stay as
// they are (their codes and their segment index are read), nothing is kept on
// the queries, and no rectangle is computed for a handful of its cells.
//
// Plan (PairList, pair_list.hip): the pair positions sorted by query row and
// cut into chunks of at most kPairUnit pairs of one row; a chunk whose codes
// (the query's set from the queries' offsets plus its columns' sets from the
// subjects') exceed the call's budget (pair_list.hpp) is cut into several
// ranges of the SUBJECTS' segment index, the units. A unit adds its counts
// into a zeroed I with atomicAdd (integers: exact, order-free).
//
// Kernel (cross_pairs_kernel): pairs_sorted_kernel over two code arrays. The
// staged run is the query's, the streamed runs are the subjects' by their
// segment index. Where the query row is cut is cached nowhere: the workgroup
// finds the cut points of its unit's segment range by binary search of the
// subjects' splitters in the row (cross_cut.hpp) and keeps them in LDS, 32-bit
// relative to the row's start; no [groups][nseg + 1] scratch index exists.
//
// Long query segments. A collection's own splitters keep its segments near
// 2,048 codes; a query is cut by foreign splitters, so a whole query of any
// size may fall into one subject segment. The sub-run walk (a segment longer
// than STAGE in passes of STAGE keys, each streaming the subjects' same
// segment again) is then the common path; it is exact because the query's
// sub-runs are disjoint and each subject code equals at most one query code.
#include "gdist_internal.hpp"
#include "cross_cut.hpp"
#include "pair_list.hpp"
#include "sketch_wave_merge.hpp"

namespace gdist {
namespace {

constexpr int NTP = 512;                    // threads of a join workgroup (8 waves)
constexpr int STAGE = 4096;                 // keys of the query staged at a time (32 KiB)

__global__ __launch_bounds__(NTP) void cross_pairs_kernel(
    const uint64_t* __restrict__ qcodes, const int64_t* __restrict__ qoff, const uint64_t* __restrict__ scodes,
    const int64_t* __restrict__ sseg, const uint64_t* __restrict__ split, int nseg,
    const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, const int64_t* __restrict__ cols,
    const int4* __restrict__ units, const unsigned long long* __restrict__ counts, int32_t* __restrict__ I) {
    __shared__ unsigned long long sa[STAGE];
    __shared__ uint32_t cut[kCrossCutMax];
    __shared__ int32_t cnt[kPairUnit];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nunits = (int64_t)counts[1];
    const int64_t per = nseg + 1;
    for (int64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const int4 un = units[u];
        const int64_t k0 = un.x;
        const int ncol = un.y;
        // defensive: never address outside the cut points
        if (un.z < 0 || un.z >= un.w || un.w > nseg || un.w - un.z >= kCrossCutMax) continue;
        const int64_t i = (int64_t)keys[k0];
        const int64_t qb = qoff[i];
        // the unit's cut points [first, end] of the query row, relative to qb
        xc_cuts(qcodes + qb, qoff[i + 1] - qb, split, nseg, un.z, un.w, cut, tid, NTP);
        if (tid < kPairUnit) cnt[tid] = 0;
        __syncthreads();
        // a unit of few columns: each column's run in S slices, a wave a slice
        const int S = ncol >= NTP / 64 ? 1 : (NTP / 64) / ncol;
        for (int p = un.z; p < un.w;) {
            const uint32_t c0 = cut[p - un.z];
            int pe = p + 1;
            while (pe < un.w && cut[pe + 1 - un.z] - c0 <= (uint32_t)STAGE) pe++;
            const int64_t a0 = qb + c0, a1 = qb + cut[pe - un.z];
            // more than one pass only for a single segment longer than STAGE
            // (exact: the query's sub-runs are disjoint)
            for (int64_t sb = a0; sb < a1; sb += STAGE) {
                const int n = (int)(a1 - sb < STAGE ? a1 - sb : STAGE);
                for (int t = tid; t < n; t += NTP) sa[t] = qcodes[sb + t];
                __syncthreads();
                const uint64_t amin = sa[0], amax = sa[n - 1];
                for (int it = wave; it < ncol * S; it += NTP / 64) {
                    const int t = it % ncol, sl = it / ncol;
                    const int64_t j = cols[vals[k0 + t]];
                    const int64_t* brow = sseg + j * per;
                    const int64_t b0 = brow[p], blen = brow[pe] - b0;
                    const int64_t lo = b0 + blen * sl / S, hi = b0 + blen * (sl + 1) / S;
                    int c = 0;
                    for (int64_t e = lo + lane; e < hi; e += 64) {
                        const uint64_t v = scodes[e];
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

// D from I: the expression of cross_epilogue_kernel, |A| from the queries'
// offsets and |B| from the subjects'; no pair is "self"
__global__ void cross_pairs_epilogue_kernel(const int64_t* __restrict__ qoff, const int64_t* __restrict__ soff,
                                            const int64_t* __restrict__ rows, const int64_t* __restrict__ cols,
                                            int64_t n, int empty_nan, const int32_t* __restrict__ I,
                                            double* __restrict__ D) {
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t i = rows[p], j = cols[p];
    const int64_t inter = I[p];
    const int64_t na = qoff[i + 1] - qoff[i], nb = soff[j + 1] - soff[j];
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

static_assert(kCrossSegMax == 4096, "build_segments makes at most 4,096 segments");

// kmer sets, every argument checked by the caller, n > 0, the subjects'
// segment index built; rows index q, cols index s; I_out / D_out: host, either
// may be null
void cross_pairs(gdist_ctx* ctx, const gdist_sets* q, const gdist_sets* s, unsigned flags, int64_t n,
                 const int64_t* rows, const int64_t* cols, int32_t* I_out, double* D_out) {
    hipStream_t st = ctx->stream;
    double codes = 0;
    for (int64_t p = 0; p < n; p++) {
        const int64_t na = q->h_off[rows[p] + 1] - q->h_off[rows[p]];
        GD_REQUIRE(na < (int64_t(1) << 32), "a query set of 2^32 codes or more");   // the cut points are 32-bit
        codes += (double)(na + s->h_off[cols[p] + 1] - s->h_off[cols[p]]);
    }
    PairList pl(ctx, q->nsets, n, rows, cols, I_out, D_out, true);   // the join adds into I, the epilogue reads it
    pl.plan_segment_units(q, s, codes);
    const unsigned grid = (unsigned)std::min<int64_t>(pl.ucap, (int64_t)ctx->cus * 8);
    cross_pairs_kernel<<<grid, NTP, 0, st>>>(q->codes.as<uint64_t>(), q->off.as<int64_t>(), s->codes.as<uint64_t>(),
                                             s->segoff.as<int64_t>(), s->seg_split.as<uint64_t>(), s->nseg, pl.keys,
                                             pl.vals, pl.cols, pl.units.as<int4>(), pl.counts, pl.I);
    GD_HIP(hipGetLastError());
    if (pl.D) {
        cross_pairs_epilogue_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(
            q->off.as<int64_t>(), s->off.as<int64_t>(), pl.rows, pl.cols, n, (flags & GDIST_EMPTY_NAN) ? 1 : 0, pl.I,
            pl.D);
        GD_HIP(hipGetLastError());
    }
    pl.finish();
}

}  // namespace gdist
