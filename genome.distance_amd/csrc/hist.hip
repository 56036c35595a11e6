// hist.hip — distribution of the distances over caller-supplied bucket edges
// on the device (gdist_histogram): the bucket report TaxCheckProcessor.java:93
// sets up and TaxCheckProcessor.java:133-135 feeds, without the distance table
// leaving HBM.
//
// The driver walks row blocks x column chunks as group_stats() does; per step
// the matrix kernels leave the block's intersection counts I (kmer sets) or
// distances D (sketches) in device memory and hist_kernel counts them into
// the call's accumulators. Pairs are split into series as gdist_group_stats
// splits them (GroupTypeSpec.java:77-95): a label < 0 on either side is a bad
// pair and nothing else; equal labels are the in-group series, others the
// out-group series. Without labels every pair is in one series.
//
// Exactness. A pair's bucket is the number of edges <= d, found by fp64
// comparisons against the edges alone: no index is computed by arithmetic on
// d, so adjacent-double and denormal edges bucket as numpy.searchsorted(edges,
// d, "right") does. Everything accumulated is an integer count, so the result
// does not depend on the order of the pairs, the block sizes or the method,
// and no floating-point atomic appears anywhere in the path.
//
// Contention. Distances are concentrated (d == 1.0 is often most pairs), so
// many lanes of a wave add to one LDS counter. Measured, that is not what the
// kernel waits on: a per-lane run in registers (bucket, its two edges, count;
// LDS touched only when the bucket changes) and a wave-aggregated add both
// lost to the plain atomicAdd per pair below on every collection but one
// whose pairs all fall into a single bucket, where the run wins by skipping
// the edge search, not the atomic ("Distance distribution",
// has every number).
//
// Accumulators (device, zeroed per call), per grouping 2 (E + 1) + 3 uint64
// slots: the in series' E + 1 buckets, the out series', the two NaN counts,
// the bad count. A workgroup adds its non-zero 32-bit LDS counters to them.
#include <algorithm>

#include "gdist_internal.hpp"

namespace gdist {
namespace {

constexpr int kSegCols = 4096;                   // columns of a work item: 64 a lane
constexpr int64_t kMaxItemsPerWave = 1 << 14;    // as group.hip: x 4096 pairs = 2^26 pairs a wave and launch
constexpr int kBatch = 4;                        // columns a lane loads before it counts them
constexpr int kMaxBuckets = GDIST_HIST_MAX_EDGES + 1;
constexpr int kMaxSlots = 2 * kMaxBuckets + 3;

// Rows [q0, q0 + nrows) against the chunk's columns [c0, c0 + nc), grouping
// blockIdx.y (labels == nullptr: one series of every pair). A work item is
// (row, segment of kSegCols columns); wave w of the launch takes the items
// w, w + waves, ...
//  The row's size and label come from roff / rlabels ([.][nrsets]), the
//  column's from coff / clabels ([.][ncsets]): one collection passes the same
//  pointers twice, the cross calls (cross.hip) the queries' and the subjects'.
//  FromCounts: src is I (int32, row a / column b at src[a * ld + b]) and d is
//  the Java expression of epilogue_kernel (matrix_step.hip), closest_select_kernel
//  and group_reduce_kernel, fp64, no contraction; else src is D (double).
template <bool FromCounts>
__global__ __launch_bounds__(256) void hist_kernel(
    const void* __restrict__ src, int64_t ld, const int64_t* __restrict__ roff, const int64_t* __restrict__ coff,
    int empty_nan, int64_t q0, int64_t nrows, int64_t c0, int64_t nc, int upper,
    const int32_t* __restrict__ rlabels, int64_t nrsets, const int32_t* __restrict__ clabels, int64_t ncsets,
    int64_t nitems, int64_t nseg, const double* __restrict__ edges, int E, unsigned long long* __restrict__ acc) {
#pragma clang fp contract(off)
    __shared__ double edge[GDIST_HIST_MAX_EDGES];
    __shared__ uint32_t cnt[kMaxSlots];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int type = blockIdx.y;
    const int nb = E + 1, nslots = 2 * nb + 3;
    const int32_t* rlab = rlabels ? rlabels + (int64_t)type * nrsets : nullptr;
    const int32_t* clab = clabels ? clabels + (int64_t)type * ncsets : nullptr;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int i = threadIdx.x; i < E; i += 256) edge[i] = edges[i];
    for (int i = threadIdx.x; i < nslots; i += 256) cnt[i] = 0;
    __syncthreads();

    // Overflow bound: the host launches enough waves that a wave takes at
    // most kMaxItemsPerWave = 2^14 items, an item is at most 4096 pairs (64 a
    // lane): a lane's NaN / bad counts stay below 2^20, and the four waves of
    // a workgroup add at most 2^28 pairs to its 32-bit LDS counters.
    uint32_t nans0 = 0, nans1 = 0, bad = 0;
    for (int64_t it = (int64_t)blockIdx.x * 4 + wave; it < nitems; it += nwaves) {
        const int64_t a = it / nseg, b0 = (it - a * nseg) * kSegCols;
        const int64_t bend = min(nc, b0 + (int64_t)kSegCols);
        const int64_t q = q0 + a;
        if (upper && c0 + bend - 1 <= q) continue;   // wholly on or left of the diagonal (wave-uniform)
        const int32_t la = rlab ? rlab[q] : 0;
        int64_t na = 0;
        if (FromCounts) na = roff[q + 1] - roff[q];
        const int32_t* Ir = static_cast<const int32_t*>(src) + a * ld;
        const double* Dr = static_cast<const double*>(src) + a * ld;
        for (int64_t bb = b0 + lane; bb < bend; bb += 64 * kBatch) {
            // the loads of kBatch columns a lane first: the walk waits on
            // memory, not on arithmetic, and what follows branches per pair
            bool ok[kBatch];
            int32_t lbv[kBatch], iv[kBatch];
            int64_t nbv[kBatch];
            double dv[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; u++) {
                const int64_t b = bb + 64 * u, j = c0 + b;
                ok[u] = b < bend && !(upper && j <= q);
                lbv[u] = iv[u] = 0;
                nbv[u] = 0;
                dv[u] = 0.0;
                if (ok[u]) {
                    lbv[u] = clab ? clab[j] : 0;
                    if (FromCounts) {
                        iv[u] = Ir[b];
                        nbv[u] = coff[j + 1] - coff[j];
                    } else {
                        dv[u] = Dr[b];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kBatch; u++) {
                if (!ok[u]) continue;
                const int32_t lb = lbv[u];
                if ((la | lb) < 0) {
                    bad++;
                    continue;
                }
                double d;
                if (FromCounts) {
                    const int64_t inter = iv[u];
                    if (inter > 0) {
                        const double uni = (double)(na + nbv[u] - inter);
                        d = 1.0 - (double)inter / uni;
                    } else {
                        d = (empty_nan && na + nbv[u] == 0) ? __builtin_nan("") : 1.0;
                    }
                } else {
                    d = dv[u];
                }
                const bool out = la != lb;
                if (d != d) {
                    nans0 += out ? 0u : 1u;
                    nans1 += out ? 1u : 0u;
                    continue;
                }
                // the number of edges <= d, by comparisons only: 10 halving
                // steps cover E <= 1023 (pos + step - 1 <= 1022)
                int pos = 0;
#pragma unroll
                for (int step = 512; step > 0; step >>= 1) {
                    const int k = pos + step;
                    if (k <= E && edge[k - 1] <= d) pos = k;
                }
                atomicAdd(&cnt[(out ? nb : 0) + pos], 1u);
            }
        }
    }
    if (nans0) atomicAdd(&cnt[2 * nb], nans0);
    if (nans1) atomicAdd(&cnt[2 * nb + 1], nans1);
    if (bad) atomicAdd(&cnt[2 * nb + 2], bad);
    __syncthreads();
    // most buckets are empty in any one step: only the non-zero counters go
    // to the 64-bit accumulators (integer adds: any order gives the same sums)
    unsigned long long* g = acc + (size_t)type * nslots;
    for (int i = threadIdx.x; i < nslots; i += 256) {
        const uint32_t v = cnt[i];
        if (v) atomicAdd(g + i, (unsigned long long)v);
    }
}

// enough waves for ~4 a SIMD, and never more than kMaxItemsPerWave items a
// wave (the kernel's overflow bound)
dim3 hist_grid(const gdist_ctx* ctx, int64_t nrows, int64_t nc, int passes) {
    const int64_t nitems = nrows * ceil_div(nc, kSegCols);
    const int64_t waves =
        std::max(std::min<int64_t>(nitems, (int64_t)ctx->cus * 16), ceil_div(nitems, kMaxItemsPerWave));
    return dim3((unsigned)ceil_div(waves, 4), (unsigned)passes);
}

}  // namespace

static void hist_finish(const unsigned long long* h, int nedges, int ntypes, int64_t* counts, int64_t* nans,
                        int64_t* bad) {
    // series 2 t / 2 t + 1 of grouping t; without labels the one series is
    // the in side of the single pass (every label reads as 0)
    const int nb = nedges + 1, passes = std::max(1, ntypes);
    const size_t tslots = (size_t)2 * nb + 3;
    const int sides = ntypes ? 2 : 1;
    for (int t = 0; t < passes; t++) {
        const unsigned long long* g = h + (size_t)t * tslots;
        for (int k = 0; k < sides; k++) {
            int64_t* row = counts + (size_t)(sides * t + k) * nb;
            for (int b = 0; b < nb; b++) row[b] = (int64_t)g[(size_t)k * nb + b];
            nans[sides * t + k] = (int64_t)g[2 * nb + k];
        }
        if (ntypes) bad[t] = (int64_t)g[2 * nb + 2];
    }
}

// Any order of the steps: the counts do not depend on it.
void hist_count(gdist_ctx* ctx, WalkSource& src, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int nedges,
                const double* edges, int ntypes, const int32_t* rlabels, const int32_t* clabels, int64_t* counts,
                int64_t* nans, int64_t* bad) {
    hipStream_t st = ctx->stream;
    const int passes = std::max(1, ntypes);
    const size_t nslots = (size_t)passes * ((size_t)2 * (nedges + 1) + 3);
    std::vector<unsigned long long> h(nslots, 0ull);
    if (r1 > r0 && c1 > c0) {
        int64_t R, W;
        closest_blocks(ctx, r1 - r0, c1 - c0, src.elem(), &R, &W);
        Walk walk(ctx, src, R, W);
        const WalkLabels lab(src, ntypes, rlabels, clabels, st);   // no labels: null, every pair in one series
        DevBuf edg((size_t)nedges * 8, st), acc(nslots * 8, st);
        h2d(edg.p, edges, (size_t)nedges * 8, st);
        GD_HIP(hipMemsetAsync(acc.p, 0, nslots * 8, st));
        const auto kernel = src.from_counts ? hist_kernel<true> : hist_kernel<false>;
        walk.run(r0, r1, c0, c1, false, [&](const WalkStep& t) {
            const int64_t nseg = ceil_div(t.nk, kSegCols);
            kernel<<<hist_grid(ctx, t.nb, t.nk, passes), 256, 0, st>>>(
                walk.blk.p, t.nk, src.roff, src.coff, src.empty_nan, t.b0, t.nb, t.k0, t.nk, src.upper, lab.rows,
                src.nrsets, lab.cols, src.ncsets, t.nb * nseg, nseg, edg.as<double>(), nedges,
                acc.as<unsigned long long>());
            GD_HIP(hipGetLastError());
        }, [](const WalkStep&) {});
        d2h(h.data(), acc.p, nslots * 8, st);
    }
    hist_finish(h.data(), nedges, ntypes, counts, nans, bad);
}

void histogram(gdist_ctx* ctx, gdist_sets* s, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int method,
               unsigned flags, int nedges, const double* edges, int ntypes, const int32_t* labels, int64_t* counts,
               int64_t* nans, int64_t* bad) {
    SelfSource src(ctx, s, method, flags);
    ctx->hist_matrix_ms = ctx->hist_reduce_ms = -1.0;
    hist_count(ctx, src, r0, r1, c0, c1, nedges, edges, ntypes, labels, labels, counts, nans, bad);
    if (src.timed) {
        ctx->hist_matrix_ms = src.fill_ms;
        ctx->hist_reduce_ms = src.consume_ms;
    }
}

}  // namespace gdist
