// within.hip — every pair within max_dist as CSR, on the device (gdist_within).
//
// The documented maxDist filter of the genomes table (GenomeProcessor.java:35)
// and the first question of dereplication and neighbour graphs: the pairs
// (i, j) of a rectangle with d(i, j) <= max_dist, all of them, row ascending
// and column ascending within a row, without the distance table leaving HBM.
//
// The driver walks row blocks only: a step is rows [b0, b1) against all of
// the call's columns (with GDIST_UPPER_TRIANGLE from max(c0, b0 + 1) on), so a
// step's survivors are already in output order and the steps arrive in row
// order. Per step the matrix kernels leave the block's intersection counts I
// (kmer sets) or distances D (sketches) in device memory, as in closest(),
// and three small launches compact them:
//   count  one wave a (row, segment of kSegCols columns) tile: the tile's
//          survivors, from __ballot / __popcll
//   scan   exclusive scan of the tile counts in row-major tile order
//          (rocPRIM), and the per-row bases gathered for the host
//   write  the same tiling and the same test; a survivor's position is its
//          tile's base plus its rank among the wave's survivors (mbcnt).
//          Only when some of the step's entries fit the caller's capacity,
//          into a staging buffer sized to the entries that fit.
// No atomic decides a position: the output is the same bytes every run, and
// does not depend on the method or the block size.
#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "gdist_internal.hpp"

namespace gdist {
namespace {

// out[i] = in[0] + .. + in[i - 1] for i < n, as int64; tmp grows to what
// rocPRIM asks for and is kept between the steps of a call (no allocation, so
// no host wait, between a step's launches after the first)
void scan_counts(hipStream_t st, const int32_t* in, int64_t* out, size_t n, DevBuf& tmp) {
    auto it = rocprim::make_transform_iterator(in, [] __device__(int32_t v) { return (int64_t)v; });
    size_t need = 0;
    GD_HIP(rocprim::exclusive_scan(nullptr, need, it, out, (int64_t)0, n, rocprim::plus<int64_t>(), st));
    if (!tmp.p || need > tmp.bytes) tmp.alloc(std::max<size_t>(need, 8), st);   // never null: null asks for the size
    GD_HIP(rocprim::exclusive_scan(tmp.p, need, it, out, (int64_t)0, n, rocprim::plus<int64_t>(), st));
}

constexpr int kLoads = 4;                    // 64-column loads a lane has in flight
constexpr int kSegCols = 64 * kLoads * 2;    // columns of a tile

// The test of one (row q, column c0 + b) cell, b < nc.
//  FromCounts: d is the Java expression of epilogue_kernel (matrix_step.hip) and
//  closest_select_kernel from I, fp64, no contraction; else d is loaded from D.
//  The row's size comes from roff, the column's from coff: one collection
//  passes the same pointer twice, gdist_cross_within the queries' and the
//  subjects' (with keep_self and without upper: q and j index different
//  collections there and their comparison decides nothing).
template <bool FromCounts>
struct RowView {
    const int32_t* Ir;
    const double* Dr;
    const int64_t* coff;
    int64_t na, q, c0;
    int empty_nan, keep_self, upper;
    double max_dist;

    __device__ __forceinline__ double dist(int64_t b) const {
#pragma clang fp contract(off)
        if (!FromCounts) return Dr[b];
        const int64_t j = c0 + b;
        const int64_t inter = Ir[b];
        const int64_t nb = coff[j + 1] - coff[j];
        if (inter > 0) {
            const double uni = (double)(na + nb - inter);
            return 1.0 - (double)inter / uni;
        }
        return (empty_nan && na + nb == 0) ? __builtin_nan("") : 1.0;
    }
    __device__ __forceinline__ bool ok(double d, int64_t b) const {
        const int64_t j = c0 + b;
        return d <= max_dist && (upper ? j > q : (keep_self || j != q));   // NaN fails the <=
    }
};

template <bool FromCounts>
__device__ __forceinline__ RowView<FromCounts> row_view(const void* src, int64_t ld, const int64_t* roff,
                                                       const int64_t* coff, int empty_nan, int64_t q0, int64_t a,
                                                       int64_t c0, int keep_self, int upper, double max_dist) {
    RowView<FromCounts> v;
    v.Ir = static_cast<const int32_t*>(src) + a * ld;
    v.Dr = static_cast<const double*>(src) + a * ld;
    v.coff = coff;
    v.q = q0 + a;
    v.na = 0;
    if (FromCounts) v.na = roff[v.q + 1] - roff[v.q];
    v.c0 = c0;
    v.empty_nan = empty_nan;
    v.keep_self = keep_self;
    v.upper = upper;
    v.max_dist = max_dist;
    return v;
}

// Rows [q0, q0 + nrows) against the step's columns [c0, c0 + nc): src is I
// (int32) or D (double), row a / column b at src[a * ld + b]. Tile it = a *
// nseg + segment; tile_count[it] = its survivors.
template <bool FromCounts>
__global__ __launch_bounds__(256) void within_count_kernel(
    const void* __restrict__ src, int64_t ld, const int64_t* __restrict__ roff, const int64_t* __restrict__ coff,
    int empty_nan, int64_t q0, int64_t c0, int64_t nc, int keep_self, int upper, double max_dist, int64_t ntiles,
    int64_t nseg, int32_t* __restrict__ tile_count) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * 4 + wave;
    if (it >= ntiles) return;   // no workgroup barrier below: a wave may leave alone
    const int64_t a = it / nseg, b0 = (it - a * nseg) * kSegCols;
    const int64_t bend = min(nc, b0 + (int64_t)kSegCols);
    const RowView<FromCounts> v =
        row_view<FromCounts>(src, ld, roff, coff, empty_nan, q0, a, c0, keep_self, upper, max_dist);
    int cnt = 0;
    if (!(upper && c0 + bend - 1 <= v.q)) {   // else wholly on or left of the diagonal (wave-uniform)
        for (int64_t g0 = b0; g0 < bend; g0 += 64 * kLoads) {
            double dv[kLoads];
#pragma unroll
            for (int u = 0; u < kLoads; u++) {
                const int64_t b = g0 + u * 64 + lane;
                dv[u] = b < bend ? v.dist(b) : __builtin_nan("");   // past the ragged end: never qualifies
            }
#pragma unroll
            for (int u = 0; u < kLoads; u++) cnt += __popcll(__ballot(v.ok(dv[u], g0 + u * 64 + lane)));
        }
    }
    if (lane == 0) tile_count[it] = cnt;
}

// row_base[a] = tile_base[a * nseg], a in [0, nrows]: what the host reads back
__global__ void within_row_base_kernel(const int64_t* __restrict__ tile_base, int64_t nseg, int64_t nrows,
                                       int64_t* __restrict__ row_base) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a <= nrows) row_base[a] = tile_base[a * nseg];
}

// The count kernel's tiling and test again; tile_base: the exclusive scan of
// tile_count with the step's total at [ntiles]. A survivor at position p <
// limit goes to col_out[p] / d_out[p] (the step's staging buffers).
template <bool FromCounts>
__global__ __launch_bounds__(256) void within_write_kernel(
    const void* __restrict__ src, int64_t ld, const int64_t* __restrict__ roff, const int64_t* __restrict__ coff,
    int empty_nan, int64_t q0, int64_t c0, int64_t nc, int keep_self, int upper, double max_dist, int64_t ntiles,
    int64_t nseg, const int64_t* __restrict__ tile_base, int64_t limit, int64_t* __restrict__ col_out,
    double* __restrict__ d_out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * 4 + wave;
    if (it >= ntiles) return;   // no workgroup barrier below: a wave may leave alone
    int64_t pos = tile_base[it];
    if (pos >= limit || tile_base[it + 1] == pos) return;   // nothing of this tile fits, or it holds nothing
    const int64_t a = it / nseg, b0 = (it - a * nseg) * kSegCols;
    const int64_t bend = min(nc, b0 + (int64_t)kSegCols);
    const RowView<FromCounts> v =
        row_view<FromCounts>(src, ld, roff, coff, empty_nan, q0, a, c0, keep_self, upper, max_dist);
    for (int64_t g0 = b0; g0 < bend; g0 += 64 * kLoads) {
        double dv[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; u++) {
            const int64_t b = g0 + u * 64 + lane;
            dv[u] = b < bend ? v.dist(b) : __builtin_nan("");
        }
#pragma unroll
        for (int u = 0; u < kLoads; u++) {
            const int64_t b = g0 + u * 64 + lane;
            const bool ok = v.ok(dv[u], b);
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const int r = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                const int64_t p = pos + r;
                if (p < limit) {
                    col_out[p] = c0 + b;
                    d_out[p] = dv[u];
                }
            }
            pos += __popcll(m);
        }
    }
}

}  // namespace

// Rows a block of gdist_within's walk: option closest_rows when set, else
// min(4096, what keeps a worst-case step within 1 GiB), at least 1. Worst
// case: every pair qualifies, so a column costs its I or D element and a
// staged (int64 column, double d) survivor.
int64_t within_rows(const gdist_ctx* ctx, int64_t nr, int64_t nc, size_t elem) {
    const int64_t per_row = std::max<int64_t>(nc, 1) * (int64_t)(elem + 16);
    int64_t R = std::max<int64_t>(1, std::min<int64_t>(4096, (int64_t(1) << 30) / per_row));
    if (ctx->has_option(OPT_CLOSEST_ROWS)) R = std::max<int64_t>(1, ctx->option(OPT_CLOSEST_ROWS, R));
    return std::min<int64_t>(R, std::max<int64_t>(nr, 1));
}

// The steps arrive in row order and a step spans the call's columns, so its
// survivors are already in output order. rowptr: r1 - r0 + 1 entries, written
// whole. col_out / d_out: the first min(total, capacity) entries.
void within_compact(gdist_ctx* ctx, WalkSource& src, int64_t r0, int64_t r1, int64_t c0, int64_t c1, double max_dist,
                    int64_t capacity, int64_t* rowptr, int64_t* col_out, double* d_out) {
    hipStream_t st = ctx->stream;
    const int64_t nr = r1 - r0, nc = c1 - c0;
    const int64_t R = within_rows(ctx, nr, nc, src.elem());
    Walk walk(ctx, src, R, nc);
    const int64_t max_tiles = R * ceil_div(nc, kSegCols);
    DevBuf tcount((size_t)(max_tiles + 1) * 4, st), tbase((size_t)(max_tiles + 1) * 8, st);
    DevBuf rbase((size_t)(R + 1) * 8, st), scan_tmp;
    std::vector<int64_t> hbase((size_t)R + 1);
    const auto count = src.from_counts ? within_count_kernel<true> : within_count_kernel<false>;
    const auto write = src.from_counts ? within_write_kernel<true> : within_write_kernel<false>;
    int64_t total = 0;   // pairs of the rows before this step
    int64_t done = 0;    // rows whose rowptr entries are written
    rowptr[0] = 0;
    walk.run(r0, r1, c0, c1, true, [&](const WalkStep& t) {
        const int64_t nseg = ceil_div(t.nk, kSegCols), ntiles = t.nb * nseg;
        count<<<(unsigned)ceil_div(ntiles, 4), 256, 0, st>>>(walk.blk.p, t.nk, src.roff, src.coff, src.empty_nan, t.b0,
                                                             t.k0, t.nk, src.keep_self, src.upper, max_dist, ntiles,
                                                             nseg, tcount.as<int32_t>());
        GD_HIP(hipGetLastError());
        // ntiles + 1 elements: the step's total lands at tbase[ntiles] (the
        // last input is not part of any exclusive sum)
        scan_counts(st, tcount.as<int32_t>(), tbase.as<int64_t>(), (size_t)ntiles + 1, scan_tmp);
        within_row_base_kernel<<<(unsigned)ceil_div(t.nb + 1, 256), 256, 0, st>>>(tbase.as<int64_t>(), nseg, t.nb,
                                                                                rbase.as<int64_t>());
        GD_HIP(hipGetLastError());
    }, [&](const WalkStep& t) {
        d2h(hbase.data(), rbase.p, (size_t)(t.nb + 1) * 8, st);
        int64_t* rp = rowptr + (t.b0 - r0);
        for (int64_t a = 0; a <= t.nb; a++) rp[a] = total + hbase[a];
        const int64_t step = hbase[t.nb];
        const int64_t fit = std::min(step, std::max<int64_t>(capacity - total, 0));
        if (fit > 0) {
            const int64_t nseg = ceil_div(t.nk, kSegCols), ntiles = t.nb * nseg;
            DevBuf sc((size_t)fit * 8, st), sd((size_t)fit * 8, st);
            walk.timed_select([&] {
                write<<<(unsigned)ceil_div(ntiles, 4), 256, 0, st>>>(
                    walk.blk.p, t.nk, src.roff, src.coff, src.empty_nan, t.b0, t.k0, t.nk, src.keep_self, src.upper,
                    max_dist, ntiles, nseg, tbase.as<int64_t>(), fit, sc.as<int64_t>(), sd.as<double>());
                GD_HIP(hipGetLastError());
            });
            d2h(col_out + total, sc.p, (size_t)fit * 8, st);
            d2h(d_out + total, sd.p, (size_t)fit * 8, st);
        }
        total += step;
        done = t.b0 - r0 + t.nb;
    });
    // the row blocks wholly on or left of the diagonal (the last ones) had no step
    std::fill(rowptr + done + 1, rowptr + nr + 1, total);
}

// method: SORTED or BITSET (resolved by the caller); ignored for sketches.
void within(gdist_ctx* ctx, gdist_sets* s, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int method,
            unsigned flags, double max_dist, int64_t capacity, int64_t* rowptr, int64_t* col_out, double* d_out) {
    ctx->within_matrix_ms = ctx->within_select_ms = -1.0;
    std::fill(rowptr, rowptr + (r1 - r0) + 1, (int64_t)0);
    if (r1 == r0 || c1 == c0) return;
    SelfSource src(ctx, s, method, flags);
    within_compact(ctx, src, r0, r1, c0, c1, max_dist, capacity, rowptr, col_out, d_out);
    // option time_kernels: the matrix kernels and the count / scan / write
    // kernels of every step apart (gdist_ctx_within_timing)
    if (src.timed) {
        ctx->within_matrix_ms = src.fill_ms;
        ctx->within_select_ms = src.consume_ms;
    }
}

}  // namespace gdist
