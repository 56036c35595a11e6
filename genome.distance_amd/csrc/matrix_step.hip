// matrix_step.hip — one step of the N×N table over the tiered bitsets: what
// is launched for a region, in which order, and what it is expected to cost.
//
// The loop of SequenceKmers.distance(other) over many pairs
// (FastaDistanceProcessor.java:177-186, GenomeProcessor.java:140,
// WidthProcessor.java:159-165) is a step here: the region's counts I from the
// tiers' kernel families (dense tiles: bitset.hip; rare walks: rare.hip;
// complement-sparse words: sparse.hip; variant words: variant.hip), then the
// distances D from I and the set sizes by the Java expression, fp64.
//
//  * the cost model (block_pairs, bitset_block_cost_s, bitset_cost_s,
//    sorted_cost_s): modelled seconds of a block, read by METHOD_AUTO, the
//    per-call rare kernel choice and the cost-balanced row partition;
//  * matrix_plan: a region's tile lists on the device, cached on the
//    collection by (region, options);
//  * bitset_matrix: the ordering of a step's families over the main and the
//    side stream (fork / join events); bitset_matrix_fused: the sparse-only
//    step of two launches and its pipeline over the two tile streams;
//  * zero_counts before a step, distance_epilogue / row_epilogue after it,
//    self_pairs_kernel for the diagonal of a full block.
#include <cmath>

#include <algorithm>

#include "gdist_internal.hpp"
#include "bitset_tiles.hpp"

namespace gdist {
namespace {

// Self pairs: |A ∩ A| = |A|. The pruned dictionary drops kmers held by one
// set only, so the bitset count of a self pair misses them; take |A|.
__global__ void self_pairs_kernel(const int64_t* __restrict__ off, int64_t lo, int64_t hi, int64_t r0, int64_t c0,
                                  int32_t* __restrict__ I, int64_t ldI) {
    const int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hi) return;
    I[(i - r0) * ldI + (i - c0)] = (int32_t)(off[i + 1] - off[i]);
}

// Java expression of SequenceKmers.distance, fp64 with contraction off:
// d = I > 0 ? 1.0 - (double)I / (double)(nA + nB - I) : 1.0
__global__ void epilogue_kernel(const int64_t* __restrict__ off, int64_t r0, int64_t r1, int64_t c0,
                                int64_t c1, int upper, int empty_nan, const int32_t* __restrict__ I,
                                int64_t ldI, double* __restrict__ D, int64_t ldD) {
#pragma clang fp contract(off)
    const int64_t ncol = c1 - c0;
    const int64_t n = (r1 - r0) * ncol;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int64_t ri = e / ncol, cj = e - ri * ncol;
        const int64_t i = r0 + ri, j = c0 + cj;
        if (upper && j <= i) continue;
        const int64_t inter = I[ri * ldI + cj];
        const int64_t na = off[i + 1] - off[i], nb = off[j + 1] - off[j];
        double d;
        if (inter > 0) {
            const double uni = (double)(na + nb - inter);
            d = 1.0 - (double)inter / uni;
        } else {
            d = (empty_nan && na + nb == 0) ? __builtin_nan("") : 1.0;
        }
        D[ri * ldD + cj] = d;
    }
}

// The epilogue by rows: block row a (set i = r0 + a), its columns [lo, nc)
// (upper: j > i) strided over the blocks of the row; the same expression as
// epilogue_kernel
__global__ __launch_bounds__(256) void epilogue_rows_kernel(const int64_t* __restrict__ off, int64_t r0, int64_t c0,
                                                            int64_t nc, int upper, int empty_nan,
                                                            const int32_t* __restrict__ I, int64_t ldI,
                                                            double* __restrict__ D, int64_t ldD) {
#pragma clang fp contract(off)
    const int64_t a = blockIdx.y, i = r0 + a;
    const int64_t l0 = upper ? i + 1 - c0 : 0;
    const int64_t lo = l0 > 0 ? l0 : 0;
    const int64_t na = off[i + 1] - off[i];
    const int32_t* Ir = I + a * ldI;
    double* Dr = D + a * ldD;
    for (int64_t b = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nc; b += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = c0 + b;
        const int64_t inter = Ir[b];
        const int64_t nb = off[j + 1] - off[j];
        double d;
        if (inter > 0) {
            const double uni = (double)(na + nb - inter);
            d = 1.0 - (double)inter / uni;
        } else {
            d = (empty_nan && na + nb == 0) ? __builtin_nan("") : 1.0;
        }
        Dr[b] = d;
    }
}

__global__ void row_epilogue_kernel(const int64_t* __restrict__ off, int64_t q, const int64_t* __restrict__ cols,
                                    int64_t ncols, int empty_nan, const int32_t* __restrict__ I,
                                    double* __restrict__ D) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    const int64_t j = cols[c];
    const int64_t na = off[q + 1] - off[q], nb = off[j + 1] - off[j];
    const int64_t inter = (j == q) ? na : I[c];
    double d;
    if (inter > 0) {
        const double uni = (double)(na + nb - inter);
        d = 1.0 - (double)inter / uni;
    } else {
        d = (empty_nan && na + nb == 0) ? __builtin_nan("") : 1.0;
    }
    D[c] = d;
}

}  // namespace

void row_epilogue(gdist_ctx* ctx, const gdist_sets* s, int64_t q, const int64_t* d_cols, int64_t ncols,
                  unsigned flags, const int32_t* d_I, double* d_D) {
    if (ncols <= 0) return;
    row_epilogue_kernel<<<(unsigned)ceil_div(ncols, 256), 256, 0, ctx->stream>>>(
        s->off.as<int64_t>(), q, d_cols, ncols, (flags & GDIST_EMPTY_NAN) ? 1 : 0, d_I, d_D);
    GD_HIP(hipGetLastError());
}

double block_pairs(int64_t r0, int64_t r1, int64_t c0, int64_t c1, bool upper) {
    if (r1 <= r0 || c1 <= c0) return 0.0;
    if (!upper) return (double)(r1 - r0) * (double)(c1 - c0);
    // row i holds columns max(c0, i + 1) .. c1 - 1: full rows while i + 1 <= c0,
    // then c1 - 1 - i for i in [c0, c1 - 1)
    const int64_t a = std::min(r1, std::max(r0, c0));            // rows [r0, a): all nc columns
    double p = (double)(a - r0) * (double)(c1 - c0);
    const int64_t b0 = a, b1 = std::min(r1, c1 - 1);              // rows [b0, b1): c1 - 1 - i columns
    if (b1 > b0) p += 0.5 * (double)(b1 - b0) * (double)((c1 - 1 - b0) + (c1 - b1));
    return p;
}

// The 128 x 128 tiles bitset_matrix launches on a block (same enumeration:
// upper-triangle blocks tile their columns from corg = r0 mod BT, diagonal
// tiles go to the DIAG launch), counted per row tile in closed form. A
// partial last row tile with RR = ceil(rows / 16) <= kPartialMaxRR runs RR of
// 8 accumulator rows and costs ~RR/8 of a tile (at least 2/8: the column
// fragments are read from LDS whatever RR is); partial columns cost full
// tiles. What the row partition must see.
static void dense_tiles(int64_t r0, int64_t r1, int64_t c0, int64_t c1, bool upper, double* off, double* diag) {
    *off = *diag = 0.0;
    if (r1 <= r0 || c1 <= c0) return;
    const int64_t tr = ceil_div(r1 - r0, BT);
    const int64_t rr = ceil_div(r1 - r0 - (tr - 1) * BT, 16);
    const double last_w = rr <= kPartialMaxRR ? (double)std::max<int64_t>(2, rr) / 8.0 : 1.0;
    auto w = [&](int64_t a) { return a == tr - 1 ? std::min(1.0, last_w) : 1.0; };
    if (!upper) {
        *off = ((double)(tr - 1) + w(tr - 1)) * (double)ceil_div(c1 - c0, BT);
        return;
    }
    const int64_t corg = c0 - (((c0 - r0) % BT) + BT) % BT;
    const int64_t dlt_t = (r0 - corg) / BT, tc2 = ceil_div(c1 - corg, BT);
    for (int64_t a = 0; a < tr; a++) {
        const int64_t x = std::max(c0, r0 + a * BT + 1);   // tile b is launched iff its last column cmax >= x
        if (c1 - 1 < x) break;                            // rows only grow: no later row tile has any
        const int64_t b_lo = std::max<int64_t>(0, ceil_div(x + 1 - corg, BT) - 1);
        if (b_lo >= tc2) continue;
        const bool has_diag = a + dlt_t >= b_lo && a + dlt_t < tc2;
        *diag += (has_diag ? 1.0 : 0.0) * w(a);
        *off += ((double)(tc2 - b_lo) - (has_diag ? 1.0 : 0.0)) * w(a);
    }
}

// the variant tier's row walk: its share of the products, and one list
// search per (entry of the block's rows, column chunk)
static double variant_cost_s(const gdist_sets* s, double f_area, double f_rows, double ncols) {
    if (!s->variant) return 0.0;
    return f_area * s->vw_products / kVariantProductsPerS +
           f_rows * (double)s->vw_entries * std::ceil(ncols / 16384.0) / kVariantVisitsPerS;
}

double bitset_block_cost_s(const gdist_sets* s, int64_t r0, int64_t r1, int64_t c0, int64_t c1, bool upper,
                           bool* rare_row_major) {
    const double n = (double)s->nsets, tot = 0.5 * n * (n - 1.0);
    const double pairs = block_pairs(r0, r1, c0, c1, upper);
    const RareChoice rc = rare_choice(rare_tier(s), tot > 0 ? std::min(1.0, pairs / tot) : 1.0,
                                      n > 0 ? (double)(r1 - r0) / n : 1.0);
    if (rare_row_major) *rare_row_major = rc.row_major;
    double off, diag;
    dense_tiles(r0, r1, c0, c1, upper, &off, &diag);
    const double tW = s->sparse ? (s->sp_fold_dense ? 0.0 : (double)s->Wd) : (double)s->W;
    // sparse tiles: exactly the tiles the block's sparse plan launches (a
    // thin, unaligned row block still visits every word in each of its row
    // blocks' tiles: round-2 G = 8 emulation, balance 0.76 with the area estimate)
    double sp_tiles = 0.0;
    if (s->sparse && r1 > r0 && c1 > c0)
        for (int64_t A = r0 / BT; A <= (r1 - 1) / BT; A++)
            for (int64_t B = c0 / BT; B <= (c1 - 1) / BT; B++) {
                const int64_t rmin = std::max(r0, A * BT);
                const int64_t cmax = std::min(c1, (B + 1) * BT) - 1;
                if (!(upper && cmax <= rmin)) sp_tiles += 1.0;
            }
    // the rare tier's pairs are recounted by the sparse tile launch's rare
    // rows (sparse.hip rare_slab_plan) when the tier is small and its lists
    // short; priced as the list-major kernel beside the tiles
    const bool rare_in_reduce = s->sparse && s->n_rare > 0 && s->rare_max_list <= kLongList &&
                                (double)s->rare_records + (double)s->rare_incs <= double(int64_t(1) << 26);
    return (off + kDiagTileShare * diag) * (double)(BT * BT) * tW / kDenseWordPairsPerS +
           (rare_in_reduce ? rc.list_s * kRareOverlapExposed : rc.cost()) +
           sparse_block_cost_s(s, tot > 0 ? std::min(1.0, pairs / tot) : 1.0, sp_tiles) +
           variant_cost_s(s, tot > 0 ? std::min(1.0, pairs / tot) : 1.0, n > 0 ? (double)(r1 - r0) / n : 1.0,
                          (double)(c1 - c0));
}

double bitset_cost_s(const gdist_sets* s, double pairs) {
    // a region given only by its pair count: its share of the rows taken as its share of the pairs
    const double tot = 0.5 * (double)s->nsets * (double)(s->nsets - 1);
    const double frac = tot > 0 ? std::min(1.0, pairs / tot) : 1.0;
    const double tW = s->sparse ? (s->sp_fold_dense ? 0.0 : (double)s->Wd) : (double)s->W;
    return pairs * tW / kDenseWordPairsPerS + rare_choice(rare_tier(s), frac, frac).cost() +
           sparse_block_cost_s(s, frac, pairs / (double)(BT * BT) + std::sqrt(2.0 * pairs) / BT) +
           variant_cost_s(s, frac, frac, (double)s->nsets);
}

double sorted_cost_s(const gdist_sets* s, double pairs) {
    // streaming hash join: 8(n_i + n_j) bytes per pair at ~6 TB/s (C3)
    const double mean_n = s->nsets ? (double)s->total / (double)s->nsets : 0.0;
    return pairs * 16.0 * mean_n / kSortedBytesPerS;
}

// The region's launch plan (tile groups, K-split, the sparse plan's slot),
// built once per region and option set, then reused
static MatrixPlan& matrix_plan(gdist_ctx* ctx, const gdist_sets* s, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                               bool upper) {
    hipStream_t st = ctx->stream;
    const int64_t nr = r1 - r0;
    const int tr = (int)ceil_div(nr, BT);
    // dense tile operands: every word, or only the dense words when the
    // complement-sparse words run in their own kernel (sparse.hip)
    const int64_t tW = s->sparse ? s->Wd : s->W;
    // Diagonal tiles of an upper-triangle region (row0 == col0) get their
    // own launch of the DIAG variant, which skips the accumulators that
    // only hold pairs with j <= i (option bitset_diag = 0 keeps one launch).
    const bool split_diag = upper && ctx->option(OPT_BITSET_DIAG, 1) != 0;
    // The last row tile of a block whose rows are not a multiple of BT
    // holds nlast rows: its tiles get launches instantiated for
    // RR = ceil(nlast / 16) accumulator rows, skipping the others' work.
    // (option bitset_partial_rr: the largest RR given its own launches, A/B)
    const int max_rr = (int)ctx->option(OPT_BITSET_PARTIAL_RR, kPartialMaxRR);

    // ---- the region's launch plan (built once, then reused)
    // the key holds every option the plan (and the sparse plan in it) reads,
    // so that changing one builds a new plan instead of reusing a stale one
    // the dense tiles on the matrix cores (FP4 MFMA) when there are enough
    // words to amortise a 256 x 256 tile's stages, however few the tiles
    // (C2-realistic: 10 tiles of 1,936 dense words, step 0.317 ms against
    // 0.442 with the AND+popcount tiles, profiles/r05/s12/ab_c2r.txt;
    // option bitset_mfma 0: the AND+popcount tiles)
    const bool use_mfma = tW >= kMfmaMinWords && ctx->option(OPT_BITSET_MFMA, 1) != 0;
    const std::vector<int64_t> key{r0, r1, c0, c1, upper ? 1 : 0, split_diag ? 1 : 0, max_rr, tW, use_mfma ? 1 : 0,
                                   ctx->option(OPT_BITSET_MFMA_GROUP, 0),
                                   ctx->option(OPT_SPARSE_RARE, 1), ctx->option(OPT_SPARSE_CHUNKS, -1),
                                   ctx->option(OPT_SPARSE_PART_BUDGET, -1), ctx->option(OPT_SPARSE_WG_PER_CU, -1),
                                   ctx->option(OPT_SPARSE_XCD, 0), ctx->option(OPT_SPARSE_BALANCE, kSparseBalanceDefault)};
    auto it = s->plans.find(key);
    if (it == s->plans.end()) {
        if (s->plans.size() >= 8) {   // row-block loops: keep the cache small
            // launches on either stream may still read the old plans' buffers
            GD_HIP(hipStreamSynchronize(ctx->side));
            GD_HIP(hipStreamSynchronize(ctx->tile2));
            GD_HIP(hipStreamSynchronize(ctx->stream));
            s->graphs.clear();        // (captured steps hold the plans' buffers)
            s->plans.clear();
        }
        auto plan = std::make_unique<MatrixPlan>();
        MatrixPlan& p = *plan;
        // Upper-triangle regions tile their columns from an origin corg <= c0
        // with corg = r0 (mod BT), so tiles lie exactly on the diagonal whatever
        // r0 is (row-sharded ranks get exact equal-area row blocks); columns
        // below c0 are loaded clamped and discarded. Diagonal tiles: col0 == row0.
        p.corg = split_diag ? c0 - (((c0 - r0) % BT) + BT) % BT : c0;
        const int64_t dlt_t = (r0 - p.corg) / BT;
        const int64_t nlast = nr - (int64_t)(tr - 1) * BT;
        p.rr = (int)ceil_div(nlast, 16);
        p.part = p.rr <= max_rr;
        std::vector<int2> grp[4];   // off-diagonal, diagonal, partial off-diagonal, partial diagonal
        const int tc2 = (int)ceil_div(c1 - p.corg, BT);
        for (int a = 0; a < tr; a++)
            for (int b = 0; b < tc2; b++) {
                const int64_t rmin = r0 + (int64_t)a * BT;
                const int64_t cmax = std::min<int64_t>(c1, p.corg + (int64_t)(b + 1) * BT) - 1;
                if (cmax < c0 || (upper && cmax <= rmin)) continue;
                const int g = ((split_diag && (int64_t)b - a == dlt_t) ? 1 : 0) + ((p.part && a == tr - 1) ? 2 : 0);
                grp[g].push_back(make_int2(a, b));
            }
        for (int g = 0; g < 4; g++) p.at[g + 1] = p.at[g] + grp[g].size();
        if (use_mfma) {
            // the MFMA tiles: 256 x 256 from (r0, c0), those holding a pair of the region
            // (option bitset_mfma_group G > 0: the tiles in blocks of G row
            // tiles x 2G column tiles, so the ~32 consecutive tiles an XCD runs
            // at once share G row panels and 2G column panels in its L2)
            std::vector<int2> mt;
            const int tm = (int)ceil_div(nr, MT), tn = (int)ceil_div(c1 - c0, MT);
            const int gr = (int)std::max<int64_t>(1, ctx->option(OPT_BITSET_MFMA_GROUP, 0));
            const int gc = ctx->option(OPT_BITSET_MFMA_GROUP, 0) > 0 ? 2 * gr : tn;
            for (int a0 = 0; a0 < tm; a0 += gr)
                for (int b0 = 0; b0 < tn; b0 += gc)
                    for (int a = a0; a < std::min(tm, a0 + gr); a++)
                        for (int b = b0; b < std::min(tn, b0 + gc); b++) {
                            const int64_t rmin = r0 + (int64_t)a * MT;
                            const int64_t cmax = std::min<int64_t>(c1, c0 + (int64_t)(b + 1) * MT) - 1;
                            if (upper && cmax <= rmin) continue;
                            mt.push_back(make_int2(a, b));
                        }
            p.nmt = (int64_t)mt.size();
            p.mtiles.alloc(mt.size() * sizeof(int2) + 8, st);
            if (!mt.empty()) h2d(p.mtiles.p, mt.data(), mt.size() * sizeof(int2), st);
        }
        p.tiles.alloc(p.at[4] * sizeof(int2) + 8, st);
        for (int g = 0; g < 4; g++)
            if (!grp[g].empty()) h2d(p.tiles.as<int2>() + p.at[g], grp[g].data(), grp[g].size() * sizeof(int2), st);
        it = s->plans.emplace(key, std::move(plan)).first;
    }
    return *it->second;
}

// One step's launches in their order: which family goes on which stream,
// behind which event. The families' kernels, grids and K splits are their
// launchers' (dense_tiles_launch in bitset.hip; rare_pairs_launch and
// rare_rows_launch in rare.hip; sparse_matrix; variant_matrix).
void bitset_matrix(gdist_ctx* ctx, const gdist_sets* s, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                   bool upper, int32_t* d_I, int64_t ldI) {
    hipStream_t st = ctx->stream;
    if (r1 - r0 <= 0 || c1 - c0 <= 0) return;
    const Region g{r0, r1, c0, c1, upper};
    MatrixPlan& p = matrix_plan(ctx, s, r0, r1, c0, c1, upper);
    if (p.at[4] == 0) {         // no pair in the region: an empty kernel span (the caller reads it)
        if (!ctx->capturing) {
            GD_HIP(hipEventRecord(ctx->ev_k0, st));
            GD_HIP(hipEventRecord(ctx->ev_k1, st));
        }
        return;
    }

    // Rare kernel per call from the cost model (rare_choice): list-major opens
    // every list and walks the pairs from this block's rows with global
    // atomics (short lists, blocks with few pairs per row: C2, the last rank
    // of a row-sharded triangle); row-major walks each row's lists into LDS
    // counters (lists feeding several increments per record: C3, C4; ranks
    // with many pairs per row). GDIST_RARE_KERNEL=0|1 forces one (A/B). The
    // list-major kernel uses atomics only, like the dense kernel, so it runs
    // beside the dense launch on the side stream (GDIST_RARE_OVERLAP=0 keeps
    // it in line).
    bool row_major = false;
    if (s->n_rare > 0) (void)bitset_block_cost_s(s, r0, r1, c0, c1, upper, &row_major);
    const bool list_major = ctx->has_option(OPT_RARE_KERNEL) ? ctx->option(OPT_RARE_KERNEL, 0) == 0 : !row_major;
    const bool overlap = s->n_rare > 0 && list_major && ctx->option(OPT_RARE_OVERLAP, 1) != 0;
    // The row-major rare kernel too, when it flushes its rows with atomics
    // (round 3, C3: its scattered list reads overlap the VALU-bound tiles)
    const bool rows_side = s->n_rare > 0 && !list_major && !s->sparse && ctx->option(OPT_RARE_OVERLAP, 1) != 0;
    // The sparse words and the list-major rare kernel add atomically, like
    // the dense tiles, so they run on the side stream beside them; so does
    // the variant tier's row walk (variant.hip)
    const bool side = overlap || s->sparse || rows_side || s->variant;
    bool rare_done = false;               // the sparse chunk reduce added the rare pairs
    if (!ctx->capturing) GD_HIP(hipEventRecord(ctx->ev_k0, st));
    // option serial_step = 1: the side stream's families run on the main
    // stream before the dense tiles, one after another (each family's time
    // alone: the C4 slice's MFMA tiles and variant walk otherwise share the
    // CUs); option dense_first: the dense tiles are issued before the side
    // stream's launches (which still wait only for the fork) — by default
    // unless the side stream carries the sparse tiles (C3: step 2.51 vs
    // 2.63 ms, C4 slice 15.8 vs 16.0 ms; C2-realistic's sparse launch first:
    // 0.321 vs 0.353 ms, profiles/r05/s16/)
    const bool serial = ctx->option(OPT_SERIAL_STEP, 0) != 0;
    // MFMA tiles that store their counts (option bitset_mfma_store) are the
    // first writers of I: the fork is recorded after the dense launch, so the
    // side families start after them
    const MfmaChoice mfma = mfma_choice(ctx, s, p);
    const bool mstore = mfma.store;
    const bool dense_first = side && (mstore || (!serial && ctx->option(OPT_DENSE_FIRST, s->sparse ? 0 : 1) != 0));
    if (side && !mstore) GD_HIP(hipEventRecord(ctx->ev_fork, st));
    auto launch_side = [&]() {
        hipStream_t sd = serial ? st : ctx->side;
        GD_HIP(hipStreamWaitEvent(sd, ctx->ev_fork, 0));
        if (s->sparse) rare_done = sparse_matrix(ctx, s, r0, r1, c0, c1, upper, d_I, ldI, sd, p.sparse);
        // beside the sparse kernel the list-major rare kernel goes to the main
        // stream after the dense tiles (the side stream is busy until the
        // sparse tiles and their reduce end: C2 0.0185 ms in line there)
        if (overlap && !s->sparse) rare_pairs_launch(ctx, s, g, d_I, ldI, sd);
        if (rows_side) rare_rows_launch(ctx, s, g, d_I, ldI, sd, true);
        if (s->variant) variant_matrix(ctx, s, r0, r1, c0, c1, upper, d_I, ldI, sd);
        GD_HIP(hipGetLastError());
        GD_HIP(hipEventRecord(ctx->ev_join, sd));
    };
    if (side && !dense_first) launch_side();
    dense_tiles_launch(ctx, s, p, mfma, g, side, d_I, ldI);
    if (side && mstore) GD_HIP(hipEventRecord(ctx->ev_fork, st));   // after the stored tiles
    if (dense_first) launch_side();
    if (overlap && s->sparse && !rare_done) rare_pairs_launch(ctx, s, g, d_I, ldI, st);
    GD_HIP(hipGetLastError());
    ctx->last.launches = 1;
    if (side) GD_HIP(hipStreamWaitEvent(st, ctx->ev_join, 0));
    // the rare walk that did not run beside the tiles runs behind the join
    if (s->n_rare > 0 && !rare_done) {
        if (overlap) {
        } else if (list_major) {
            rare_pairs_launch(ctx, s, g, d_I, ldI, st);
        } else if (!rows_side) {
            rare_rows_launch(ctx, s, g, d_I, ldI, st, false);
        }
        GD_HIP(hipGetLastError());
        ctx->last.launches = 2;
    }
    if (!ctx->capturing) GD_HIP(hipEventRecord(ctx->ev_k1, st));
    const int64_t lo = std::max(r0, c0), hi = std::min(r1, c1);
    if (!upper && hi > lo) {
        self_pairs_kernel<<<(unsigned)ceil_div(hi - lo, 256), 256, 0, st>>>(s->off.as<int64_t>(), lo, hi, r0, c0, d_I,
                                                                             ldI);
        GD_HIP(hipGetLastError());
    }
}

bool bitset_matrix_fused(gdist_ctx* ctx, const gdist_sets* s, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                         bool upper, unsigned flags, int32_t* d_I, int64_t ldI, double* d_D, int64_t ldD,
                         bool pipelined) {
    // One stream, two launches: the sparse tile kernel (dense words folded
    // in) and its chunk reduce, which adds the rare pairs, STORES I (no
    // zeroing) and writes D (no epilogue launch). Only when every count of
    // the region comes from that reduce: sparse tier, no dense-word launch,
    // chunk partials, the rare pairs in its table (or no rare tier).
    if (!s->sparse || s->variant || !d_D || ctx->option(OPT_SPARSE_FUSED, 1) == 0) return false;
    if (r1 <= r0 || c1 <= c0 || !(s->sp_fold_dense || s->Wd == 0)) return false;
    MatrixPlan& p = matrix_plan(ctx, s, r0, r1, c0, c1, upper);
    sparse_plan(ctx, s, r0, r1, c0, c1, upper, ctx->stream, p.sparse);
    if (p.sparse.ntiles == 0 || !p.sparse.use_part || (s->n_rare > 0 && !p.sparse.rare_in)) return false;
    SparseEpilogue ep;
    ep.D = d_D;
    ep.ldD = ldD;
    ep.off = s->off.as<int64_t>();
    ep.empty_nan = (flags & GDIST_EMPTY_NAN) ? 1 : 0;
    hipStream_t st = ctx->stream;
    if (pipelined) {
        // Consecutive steps share nothing but the partials and the rare
        // slab: with two copies of those, this step's tile launch goes to a
        // stream of its own (the two tile streams turn about, so that two
        // consecutive launches never queue behind each other) and fills the
        // slots the previous launch's tail leaves idle, while the previous
        // reduce runs beside it. The reduce stays on the context's stream,
        // behind the event of its tile launch: outputs complete in that
        // stream's order, and every tile launch so far has finished when
        // this step's reduce runs, so whatever is ordered against the
        // context's stream later (downloads, frees, rebuilds, other queries)
        // is ordered against the tile streams too.
        SparseScratch& sc = p.sparse;
        if (!sparse_pipe_ready(ctx, sc)) return false;
        const int64_t seq = ctx->api_seq.load();
        SparsePipe pp;
        pp.copy = (int)(sc.turn & 1);
        const int ts = (int)(ctx->pipe_calls & 1);
        pp.tile_st = ts ? ctx->tile2 : ctx->side;
        pp.ev_tile = ctx->ev_tile[ts];
        // The forward hazard: the tile launch must not pass work queued on
        // the context's stream before this call. In an unbroken run of
        // pipelined steps on one collection (the API entry before this one
        // was such a step) a plan that already took a step of the run has
        // nothing of its own on that stream but its reduces: the launch
        // waits only for the reduce that last read the copy it overwrites,
        // two of the plan's steps back. Anything else (the plan's first
        // step of a run, another collection, any other call in between) is
        // fully ordered behind the context's stream.
        const bool run = ctx->pipe_sets == s && ctx->pipe_seq + 1 == seq;
        if (!run) ctx->pipe_run0 = seq;
        if (run && sc.pipe_seq >= ctx->pipe_run0) {
            if (sc.ev_read_set[pp.copy]) GD_HIP(hipStreamWaitEvent(pp.tile_st, sc.ev_read[pp.copy], 0));
        } else {
            GD_HIP(hipEventRecord(ctx->ev_order, st));
            GD_HIP(hipStreamWaitEvent(pp.tile_st, ctx->ev_order, 0));
            ctx->n_pipe_ordered++;
        }
        sparse_matrix(ctx, s, r0, r1, c0, c1, upper, d_I, ldI, st, sc, &ep, &pp);
        GD_HIP(hipEventRecord(sc.ev_read[pp.copy], st));
        sc.ev_read_set[pp.copy] = true;
        sc.turn++;
        sc.pipe_seq = seq;
        ctx->pipe_calls++;
        ctx->pipe_seq = seq;
        ctx->pipe_sets = s;
        ctx->n_pipe++;
        ctx->last.launches = 1;
        return true;
    }
    if (!ctx->capturing) GD_HIP(hipEventRecord(ctx->ev_k0, st));
    sparse_matrix(ctx, s, r0, r1, c0, c1, upper, d_I, ldI, st, p.sparse, &ep);
    if (!ctx->capturing) GD_HIP(hipEventRecord(ctx->ev_k1, st));
    ctx->last.launches = 1;
    return true;
}

namespace {
// row a of the block: columns j > i zeroed, 16-byte stores from the first
// 16-byte boundary (round 5: 4-byte stores ran at 2.3 TB/s, C3 0.088 ms a step)
__global__ void zero_upper_kernel(int32_t* __restrict__ I, int64_t ldI, int64_t r0, int64_t c0, int64_t nr, int64_t nc) {
    const int64_t a = blockIdx.y;
    const int64_t l0 = r0 + a + 1 - c0;                 // first column position with j > i
    const int64_t lo = l0 > 0 ? l0 : 0;
    if (lo >= nc) return;
    int32_t* row = I + a * ldI;
    const int64_t head = std::min<int64_t>(nc - lo, (int64_t)(((16u - ((uintptr_t)(row + lo) & 15u)) & 15u) >> 2));
    if (blockIdx.x == 0 && threadIdx.x < head) row[lo + threadIdx.x] = 0;
    const int64_t bb = lo + head, n4 = (nc - bb) >> 2;
    int4* body = reinterpret_cast<int4*>(row + bb);
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n4; k += (int64_t)gridDim.x * blockDim.x)
        body[k] = make_int4(0, 0, 0, 0);
    const int64_t t = bb + 4 * n4 + threadIdx.x;
    if (blockIdx.x == 0 && t < nc) row[t] = 0;
}
}  // namespace

void zero_counts(gdist_ctx* ctx, int64_t r0, int64_t r1, int64_t c0, int64_t c1, bool upper, int32_t* d_I,
                 int64_t ldI) {
    const int64_t nr = r1 - r0, nc = c1 - c0;
    if (nr <= 0 || nc <= 0) return;
    if (!upper) {
        GD_HIP(hipMemset2DAsync(d_I, ldI * 4, 0, nc * 4, nr, ctx->stream));
        return;
    }
    for (int64_t a0 = 0; a0 < nr; a0 += 65535) {       // grid.y limit
        const int64_t rows = std::min<int64_t>(65535, nr - a0);
        dim3 grid((unsigned)std::min<int64_t>(16, ceil_div(nc, 1024)), (unsigned)rows);
        zero_upper_kernel<<<grid, 256, 0, ctx->stream>>>(d_I + a0 * ldI, ldI, r0 + a0, c0, rows, nc);
        GD_HIP(hipGetLastError());
    }
}

void distance_epilogue(gdist_ctx* ctx, const gdist_sets* s, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                       bool upper, unsigned flags, const int32_t* d_I, int64_t ldI, double* d_D, int64_t ldD) {
    const int64_t nr = r1 - r0, nc = c1 - c0;
    if (nr <= 0 || nc <= 0) return;
    // a block row a, its columns strided (round 5: the flat kernel's 64-bit
    // division per element and its skipped lower half ran C3's epilogue at
    // 0.18 ms a step; option epilogue_rows 0 keeps it, A/B)
    if (ctx->option(OPT_EPILOGUE_ROWS, 1) == 0) {
        epilogue_kernel<<<grid_for(nr * nc), 256, 0, ctx->stream>>>(s->off.as<int64_t>(), r0, r1, c0, c1,
                                                                     upper ? 1 : 0, (flags & GDIST_EMPTY_NAN) ? 1 : 0,
                                                                     d_I, ldI, d_D, ldD);
        GD_HIP(hipGetLastError());
        return;
    }
    for (int64_t a0 = 0; a0 < nr; a0 += 65535) {       // grid.y limit
        const int64_t rows = std::min<int64_t>(65535, nr - a0);
        dim3 grid((unsigned)std::min<int64_t>(16, ceil_div(nc, 1024)), (unsigned)rows);
        epilogue_rows_kernel<<<grid, 256, 0, ctx->stream>>>(s->off.as<int64_t>(), r0 + a0, c0, nc, upper ? 1 : 0,
                                                           (flags & GDIST_EMPTY_NAN) ? 1 : 0, d_I + a0 * ldI,
                                                           ldI, d_D + a0 * ldD, ldD);
        GD_HIP(hipGetLastError());
    }
}

}  // namespace gdist
