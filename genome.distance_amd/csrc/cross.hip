// cross.hip — new query sets against a resident collection (gdist_cross_*).
//
// The reference keeps its genome database loaded and answers one
// getClosest(kmers, n, maxDist) per incoming genome (FindProcessor.java:94-110,
// MashProcessor.java:130-150). Here the subjects are a collection that stays
// as it is (its codes and its segment index are read, nothing of it is
// written) and the queries are another collection of the same kmer spec.
//
// Query segment index: per row block the query rows are cut by the SUBJECTS'
// splitters (sorted.hip segment_rows) into a scratch [rows][nseg + 1] index of
// the queries' codes; segment p of a query can only meet segment p of a
// subject. Nothing is cached on either collection.
//
// Units (cross_plan.hpp, host): (query row, block of <= 64 consecutive subject
// columns, segment range). sorted_join_kernel's one workgroup per (row, block)
// leaves one query against 1,000 subjects with 16 workgroups on 256 CUs, each
// hashing the whole query; a (row, block) over the budget is cut by segment
// range, as gdist_pairs cuts its chunks.
//
// Kernel (cross_join_kernel): 512 threads walk units. Per segment the 64 KiB
// open-addressing LDS table is filled from the QUERY's segment (sub-chunks of
// 4,096 keys: exact, the sub-runs are disjoint; the all-ones code is kept
// beside the table as sorted_join_kernel keeps it), then each wave streams its
// columns' same segment of the SUBJECT codes, coalesced, and probes. The
// per-column counts stay in LDS; at the unit's end the non-zero ones are added
// to the zeroed I block with atomicAdd: integers, so the sum over a (row,
// block)'s units is exact and order-free.
//
// Consumers. A step's counts never leave the device; what follows the join
// differs by entry point: the distance epilogue (gdist_cross_matrix), the
// top-n select (gdist_cross_closest), the CSR compaction of within.hip
// (gdist_cross_within), the limb sums of group.hip (gdist_cross_group_stats)
// and the bucket counts of hist.hip (gdist_cross_histogram). Each is the
// kernel its one-collection twin runs, given the queries' offsets and labels
// for the rows and the subjects' for the columns.
//
// Two sketch collections take the same consumers over another source
// (SketchCrossSource, sketch_cross.hip), whose steps hold distances; nothing
// above (segment index, units, join, epilogue) runs for them.
#include <algorithm>
#include <cstring>

#include "cross_plan.hpp"
#include "gdist_internal.hpp"

namespace gdist {
namespace {

constexpr int TBL_LOG2 = 13;
constexpr int TBL = 1 << TBL_LOG2;        // 8192 slots = 64 KiB
constexpr int SUB = TBL / 2;              // keys a table fill holds at most
constexpr int NTX = 512;                  // threads of a workgroup (8 waves)
constexpr int PF = 8;                     // 64-code loads a wave keeps in flight per column
constexpr uint64_t EMPTY = ~0ULL;

__device__ __forceinline__ uint32_t slot_of(uint64_t v) {
    return (uint32_t)((v * 0x9E3779B97F4A7C15ull) >> (64 - TBL_LOG2));
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// qseg: [rows][nseg + 1] positions into qcodes, row 0 = the block's first
// query; sseg: the subjects' index. I: [rows][ldI], column 0 = subject c0;
// the units' rows and column blocks are relative to the same origin.
__global__ __launch_bounds__(NTX, 1) void cross_join_kernel(
    const uint64_t* __restrict__ qcodes, const int64_t* __restrict__ qseg, const uint64_t* __restrict__ scodes,
    const int64_t* __restrict__ sseg, int nseg, const int4* __restrict__ units, int64_t nunits, int64_t nrows,
    int64_t c0, int64_t c1, int32_t* __restrict__ I, int64_t ldI) {
    __shared__ unsigned long long table[TBL];
    __shared__ int32_t cnt[kCrossCols];
    __shared__ int has_empty_key;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t per = nseg + 1;
    int64_t u, uend, ustride;
    cross_unit_walk(gridDim.x, blockIdx.x, nunits, &u, &uend, &ustride);
    for (; u < uend; u += ustride) {
        const int4 un = units[u];
        const int64_t a = un.x;
        const int64_t cs = c0 + (int64_t)un.y * kCrossCols;
        // defensive: never address outside the region
        if (a < 0 || a >= nrows || un.y < 0 || cs >= c1 || un.z < 0 || un.w > nseg) continue;
        const int ncol = (int)(cs + kCrossCols < c1 ? kCrossCols : c1 - cs);
        const int64_t* arow = qseg + a * per;
        if (tid < kCrossCols) cnt[tid] = 0;
        for (int p = un.z; p < un.w; p++) {
            const int64_t a0 = arow[p], a1 = arow[p + 1];
            if (a0 == a1) continue;
            for (int64_t sb = a0; sb < a1; sb += SUB) {
                const int64_t se = sb + SUB < a1 ? sb + SUB : a1;
                for (int t = tid; t < TBL; t += NTX) table[t] = EMPTY;
                if (tid == 0) has_empty_key = 0;
                __syncthreads();
                for (int64_t e = sb + tid; e < se; e += NTX) {
                    const uint64_t v = qcodes[e];
                    if (v == EMPTY) { has_empty_key = 1; continue; }
                    uint32_t h = slot_of(v);
                    while (true) {
                        const unsigned long long old = atomicCAS(&table[h], EMPTY, (unsigned long long)v);
                        if (old == EMPTY) break;
                        h = (h + 1) & (TBL - 1);
                    }
                }
                __syncthreads();
                const int hek = has_empty_key;
                // column t belongs to wave t mod 8 alone: no atomics on cnt
                for (int t = wave; t < ncol; t += NTX / 64) {
                    const int64_t* brow = sseg + (cs + t) * per;
                    const int64_t b0 = brow[p], b1 = brow[p + 1];
                    int c = 0;
                    // PF wave-wide loads in flight before the first probe: a wave
                    // that waits for one 512 B load at a time streams at the
                    // memory latency, not the bandwidth
                    for (int64_t g0 = b0; g0 < b1; g0 += 64 * PF) {
                        uint64_t v[PF];
#pragma unroll
                        for (int k = 0; k < PF; k++) {
                            const int64_t e = g0 + k * 64 + lane;
                            v[k] = e < b1 ? scodes[e] : 0;
                        }
#pragma unroll
                        for (int k = 0; k < PF; k++) {
                            if (g0 + k * 64 + lane >= b1) continue;
                            if (v[k] == EMPTY) { c += hek; continue; }
                            uint32_t h = slot_of(v[k]);
                            while (true) {
                                const unsigned long long tv = table[h];
                                if (tv == v[k]) { c++; break; }
                                if (tv == EMPTY) break;
                                h = (h + 1) & (TBL - 1);
                            }
                        }
                    }
                    c = wave_sum(c);
                    if (lane == 0) cnt[t] += c;
                }
                __syncthreads();
            }
        }
        __syncthreads();
        if (tid < ncol) {
            const int c = cnt[tid];
            if (c) atomicAdd(I + a * ldI + (cs - c0) + tid, c);
        }
        __syncthreads();
    }
}

// D from I: the expression of closest_select_kernel / epilogue_kernel, the
// row's size from the queries' offsets and the column's from the subjects'
__global__ __launch_bounds__(256) void cross_epilogue_kernel(const int64_t* __restrict__ qoff,
                                                             const int64_t* __restrict__ soff, int64_t q0,
                                                             int64_t nrows, int64_t c0, int64_t nc, int empty_nan,
                                                             const int32_t* __restrict__ I, double* __restrict__ D) {
#pragma clang fp contract(off)
    const int64_t n = nrows * nc;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int64_t a = e / nc, b = e - a * nc;
        const int64_t i = q0 + a, j = c0 + b;
        const int64_t inter = I[e];
        const int64_t na = qoff[i + 1] - qoff[i], nb = soff[j + 1] - soff[j];
        double d;
        if (inter > 0) {
            const double uni = (double)(na + nb - inter);
            d = 1.0 - (double)inter / uni;
        } else {
            d = (empty_nan && na + nb == 0) ? __builtin_nan("") : 1.0;
        }
        D[e] = d;
    }
}

// The walk's source (gdist_internal.hpp) for two collections. Per row block
// the queries' segment rows; per step the plan, the zeroed counts and the join.
// No cell is left out as self or as lower triangle: row and column index
// different collections and their comparison decides nothing.
struct CrossSource : WalkSource {
    gdist_ctx* ctx;
    const gdist_sets* q;
    const gdist_sets* s;
    DevBuf qseg, dunits;
    std::vector<CrossUnit> units;
    int64_t nunits = 0;

    CrossSource(gdist_ctx* c, const gdist_sets* queries, const gdist_sets* subjects, unsigned flags)
        : ctx(c), q(queries), s(subjects) {
        empty_nan = (flags & GDIST_EMPTY_NAN) ? 1 : 0;
        roff = q->off.as<int64_t>();
        coff = s->off.as<int64_t>();
        nrsets = q->nsets;
        ncsets = s->nsets;
        timed = ctx->option(OPT_TIME_KERNELS, 0) != 0;
    }

    void rows(int64_t b0, int64_t b1) override {
        // the first block is the largest: one allocation a call
        const size_t need = (size_t)(b1 - b0) * (s->nseg + 1) * 8 + 8;
        if (qseg.bytes < need) qseg.alloc(need, ctx->stream);
        segment_rows(ctx, q->codes.as<uint64_t>(), q->off.as<int64_t>() + b0, b1 - b0, s->seg_split.as<uint64_t>(),
                     s->nseg, qseg.as<int64_t>());
    }

    void stage(int64_t b0, int64_t b1, int64_t k0, int64_t k1, void* blk) override {
        hipStream_t st = ctx->stream;
        units.clear();
        const int64_t budget =
            cross_budget(cross_region_codes(q->h_off.data(), b0, b1, s->h_off.data(), k0, k1), ctx->cus);
        cross_plan(q->h_off.data(), b0, b1, s->h_off.data(), k0, k1, s->nseg, budget, units);
        const size_t bytes = units.size() * sizeof(CrossUnit);
        if (dunits.bytes < bytes) dunits.alloc(bytes, st);
        h2d(dunits.p, units.data(), bytes, st);
        GD_HIP(hipMemsetAsync(blk, 0, (size_t)(b1 - b0) * (k1 - k0) * 4, st));
        nunits += (int64_t)units.size();
    }

    void fill(int64_t b0, int64_t b1, int64_t k0, int64_t k1, void* blk) override {
        const int64_t nu = (int64_t)units.size();
        if (!nu) return;
        // two workgroups a CU hold their tables in its LDS; a multiple of the 8 XCDs
        const unsigned grid = (unsigned)std::min<int64_t>(nu, (int64_t)std::max(ctx->cus, 8) / 8 * 8 * 2);
        cross_join_kernel<<<grid, NTX, 0, ctx->stream>>>(q->codes.as<uint64_t>(), qseg.as<int64_t>(),
                                                         s->codes.as<uint64_t>(), s->segoff.as<int64_t>(), s->nseg,
                                                         dunits.as<int4>(), nu, b1 - b0, k0, k1,
                                                         static_cast<int32_t*>(blk), k1 - k0);
        GD_HIP(hipGetLastError());
    }

    // gdist_ctx_cross_info, after a walk
    void report() const {
        ctx->cross_units = nunits;
        if (timed) {
            ctx->cross_join_ms = fill_ms;
            ctx->cross_select_ms = consume_ms;
        }
    }
};

}  // namespace

static_assert(sizeof(CrossUnit) == sizeof(int4), "units are uploaded as 16-byte records");

namespace {

// the source of the pair's kind: kmer sets join by the segment index, sketches
// merge (sketch_cross.hip); f(src) runs the walk and reports
template <class F>
void with_source(gdist_ctx* ctx, const gdist_sets* q, const gdist_sets* s, unsigned flags, F&& f) {
    if (q->kind == GDIST_SKETCH) {
        SketchCrossSource src(ctx, q, s, flags);
        f(src);
    } else {
        CrossSource src(ctx, q, s, flags);
        f(src);
    }
}

}  // namespace

// every argument checked by the caller, kmer sets: the subjects' segment index
// built; I_out / D_out: host, row stride ld, either may be null. Sketches: I
// is the common count, and D comes from the merge kernel itself (no epilogue)
void cross_matrix(gdist_ctx* ctx, const gdist_sets* q, const gdist_sets* s, int64_t q0, int64_t q1, int64_t c0,
                  int64_t c1, unsigned flags, int32_t* I_out, double* D_out, int64_t ld) {
    hipStream_t st = ctx->stream;
    int64_t R, W;
    closest_blocks(ctx, q1 - q0, c1 - c0, 12, &R, &W);   // a step's I and D
    DevBuf dD;
    if (D_out) dD.alloc((size_t)R * W * 8 + 8, st);
    std::vector<int32_t> hI;
    std::vector<double> hD;
    auto run = [&](auto& src, auto&& epilogue) {
        Walk walk(ctx, src, R, W);
        walk.run(q0, q1, c0, c1, false, [&](const WalkStep& t) { epilogue(walk, t); }, [&](const WalkStep& t) {
            const size_t cells = (size_t)t.nb * t.nk;
            if (D_out) {
                hD.resize(cells);
                d2h(hD.data(), dD.p, cells * 8, st);
                for (int64_t a = 0; a < t.nb; a++)
                    std::memcpy(D_out + (t.b0 - q0 + a) * ld + (t.k0 - c0), hD.data() + (size_t)a * t.nk,
                                (size_t)t.nk * 8);
            }
            if (I_out) {
                hI.resize(cells);
                d2h(hI.data(), walk.blk.p, cells * 4, st);
                for (int64_t a = 0; a < t.nb; a++)
                    std::memcpy(I_out + (t.b0 - q0 + a) * ld + (t.k0 - c0), hI.data() + (size_t)a * t.nk,
                                (size_t)t.nk * 4);
            }
        });
        src.report();
    };
    if (q->kind == GDIST_SKETCH) {
        SketchCrossSource src(ctx, q, s, flags);
        src.matrix = true;
        src.want_common = I_out != nullptr;
        src.d_to = dD.as<double>();
        run(src, [](Walk&, const WalkStep&) {});
        return;
    }
    CrossSource src(ctx, q, s, flags);
    run(src, [&](Walk& walk, const WalkStep& t) {
        if (!D_out) return;
        const int64_t cells = t.nb * t.nk;
        const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(cells, 256), (int64_t)ctx->cus * 16);
        cross_epilogue_kernel<<<grid, 256, 0, st>>>(src.roff, src.coff, t.b0, t.nb, t.k0, t.nk, src.empty_nan,
                                                    walk.blk.as<int32_t>(), dD.as<double>());
        GD_HIP(hipGetLastError());
    });
}

// The twins: the one-collection call's consumer over the pair's source. closest
// and within: a non-empty rectangle (n >= 1); group_stats and histogram: any
void cross_closest(gdist_ctx* ctx, const gdist_sets* q, const gdist_sets* s, int64_t q0, int64_t q1, int64_t c0,
                   int64_t c1, unsigned flags, int n, double max_dist, int64_t* idx_out, double* d_out,
                   int32_t* count_out) {
    with_source(ctx, q, s, flags, [&](auto& src) {
        closest_select(ctx, src, q0, q1, c0, c1, n, max_dist, idx_out, d_out, count_out);
        src.report();
    });
}

void cross_within(gdist_ctx* ctx, const gdist_sets* q, const gdist_sets* s, int64_t q0, int64_t q1, int64_t c0,
                  int64_t c1, unsigned flags, double max_dist, int64_t capacity, int64_t* rowptr, int64_t* col_out,
                  double* d_out) {
    with_source(ctx, q, s, flags, [&](auto& src) {
        within_compact(ctx, src, q0, q1, c0, c1, max_dist, capacity, rowptr, col_out, d_out);
        src.report();
    });
}

void cross_group_stats(gdist_ctx* ctx, const gdist_sets* q, const gdist_sets* s, int64_t q0, int64_t q1, int64_t c0,
                       int64_t c1, unsigned flags, int ntypes, const int32_t* qlabels, const int32_t* slabels,
                       gdist_group_side* out, int64_t* bad) {
    with_source(ctx, q, s, flags, [&](auto& src) {
        group_reduce(ctx, src, q0, q1, c0, c1, ntypes, qlabels, slabels, out, bad);
        if (q1 > q0 && c1 > c0) src.report();
    });
}

void cross_histogram(gdist_ctx* ctx, const gdist_sets* q, const gdist_sets* s, int64_t q0, int64_t q1, int64_t c0,
                     int64_t c1, unsigned flags, int nedges, const double* edges, int ntypes, const int32_t* qlabels,
                     const int32_t* slabels, int64_t* counts, int64_t* nans, int64_t* bad) {
    with_source(ctx, q, s, flags, [&](auto& src) {
        hist_count(ctx, src, q0, q1, c0, c1, nedges, edges, ntypes, qlabels, slabels, counts, nans, bad);
        if (q1 > q0 && c1 > c0) src.report();
    });
}

}  // namespace gdist
