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

// The walk every entry point shares: row blocks x ascending column chunks. Per
// row block the queries' segment rows; per step the plan, the zeroed counts
// and the join. `after(b0, nb, k0, nk, last)` queues the kernels that consume
// the step's counts (blk: [nb][nk] int32, inside the timed span), then
// `out(b0, nb, k0, nk, last)` downloads what the step finished.
struct CrossWalk {
    gdist_ctx* ctx;
    const gdist_sets* q;
    const gdist_sets* s;
    int64_t R, W;
    DevBuf blk, qseg, dunits;
    std::vector<CrossUnit> units;
    bool timed;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    double join_ms = 0, select_ms = 0;
    int64_t nunits = 0;

    CrossWalk(gdist_ctx* c, const gdist_sets* queries, const gdist_sets* subjects, int64_t rows, int64_t cols)
        : ctx(c), q(queries), s(subjects), R(rows), W(cols), timed(c->option(OPT_TIME_KERNELS, 0) != 0) {
        hipStream_t st = ctx->stream;
        blk.alloc((size_t)R * W * 4 + 8, st);
        qseg.alloc((size_t)R * (s->nseg + 1) * 8 + 8, st);
        if (timed) for (auto& e : ev) GD_HIP(hipEventCreate(&e));
    }
    ~CrossWalk() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }

    template <class After, class Out>
    void run(int64_t q0, int64_t q1, int64_t c0, int64_t c1, After&& after, Out&& out) {
        hipStream_t st = ctx->stream;
        const int nseg = s->nseg;
        for (int64_t b0 = q0; b0 < q1; b0 += R) {
            const int64_t b1 = std::min(q1, b0 + R), nb = b1 - b0;
            segment_rows(ctx, q->codes.as<uint64_t>(), q->off.as<int64_t>() + b0, nb, s->seg_split.as<uint64_t>(), nseg,
                         qseg.as<int64_t>());
            for (int64_t k0 = c0; k0 < c1; k0 += W) {
                const int64_t k1 = std::min(c1, k0 + W), nk = k1 - k0;
                units.clear();
                const int64_t budget =
                    cross_budget(cross_region_codes(q->h_off.data(), b0, b1, s->h_off.data(), k0, k1), ctx->cus);
                cross_plan(q->h_off.data(), b0, b1, s->h_off.data(), k0, k1, nseg, budget, units);
                const int64_t nu = (int64_t)units.size();
                if (nu) {
                    if (dunits.bytes < (size_t)nu * sizeof(CrossUnit)) dunits.alloc((size_t)nu * sizeof(CrossUnit), st);
                    h2d(dunits.p, units.data(), (size_t)nu * sizeof(CrossUnit), st);
                }
                GD_HIP(hipMemsetAsync(blk.p, 0, (size_t)nb * nk * 4, st));
                if (timed) GD_HIP(hipEventRecord(ev[0], st));
                if (nu) {
                    // two workgroups a CU hold their tables in its LDS; a multiple of the 8 XCDs
                    const unsigned grid = (unsigned)std::min<int64_t>(nu, (int64_t)std::max(ctx->cus, 8) / 8 * 8 * 2);
                    cross_join_kernel<<<grid, NTX, 0, st>>>(q->codes.as<uint64_t>(), qseg.as<int64_t>(),
                                                            s->codes.as<uint64_t>(), s->segoff.as<int64_t>(), nseg,
                                                            dunits.as<int4>(), nu, nb, k0, k1, blk.as<int32_t>(), nk);
                    GD_HIP(hipGetLastError());
                }
                if (timed) GD_HIP(hipEventRecord(ev[1], st));
                after(b0, nb, k0, nk, k1 == c1 ? 1 : 0);
                if (timed) {
                    GD_HIP(hipEventRecord(ev[2], st));
                    GD_HIP(hipEventSynchronize(ev[2]));
                    float j = 0, sl = 0;
                    GD_HIP(hipEventElapsedTime(&j, ev[0], ev[1]));
                    GD_HIP(hipEventElapsedTime(&sl, ev[1], ev[2]));
                    join_ms += j;
                    select_ms += sl;
                }
                out(b0, nb, k0, nk, k1 == c1 ? 1 : 0);
                nunits += nu;
            }
        }
    }

    // a consumer kernel that can only be queued from `out` (it needs what the
    // step downloaded): its time joins select_ms
    template <class F>
    void timed_select(F&& f) {
        hipStream_t st = ctx->stream;
        if (timed) GD_HIP(hipEventRecord(ev[1], st));
        f();
        if (timed) {
            GD_HIP(hipEventRecord(ev[2], st));
            GD_HIP(hipEventSynchronize(ev[2]));
            float sl = 0;
            GD_HIP(hipEventElapsedTime(&sl, ev[1], ev[2]));
            select_ms += sl;
        }
    }

    void report() {
        ctx->cross_units = nunits;
        if (timed) {
            ctx->cross_join_ms = join_ms;
            ctx->cross_select_ms = select_ms;
        }
    }
};

}  // namespace

static_assert(sizeof(CrossUnit) == sizeof(int4), "units are uploaded as 16-byte records");

// every argument checked by the caller, the subjects' segment index built;
// I_out / D_out: host, row stride ld, either may be null
void cross_matrix(gdist_ctx* ctx, const gdist_sets* q, const gdist_sets* s, int64_t q0, int64_t q1, int64_t c0,
                  int64_t c1, unsigned flags, int32_t* I_out, double* D_out, int64_t ld) {
    hipStream_t st = ctx->stream;
    const int empty_nan = (flags & GDIST_EMPTY_NAN) ? 1 : 0;
    int64_t R, W;
    closest_blocks(ctx, q1 - q0, c1 - c0, 12, &R, &W);   // a step's I and D
    CrossWalk walk(ctx, q, s, R, W);
    DevBuf dD;
    if (D_out) dD.alloc((size_t)R * W * 8 + 8, st);
    std::vector<int32_t> hI;
    std::vector<double> hD;
    walk.run(q0, q1, c0, c1, [&](int64_t b0, int64_t nb, int64_t k0, int64_t nk, int) {
        if (!D_out) return;
        const size_t cells = (size_t)nb * nk;
        const unsigned grid = (unsigned)std::min<int64_t>(ceil_div((int64_t)cells, 256), (int64_t)ctx->cus * 16);
        cross_epilogue_kernel<<<grid, 256, 0, st>>>(q->off.as<int64_t>(), s->off.as<int64_t>(), b0, nb, k0, nk, empty_nan,
                                                    walk.blk.as<int32_t>(), dD.as<double>());
        GD_HIP(hipGetLastError());
    }, [&](int64_t b0, int64_t nb, int64_t k0, int64_t nk, int) {
        const size_t cells = (size_t)nb * nk;
        if (D_out) {
            hD.resize(cells);
            d2h(hD.data(), dD.p, cells * 8, st);
            for (int64_t a = 0; a < nb; a++)
                std::memcpy(D_out + (b0 - q0 + a) * ld + (k0 - c0), hD.data() + (size_t)a * nk, (size_t)nk * 8);
        }
        if (I_out) {
            hI.resize(cells);
            d2h(hI.data(), walk.blk.p, cells * 4, st);
            for (int64_t a = 0; a < nb; a++)
                std::memcpy(I_out + (b0 - q0 + a) * ld + (k0 - c0), hI.data() + (size_t)a * nk, (size_t)nk * 4);
        }
    });
    walk.report();
}

// as cross_matrix; n >= 1, a non-empty rectangle. The counts stay on the
// device and D is never written: the select folds each step's counts into the
// rows' lists (closest.hip)
void cross_closest(gdist_ctx* ctx, const gdist_sets* q, const gdist_sets* s, int64_t q0, int64_t q1, int64_t c0,
                   int64_t c1, unsigned flags, int n, double max_dist, int64_t* idx_out, double* d_out,
                   int32_t* count_out) {
    hipStream_t st = ctx->stream;
    const int empty_nan = (flags & GDIST_EMPTY_NAN) ? 1 : 0;
    int L = 128;
    while (L < n) L <<= 1;
    int64_t R, W;
    closest_blocks(ctx, q1 - q0, c1 - c0, 4, &R, &W);
    CrossWalk walk(ctx, q, s, R, W);
    DevBuf sd((size_t)R * L * 8 + 8, st), sc((size_t)R * L * 4 + 4, st), sn((size_t)R * 4 + 4, st);
    DevBuf oi((size_t)R * n * 8 + 8, st), od((size_t)R * n * 8 + 8, st), oc((size_t)R * 4 + 4, st);
    walk.run(q0, q1, c0, c1, [&](int64_t b0, int64_t nb, int64_t k0, int64_t nk, int last) {
        if (k0 == c0) GD_HIP(hipMemsetAsync(sn.p, 0, (size_t)nb * 4, st));
        closest_select_counts(ctx, walk.blk.as<int32_t>(), nk, q->off.as<int64_t>(), s->off.as<int64_t>(), empty_nan, b0,
                              nb, k0, nk, n, L, max_dist, sd.as<unsigned long long>(), sc.as<uint32_t>(),
                              sn.as<int32_t>(), last, oi.as<int64_t>(), od.as<double>(), oc.as<int32_t>());
    }, [&](int64_t b0, int64_t nb, int64_t, int64_t, int last) {
        if (last) {
            d2h(idx_out + (b0 - q0) * n, oi.p, (size_t)nb * n * 8, st);
            d2h(d_out + (b0 - q0) * n, od.p, (size_t)nb * n * 8, st);
            d2h(count_out + (b0 - q0), oc.p, (size_t)nb * 4, st);
        }
    });
    walk.report();
}

// as cross_matrix; a non-empty rectangle. A row needs its full column width
// before it can be compacted in (row, column) order: the walk is by row blocks
// of within()'s sizing over all of [c0, c1), one step a block, and the steps
// arrive in row order
void cross_within(gdist_ctx* ctx, const gdist_sets* q, const gdist_sets* s, int64_t q0, int64_t q1, int64_t c0,
                  int64_t c1, unsigned flags, double max_dist, int64_t capacity, int64_t* rowptr, int64_t* col_out,
                  double* d_out) {
    hipStream_t st = ctx->stream;
    const int empty_nan = (flags & GDIST_EMPTY_NAN) ? 1 : 0;
    const int64_t nc = c1 - c0;
    const int64_t R = within_rows(ctx, q1 - q0, nc, 4);
    CrossWalk walk(ctx, q, s, R, nc);
    const int64_t max_tiles = within_tiles(R, nc);
    DevBuf tcount((size_t)(max_tiles + 1) * 4, st), tbase((size_t)(max_tiles + 1) * 8, st);
    DevBuf rbase((size_t)(R + 1) * 8, st), scan_tmp;
    std::vector<int64_t> hbase((size_t)R + 1);
    int64_t total = 0;   // pairs of the rows before this step
    rowptr[0] = 0;
    walk.run(q0, q1, c0, c1, [&](int64_t b0, int64_t nb, int64_t k0, int64_t nk, int) {
        within_count_counts(ctx, walk.blk.as<int32_t>(), nk, q->off.as<int64_t>(), s->off.as<int64_t>(), empty_nan, b0,
                            nb, k0, nk, max_dist, tcount.as<int32_t>(), tbase.as<int64_t>(), rbase.as<int64_t>(),
                            scan_tmp);
    }, [&](int64_t b0, int64_t nb, int64_t k0, int64_t nk, int) {
        d2h(hbase.data(), rbase.p, (size_t)(nb + 1) * 8, st);
        int64_t* rp = rowptr + (b0 - q0);
        for (int64_t a = 0; a <= nb; a++) rp[a] = total + hbase[a];
        const int64_t step = hbase[nb];
        const int64_t fit = std::min(step, std::max<int64_t>(capacity - total, 0));
        if (fit > 0) {
            DevBuf sc((size_t)fit * 8, st), sd((size_t)fit * 8, st);
            walk.timed_select([&] {
                within_write_counts(ctx, walk.blk.as<int32_t>(), nk, q->off.as<int64_t>(), s->off.as<int64_t>(),
                                    empty_nan, b0, nb, k0, nk, max_dist, tbase.as<int64_t>(), fit, sc.as<int64_t>(),
                                    sd.as<double>());
            });
            d2h(col_out + total, sc.p, (size_t)fit * 8, st);
            d2h(d_out + total, sd.p, (size_t)fit * 8, st);
        }
        total += step;
    });
    walk.report();
}

// as cross_matrix, any rectangle (an empty one: the n == 0 form). Each step's
// counts are folded into the call's accumulators, as group_stats() folds them
void cross_group_stats(gdist_ctx* ctx, const gdist_sets* q, const gdist_sets* s, int64_t q0, int64_t q1, int64_t c0,
                       int64_t c1, unsigned flags, int ntypes, const int32_t* qlabels, const int32_t* slabels,
                       gdist_group_side* out, int64_t* bad) {
    hipStream_t st = ctx->stream;
    const int empty_nan = (flags & GDIST_EMPTY_NAN) ? 1 : 0;
    const size_t nslots = group_slots(ntypes);
    std::vector<unsigned long long> h(nslots, 0ull);
    if (q1 > q0 && c1 > c0) {
        int64_t R, W;
        closest_blocks(ctx, q1 - q0, c1 - c0, 4, &R, &W);
        CrossWalk walk(ctx, q, s, R, W);
        DevBuf qlab((size_t)ntypes * q->nsets * 4, st), slab((size_t)ntypes * s->nsets * 4, st), acc(nslots * 8, st);
        h2d(qlab.p, qlabels, (size_t)ntypes * q->nsets * 4, st);
        h2d(slab.p, slabels, (size_t)ntypes * s->nsets * 4, st);
        GD_HIP(hipMemsetAsync(acc.p, 0, nslots * 8, st));
        walk.run(q0, q1, c0, c1, [&](int64_t b0, int64_t nb, int64_t k0, int64_t nk, int) {
            group_reduce_counts(ctx, walk.blk.as<int32_t>(), nk, q->off.as<int64_t>(), s->off.as<int64_t>(), empty_nan,
                                b0, nb, k0, nk, ntypes, qlab.as<int32_t>(), q->nsets, slab.as<int32_t>(), s->nsets,
                                acc.as<unsigned long long>());
        }, [](int64_t, int64_t, int64_t, int64_t, int) {});
        d2h(h.data(), acc.p, nslots * 8, st);
        walk.report();
    }
    group_finish(h.data(), ntypes, out, bad);
}

// as cross_group_stats with the bucket counts of histogram()
void cross_histogram(gdist_ctx* ctx, const gdist_sets* q, const gdist_sets* s, int64_t q0, int64_t q1, int64_t c0,
                     int64_t c1, unsigned flags, int nedges, const double* edges, int ntypes, const int32_t* qlabels,
                     const int32_t* slabels, int64_t* counts, int64_t* nans, int64_t* bad) {
    hipStream_t st = ctx->stream;
    const int empty_nan = (flags & GDIST_EMPTY_NAN) ? 1 : 0;
    const size_t nslots = hist_slots(nedges, ntypes);
    std::vector<unsigned long long> h(nslots, 0ull);
    if (q1 > q0 && c1 > c0) {
        int64_t R, W;
        closest_blocks(ctx, q1 - q0, c1 - c0, 4, &R, &W);
        CrossWalk walk(ctx, q, s, R, W);
        DevBuf qlab((size_t)ntypes * q->nsets * 4, st), slab((size_t)ntypes * s->nsets * 4, st);
        DevBuf edg((size_t)nedges * 8, st), acc(nslots * 8, st);
        h2d(qlab.p, qlabels, (size_t)ntypes * q->nsets * 4, st);
        h2d(slab.p, slabels, (size_t)ntypes * s->nsets * 4, st);
        h2d(edg.p, edges, (size_t)nedges * 8, st);
        GD_HIP(hipMemsetAsync(acc.p, 0, nslots * 8, st));
        walk.run(q0, q1, c0, c1, [&](int64_t b0, int64_t nb, int64_t k0, int64_t nk, int) {
            hist_counts(ctx, walk.blk.as<int32_t>(), nk, q->off.as<int64_t>(), s->off.as<int64_t>(), empty_nan, b0, nb,
                        k0, nk, ntypes, qlab.as<int32_t>(), q->nsets, slab.as<int32_t>(), s->nsets, edg.as<double>(),
                        nedges, acc.as<unsigned long long>());
        }, [](int64_t, int64_t, int64_t, int64_t, int) {});
        d2h(h.data(), acc.p, nslots * 8, st);
        walk.report();
    }
    hist_finish(h.data(), nedges, ntypes, counts, nans, bad);
}

}  // namespace gdist
