// rare.hip — the rare tier in a step: the kmers held by 2 .. T - 1 sets, kept
// as posting lists (bitset_build.hip build_postings), added to |A∩B|.
//
// The rare tier's share of the SequenceKmers.distance(other) loop over many
// pairs (FastaDistanceProcessor.java:177-186, GenomeProcessor.java:140,
// WidthProcessor.java:159-165): a kmer held by m sets adds 1 (its list's
// weight, identical lists merged) to each of its m(m-1)/2 pairs instead of
// costing a bit column over all N^2/2 pairs.
//
// Three walks and their host launchers. List-major (rare_pairs_kernel): a lane
// per list, its pairs in the region added with global atomics. Row-major
// (rare_rows_kernel: LDS counters per chunk of RCH columns;
// rare_rows_direct_kernel: every record once, global atomics): a workgroup
// per row of the block over the set -> list CSR. The row query
// (rare_query_kernel + gather_add_kernel): one set against all. Which walk a
// step takes, on which stream and behind which event, is bitset_matrix's
// (matrix_step.hip); rare_tier() is what its cost model reads.
#include <algorithm>

#include "gdist_internal.hpp"

namespace gdist {
namespace {

// Lists of kLongList+ sets (gdist_internal.hpp) are walked by a whole wave
// (lanes stride the members) instead of one lane: a lane-serial walk of an
// m-member list is an O(m) (row-major) or O(m^2) (list-major) tail the rest
// of the wave idles on.

// pairs (s = psets[x], t = psets[y]) for y in [y0, e) step dy, s < t
__device__ __forceinline__ void rare_pair_walk(const uint32_t* __restrict__ psets, int64_t x, int64_t y0, int64_t e,
                                               int dy, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int upper,
                                               int32_t w, int32_t* __restrict__ I, int64_t ldI) {
    const int64_t s = psets[x];
    const bool srow = s >= r0 && s < r1, scol = s >= c0 && s < c1;
    if (!srow && (upper || !scol)) return;
    for (int64_t y = y0; y < e; y += dy) {
        const int64_t t = psets[y];                  // t > s
        if (srow && t >= c0 && t < c1) atomicAdd(I + (s - r0) * ldI + (t - c0), w);
        if (!upper && scol && t >= r0 && t < r1) atomicAdd(I + (t - r0) * ldI + (s - c0), w);
    }
}

// Rare tier: every posting list (ascending set ids) adds its weight (the
// number of kmers sharing it) to each of its m(m-1)/2 pairs that fall in the
// region. One lane per list; lists of kLongList+ members are taken by the
// wave (trip counts are wave-uniform).
__global__ __launch_bounds__(256) void rare_pairs_kernel(const int64_t* __restrict__ poff,
                                                         const uint32_t* __restrict__ psets,
                                                         const uint32_t* __restrict__ pw, int64_t nposts,
                                                         int64_t r0, int64_t r1, int64_t c0, int64_t c1, int upper,
                                                         int32_t* __restrict__ I, int64_t ldI) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (int64_t pb = (int64_t)blockIdx.x * blockDim.x; pb < nposts; pb += stride) {
        const int64_t p = pb + threadIdx.x;
        int64_t b = 0, e = 0;
        int32_t w = 0;
        if (p < nposts) { b = poff[p]; e = poff[p + 1]; w = (int32_t)pw[p]; }
        const bool lng = e - b >= kLongList;
        for (unsigned long long m = __ballot(lng); m; m &= m - 1) {
            const int l = __ffsll((long long)m) - 1;
            const int64_t lb = __shfl((long long)b, l, 64), le = __shfl((long long)e, l, 64);
            const int32_t lw = __shfl(w, l, 64);
            for (int64_t x = lb; x < le - 1; x++)
                rare_pair_walk(psets, x, x + 1 + lane, le, 64, r0, r1, c0, c1, upper, lw, I, ldI);
        }
        if (!lng)
            for (int64_t x = b; x < e - 1; x++)
                rare_pair_walk(psets, x, x + 1, e, 1, r0, r1, c0, c1, upper, w, I, ldI);
    }
}

// Rare tier, row-major: one workgroup per (row set i, chunk of RCH columns).
// The row's rare kmers (set -> rare CSR) are walked by the threads; each
// member j of their posting lists adds 1 to an LDS counter; the counters are
// then added to I's row once, coalesced. No global atomics, and each (i, j)
// is owned by exactly one workgroup (the dense kernel ran before, in stream
// order).
constexpr int RCH = 16384;   // max columns per LDS chunk (64 KiB of counters)

// grid = nr rows x nch column chunks x nsplit slices of the row's rare kmers;
// counters live in dynamic LDS sized to the chunk. With nsplit > 1 several
// workgroups share a row chunk and flush with global atomics.
// Member = uint32 (post_sets) or uint16 (post_sets16, collections of at most
// 65,536 sets): the walk's scattered list reads are whole lines from HBM or
// the Infinity Cache, and 2-byte members halve the lines a list spans and
// let C3's lists (72 M members: 287 MB as uint32) sit in the 256 MiB cache.
// NT threads a workgroup (option rare_rows_threads: 512 default, 256): the
// walk is latency-bound (each record's members are a dependent load after its
// record's), and the 40 KiB of counters of a C3 row allow 4 workgroups a CU:
// 512 threads make that the full 32 waves a CU instead of 16
// C16 (round 5): 16-bit counters, two to an LDS dword, when no row's rare
// kmers weigh 65,536 or more (rare_row_wmax, build time: a count never
// carries into its neighbour) — C3's 10,000 columns take 20 KiB instead of
// 40, so a workgroup fits on a CU beside an MFMA dense-tile workgroup.
template <typename M, int NT, bool C16 = false>
__global__ __launch_bounds__(NT) void rare_rows_kernel(const int64_t* __restrict__ soff,
                                                        const uint64_t* __restrict__ sent,
                                                        const uint32_t* __restrict__ sw,
                                                        const uint16_t* __restrict__ sskip,
                                                        const M* __restrict__ psets, int64_t r0, int64_t r1,
                                                        int64_t c0, int64_t c1, int nch, int nsplit, int upper,
                                                        int atomic_flush, int32_t* __restrict__ I, int64_t ldI) {
    constexpr int PER = 16 / (int)sizeof(M);     // members per 16-byte load
    extern __shared__ int32_t cnt[];
    const int64_t unit = blockIdx.x / nsplit;
    const int split = blockIdx.x % nsplit;
    const int64_t i = r0 + unit / nch;
    const int ch = (int)(unit % nch);
    const int64_t cb = c0 + (int64_t)ch * RCH;
    const int64_t ce = cb + RCH < c1 ? cb + RCH : c1;
    if (i >= r1 || cb >= ce || (upper && ce - 1 <= i)) return;
    const int n = (int)(ce - cb);
    const int nw = C16 ? (n + 1) >> 1 : n;
    for (int t = threadIdx.x; t < nw; t += blockDim.x) cnt[t] = 0;
    __syncthreads();
    auto add = [&](int64_t t, int32_t v) {
        if (C16) atomicAdd(&cnt[(t - cb) >> 1], v << (((t - cb) & 1) << 4));
        else atomicAdd(&cnt[t - cb], v);
    };
    const int64_t lo = upper && i + 1 > cb ? i + 1 : cb;
    const int64_t rb = soff[i], re = soff[i + 1];
    const int64_t per = (re - rb + nsplit - 1) / nsplit;
    const int64_t xb = rb + per * split;
    const int64_t xe = xb + per < re ? xb + per : re;
    const int lane = threadIdx.x & 63;
    for (int64_t xbase = xb; xbase < xe; xbase += blockDim.x) {   // wave-uniform trip count
        const int64_t x = xbase + threadIdx.x;
        const uint64_t ent = x < xe ? sent[x] : 0ull;  // coalesced: no random bounds lookup
        const int32_t w = x < xe ? (int32_t)sw[x] : 0;
        const int64_t b0 = (int64_t)(ent >> 24), e = b0 + (int64_t)(ent & 0xFFFFFFu);
        // upper triangle: only the members after the row's own set (ascending lists)
        const int64_t b = upper && x < xe ? b0 + sskip[x] : b0;
        const bool lng = e - b >= kLongList;
        for (unsigned long long m = __ballot(lng); m; m &= m - 1) {   // long lists: the wave walks them
            const int l = __ffsll((long long)m) - 1;
            const int64_t lb = __shfl((long long)b, l, 64), le = __shfl((long long)e, l, 64);
            const int32_t lw = __shfl(w, l, 64);
            for (int64_t y = lb + lane; y < le; y += 64) {
                const int64_t t = psets[y];
                if (t >= lo && t < ce && t != i) add(t, lw);
            }
        }
        if (lng) continue;
        // PER members per 16-byte load (global_load_dwordx4 when the list
        // start is dword-aligned; post_sets / post_sets16 are padded past the
        // last list)
#pragma unroll 2
        for (int64_t y = b; y < e; y += PER) {
            M mem[PER];
            __builtin_memcpy(mem, psets + y, 16);
#pragma unroll
            for (int u = 0; u < PER; u++) {
                const int64_t t = mem[u];
                if (y + u < e && t >= lo && t < ce && t != i) add(t, w);
            }
        }
    }
    __syncthreads();
    int32_t* row = I + (i - r0) * ldI + (cb - c0);
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        const int v = C16 ? (int)(((uint32_t)cnt[t >> 1] >> ((t & 1) << 4)) & 0xFFFFu) : cnt[t];
        if (v && cb + t >= lo) {
            if (nsplit > 1 || atomic_flush) atomicAdd(row + t, v);
            else row[t] += v;
        }
    }
}

// Rare tier, row-major over a wide column range (round 5; C4's 100,000
// columns would need 7 LDS chunks, and rare_rows_kernel walks every list of
// the row once PER CHUNK, filtering its members to the chunk: 10.2 ms on the
// C4 slice for 0.9 GB of algorithmic bytes). Here each (set, list) record of
// the row is walked ONCE and every member in [lo, c1) adds the list's weight
// straight into I's row with a device-scope atomic (the dense tiles and the
// variant walk beside it add atomically too). A thread takes one record
// (16-byte member loads, as rare_rows_kernel); long lists go to the whole
// wave. Grid: rows x nsplit slices of the row's records.
template <typename M>
__global__ __launch_bounds__(256) void rare_rows_direct_kernel(const int64_t* __restrict__ soff,
                                                               const uint64_t* __restrict__ sent,
                                                               const uint32_t* __restrict__ sw,
                                                               const uint16_t* __restrict__ sskip,
                                                               const M* __restrict__ psets, int64_t r0, int64_t r1,
                                                               int64_t c0, int64_t c1, int nsplit, int upper,
                                                               int32_t* __restrict__ I, int64_t ldI) {
    constexpr int PER = 16 / (int)sizeof(M);
    const int64_t i = r0 + blockIdx.x / nsplit;
    const int split = blockIdx.x % nsplit;
    if (i >= r1) return;
    const int64_t lo = upper && i + 1 > c0 ? i + 1 : c0;
    if (lo >= c1) return;
    int32_t* row = I + (i - r0) * ldI - c0;                 // row[t] for column t
    const int64_t rb = soff[i], re = soff[i + 1];
    const int64_t per = (re - rb + nsplit - 1) / nsplit;
    const int64_t xb = rb + per * split;
    const int64_t xe = xb + per < re ? xb + per : re;
    const int lane = threadIdx.x & 63;
    for (int64_t xbase = xb; xbase < xe; xbase += blockDim.x) {   // wave-uniform trip count
        const int64_t x = xbase + threadIdx.x;
        const uint64_t ent = x < xe ? sent[x] : 0ull;
        const int32_t w = x < xe ? (int32_t)sw[x] : 0;
        const int64_t b0 = (int64_t)(ent >> 24), e = b0 + (int64_t)(ent & 0xFFFFFFu);
        const int64_t b = upper && x < xe ? b0 + sskip[x] : b0;
        const bool lng = e - b >= kLongList;
        for (unsigned long long m = __ballot(lng); m; m &= m - 1) {
            const int l = __ffsll((long long)m) - 1;
            const int64_t lb = __shfl((long long)b, l, 64), le = __shfl((long long)e, l, 64);
            const int32_t lw = __shfl(w, l, 64);
            for (int64_t y = lb + lane; y < le; y += 64) {
                const int64_t t = psets[y];
                if (t >= lo && t < c1 && t != i) atomicAdd(row + t, lw);
            }
        }
        if (lng) continue;
#pragma unroll 2
        for (int64_t y = b; y < e; y += PER) {
            M mem[PER];
            __builtin_memcpy(mem, psets + y, 16);
#pragma unroll
            for (int u = 0; u < PER; u++) {
                const int64_t t = mem[u];
                if (y + u < e && t >= lo && t < c1 && t != i) atomicAdd(row + t, w);
            }
        }
    }
}

// Rare tier of one query set q: cnt[t] += shared rare kmers of q and t
// (global atomics, one row's worth); gather_add adds cnt[cols[c]] to I[c]
// for every requested column position (duplicates included).
__global__ __launch_bounds__(256) void rare_query_kernel(const int64_t* __restrict__ soff,
                                                         const uint64_t* __restrict__ sent,
                                                         const uint32_t* __restrict__ sw,
                                                         const uint32_t* __restrict__ psets, int64_t q,
                                                         int32_t* __restrict__ cnt) {
    const int64_t xb = soff[q], xe = soff[q + 1];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (int64_t xbase = xb + (int64_t)blockIdx.x * blockDim.x; xbase < xe; xbase += stride) {
        const int64_t x = xbase + threadIdx.x;
        const uint64_t ent = x < xe ? sent[x] : 0ull;
        const int32_t w = x < xe ? (int32_t)sw[x] : 0;
        const int64_t b = (int64_t)(ent >> 24), e = b + (int64_t)(ent & 0xFFFFFFu);
        const bool lng = e - b >= kLongList;
        for (unsigned long long m = __ballot(lng); m; m &= m - 1) {
            const int l = __ffsll((long long)m) - 1;
            const int64_t lb = __shfl((long long)b, l, 64), le = __shfl((long long)e, l, 64);
            const int32_t lw = __shfl(w, l, 64);
            for (int64_t y = lb + lane; y < le; y += 64) {
                const int64_t t = psets[y];
                if (t != q) atomicAdd(cnt + t, lw);
            }
        }
        if (lng) continue;
        for (int64_t y = b; y < e; y++) {
            const int64_t t = psets[y];
            if (t != q) atomicAdd(cnt + t, w);
        }
    }
}

__global__ void gather_add_kernel(const int64_t* __restrict__ cols, int64_t ncols, const int32_t* __restrict__ cnt,
                                  int32_t* __restrict__ I) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < ncols) I[c] += cnt[cols[c]];
}

}  // namespace

RareTier rare_tier(const gdist_sets* s) {
    RareTier t;
    t.incs = (double)s->rare_incs;
    t.incs_long = (double)s->rare_incs_long;
    t.records = (double)s->rare_records;
    t.lists = (double)s->n_rare;
    return t;
}

void rare_pairs_launch(gdist_ctx* ctx, const gdist_sets* s, const Region& g, int32_t* d_I, int64_t ldI, hipStream_t rs) {
    FamilyTimer ft(ctx, GDIST_KERNEL_RARE, rs);
    rare_pairs_kernel<<<grid_for(s->n_rare, 256, 256 * 64), 256, 0, rs>>>(
        s->post_off.as<int64_t>(), s->post_sets.as<uint32_t>(), s->post_w.as<uint32_t>(), s->n_rare, g.r0, g.r1, g.c0,
        g.c1, g.upper ? 1 : 0, d_I, ldI);
    ft.end();
}

void rare_rows_launch(gdist_ctx* ctx, const gdist_sets* s, const Region& g, int32_t* d_I, int64_t ldI, hipStream_t rs,
                      bool atomic_flush) {
    const int64_t r0 = g.r0, r1 = g.r1, c0 = g.c0, c1 = g.c1, nr = r1 - r0, nc = c1 - c0;
    const bool upper = g.upper;
    const int nch = (int)ceil_div(nc, RCH);
    // past one LDS chunk of columns every record once, members added to I
    // by atomics (option rare_direct; the LDS kernel re-walks the row's
    // lists once per chunk)
    if (ctx->option(OPT_RARE_DIRECT, nch > 1 ? 1 : 0) != 0) {
        const int dsplit = (int)std::max<int64_t>(1, std::min<int64_t>(64, ceil_div((int64_t)ctx->cus * 8, nr)));
        const int64_t dgrid = nr * dsplit;
        GD_REQUIRE(dgrid < (int64_t(1) << 31), "rare-tier grid too large");
        FamilyTimer ft(ctx, GDIST_KERNEL_RARE, rs);
        if (s->post_sets16.p)
            rare_rows_direct_kernel<uint16_t><<<(unsigned)dgrid, 256, 0, rs>>>(
                s->srare_off.as<int64_t>(), s->srare_ent.as<uint64_t>(), s->srare_w.as<uint32_t>(),
                s->srare_skip.as<uint16_t>(), s->post_sets16.as<uint16_t>(), r0, r1, c0, c1, dsplit,
                upper ? 1 : 0, d_I, ldI);
        else
            rare_rows_direct_kernel<uint32_t><<<(unsigned)dgrid, 256, 0, rs>>>(
                s->srare_off.as<int64_t>(), s->srare_ent.as<uint64_t>(), s->srare_w.as<uint32_t>(),
                s->srare_skip.as<uint16_t>(), s->post_sets.as<uint32_t>(), r0, r1, c0, c1, dsplit,
                upper ? 1 : 0, d_I, ldI);
        GD_HIP(hipGetLastError());
        ft.end();
        return;
    }
    const int64_t units = nr * nch;
    // few rows (C2: 1000): slice each row's rare kmers over several workgroups
    const int nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(16, ceil_div((int64_t)ctx->cus * 8, units)));
    const int64_t rgrid = units * nsplit;
    GD_REQUIRE(rgrid < (int64_t(1) << 31), "rare-tier grid too large");
    // 16-bit counters when no row can reach 2^16 (option rare_c16, default on)
    const bool c16 = s->rare_row_wmax < 65536 && ctx->option(OPT_RARE_C16, 1) != 0;
    const size_t lds = c16 ? (size_t)((std::min<int64_t>(nc, RCH) + 1) / 2) * 4 : (size_t)std::min<int64_t>(nc, RCH) * 4;
    FamilyTimer ft(ctx, GDIST_KERNEL_RARE, rs);
    // threads a workgroup: the LDS counters allow 4 workgroups a CU up to
    // 40 KiB (10,240 columns: C3), 2 beyond (C4's 64 KiB chunks); 32 waves
    // a CU either way (option rare_rows_threads 256 / 512 / 1024)
    const int64_t nt_opt = ctx->option(OPT_RARE_ROWS_THREADS, lds > 40 * 1024 ? 1024 : 512);
    const int rt = nt_opt == 256 ? 256 : nt_opt == 1024 ? 1024 : 512;
    auto go = [&](auto kern, int nt, auto* members) {
        kern<<<(unsigned)rgrid, nt, lds, rs>>>(s->srare_off.as<int64_t>(), s->srare_ent.as<uint64_t>(),
                                               s->srare_w.as<uint32_t>(), s->srare_skip.as<uint16_t>(), members,
                                               r0, r1, c0, c1, nch, nsplit, upper ? 1 : 0, atomic_flush ? 1 : 0,
                                               d_I, ldI);
    };
    if (s->post_sets16.p && c16) {
        if (rt == 1024) go(rare_rows_kernel<uint16_t, 1024, true>, 1024, s->post_sets16.as<uint16_t>());
        else if (rt == 512) go(rare_rows_kernel<uint16_t, 512, true>, 512, s->post_sets16.as<uint16_t>());
        else go(rare_rows_kernel<uint16_t, 256, true>, 256, s->post_sets16.as<uint16_t>());
    } else if (s->post_sets16.p) {
        if (rt == 1024) go(rare_rows_kernel<uint16_t, 1024>, 1024, s->post_sets16.as<uint16_t>());
        else if (rt == 512) go(rare_rows_kernel<uint16_t, 512>, 512, s->post_sets16.as<uint16_t>());
        else go(rare_rows_kernel<uint16_t, 256>, 256, s->post_sets16.as<uint16_t>());
    } else {
        if (rt == 1024) go(rare_rows_kernel<uint32_t, 1024>, 1024, s->post_sets.as<uint32_t>());
        else if (rt == 512) go(rare_rows_kernel<uint32_t, 512>, 512, s->post_sets.as<uint32_t>());
        else go(rare_rows_kernel<uint32_t, 256>, 256, s->post_sets.as<uint32_t>());
    }
    ft.end();
}

void rare_query_launch(gdist_ctx* ctx, const gdist_sets* s, int64_t q, int32_t* cnt) {
    rare_query_kernel<<<256, 256, 0, ctx->stream>>>(s->srare_off.as<int64_t>(), s->srare_ent.as<uint64_t>(),
                                                    s->srare_w.as<uint32_t>(), s->post_sets.as<uint32_t>(), q, cnt);
}

void gather_add_launch(gdist_ctx* ctx, const int64_t* d_cols, int64_t ncols, const int32_t* cnt, int32_t* d_I) {
    gather_add_kernel<<<(unsigned)ceil_div(ncols, 256), 256, 0, ctx->stream>>>(d_cols, ncols, cnt, d_I);
}

}  // namespace gdist
