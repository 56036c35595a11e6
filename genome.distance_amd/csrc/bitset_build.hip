// bitset_build.hip — builds the two-tier representation the steps read: the
// dictionary, the dictionary-rank bitsets and the rare tier's posting lists.
//
// What SequenceKmers keeps per sequence as a hash set of kmers (the sets that
// FastaDistanceProcessor.java:177-186 intersects pair by pair) becomes one
// structure per collection. Dictionary: all codes of all sets, sorted; a run
// of equal codes is one entry with the number of sets holding it (a Summary;
// summaries of disjoint set ranges merge by summing counts). Kmers held by
// one set can never contribute to an intersection, so by default they are
// left out (|A| still counts them: it comes from the CSR sizes; the result is
// exact either way, tests check both). Codes held by >= T sets are the dense
// tier, one bit column each (rows filled by bitset_fill.hip); codes held by
// 2 .. T - 1 sets are the rare tier, one posting list each, identical lists
// merged (build_postings). T is the cost model's (choose_rare_threshold).
// build_bitsets runs the whole build and hands over to variant.hip /
// sparse.hip where their tiers apply; free_bitsets drops every tier.
#include <cstring>

#include <algorithm>

#include "gdist_internal.hpp"
#include "bitset_tiles.hpp"

namespace gdist {
namespace {

__global__ void head_flags_u64(const uint64_t* __restrict__ keys, int64_t n, int32_t* __restrict__ flag) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// run heads -> unique code and run start
__global__ void run_heads_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ flag,
                                 const int64_t* __restrict__ pos, int64_t n, uint64_t* __restrict__ uniq,
                                 int64_t* __restrict__ start) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (flag[i]) { uniq[pos[i]] = keys[i]; start[pos[i]] = i; }
}

// total weight per run: weights given (prefix sums cw over elements) or 1 per element
__global__ void run_totals_kernel(const int64_t* __restrict__ start, int64_t nruns, int64_t n,
                                  const int64_t* __restrict__ cw, uint32_t* __restrict__ total) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nruns) return;
    const int64_t b = start[r], e = (r + 1 < nruns) ? start[r + 1] : n;
    const int64_t t = cw ? (cw[e] - cw[b]) : (e - b);
    total[r] = (uint32_t)(t > 0xFFFFFFFFll ? 0xFFFFFFFFll : t);
}


__global__ void compact_u64_kernel(const uint64_t* __restrict__ v, const int32_t* __restrict__ flag,
                                   const int64_t* __restrict__ pos, int64_t n, uint64_t* __restrict__ out) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (flag[i]) out[pos[i]] = v[i];
}

__global__ void compact_u32_kernel(const uint32_t* __restrict__ v, const int32_t* __restrict__ flag,
                                   const int64_t* __restrict__ pos, int64_t n, uint32_t* __restrict__ out) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (flag[i]) out[pos[i]] = v[i];
}

__global__ void widen_u32_kernel(const uint32_t* __restrict__ in, int64_t n, int64_t* __restrict__ out) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = in[i];
}

// posting offsets: first record of each rare rank
__global__ void posting_offsets_kernel(const uint64_t* __restrict__ recs, int64_t n, int64_t nposts,
                                       int64_t* __restrict__ off) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > nposts) return;
    const uint64_t v = (uint64_t)p << 32;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (recs[mid] < v) lo = mid + 1; else hi = mid;
    }
    off[p] = lo;
}

__global__ void posting_sets_kernel(const uint64_t* __restrict__ recs, int64_t n, uint32_t* __restrict__ sets) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) sets[i] = (uint32_t)recs[i];
}

// set-side entries: rare rank -> (list start << 24 | list length)
__global__ void rare_entries_kernel(const uint64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ poff,
                                    uint64_t* __restrict__ ent) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t r = (uint32_t)keys[i];
        const int64_t b = poff[r];
        ent[i] = ((uint64_t)b << 24) | (uint64_t)(poff[r + 1] - b);
    }
}

// per (set, list) record: one past the set's position in its list (the
// members an upper-triangle row walk starts at; lists are ascending), 0
// past 65534 members (the walk then starts at the list's first member)
__global__ void rare_skip_kernel(const uint64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ poff,
                                 const uint32_t* __restrict__ psets, uint16_t* __restrict__ skip) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t set = (uint32_t)(keys[i] >> 32), r = (uint32_t)keys[i];
        int64_t lo = poff[r], hi = poff[r + 1];
        const int64_t b = lo;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (psets[mid] < set) lo = mid + 1; else hi = mid;
        }
        const int64_t k = lo - b + 1;
        skip[i] = k < 65535 ? (uint16_t)k : (uint16_t)0;
    }
}

// set -> rare CSR: records (rare << 32 | set) become (set << 32 | rare)
__global__ void swap_halves_kernel(const uint64_t* __restrict__ in, int64_t n, uint64_t* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = (in[i] << 32) | (in[i] >> 32);
}

// rare-tier mass: count of records each rare dictionary entry will produce
__global__ void rare_flag_kernel(const uint32_t* __restrict__ cnt, int64_t n, int64_t T, int keep,
                                 int32_t* __restrict__ dflag, int32_t* __restrict__ rflag, int64_t* __restrict__ rmass) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t c = cnt[i];
        const bool dense = keep || (c >= 2 && (int64_t)c >= T);
        const bool rare = !keep && c >= 2 && (int64_t)c < T;
        dflag[i] = dense ? 1 : 0;
        rflag[i] = rare ? 1 : 0;
        rmass[i] = rare ? (int64_t)c : 0;
    }
}

}  // namespace

// ---- dictionary construction ------------------------------------------
// A Summary is a sorted array of distinct codes with the number of sets
// holding each. Summaries of disjoint set ranges merge by summing counts; the
// dictionary is the codes with count >= 2 (or all codes, keep_singletons).


// (keys sorted) -> runs: unique codes, run starts, run count
void runs_of(gdist_ctx* ctx, const uint64_t* keys, int64_t n, DevBuf& flag, DevBuf& pos, DevBuf& uniq,
             DevBuf& start, int64_t& nruns) {
    hipStream_t st = ctx->stream;
    flag.alloc(n * 4 + 4, st);
    pos.alloc(n * 8 + 8, st);
    nruns = 0;
    if (n == 0) { uniq.alloc(8, st); start.alloc(8, st); return; }
    head_flags_u64<<<grid_for(n), 256, 0, st>>>(keys, n, flag.as<int32_t>());
    GD_HIP(hipGetLastError());
    exclusive_scan_i32_to_i64(ctx, flag.as<int32_t>(), pos.as<int64_t>(), (size_t)n);
    int64_t last = 0;
    int32_t lf = 0;
    d2h(&last, pos.as<int64_t>() + n - 1, 8, st);
    d2h(&lf, flag.as<int32_t>() + n - 1, 4, st);
    GD_HIP(hipStreamSynchronize(st));
    nruns = last + lf;
    uniq.alloc(nruns * 8 + 8, st);
    start.alloc(nruns * 8 + 8, st);
    run_heads_kernel<<<grid_for(n), 256, 0, st>>>(keys, flag.as<int32_t>(), pos.as<int64_t>(), n,
                                                   uniq.as<uint64_t>(), start.as<int64_t>());
    GD_HIP(hipGetLastError());
}

namespace {

// merge (codes, counts) parts into one summary
void merge_parts(gdist_ctx* ctx, const std::vector<SummaryView>& parts, Summary& out, int end_bit = 64) {
    hipStream_t st = ctx->stream;
    int64_t m = 0;
    for (auto& p : parts) m += p.n;
    DevBuf kA(m * 8 + 8, st), kB(m * 8 + 8, st), vA(m * 4 + 4, st), vB(m * 4 + 4, st);
    int64_t at = 0;
    for (auto& p : parts) {
        if (p.n) {
            GD_HIP(hipMemcpyAsync(kA.as<uint64_t>() + at, p.codes, p.n * 8, hipMemcpyDeviceToDevice, st));
            GD_HIP(hipMemcpyAsync(vA.as<uint32_t>() + at, p.counts, p.n * 4, hipMemcpyDeviceToDevice, st));
        }
        at += p.n;
    }
    uint64_t* keys = kA.as<uint64_t>(); uint64_t* kalt = kB.as<uint64_t>();
    int32_t* vals = vA.as<int32_t>(); int32_t* valt = vB.as<int32_t>();
    if (parts.size() > 1) sort_pairs_u64_i32(ctx, keys, kalt, vals, valt, (size_t)m, 0, end_bit);
    DevBuf flag, pos, start;
    runs_of(ctx, keys, m, flag, pos, out.codes, start, out.n);
    // per-run sum of counts via prefix sums of the counts
    DevBuf wide((m + 1) * 8, st), cw((m + 1) * 8, st);
    if (m) {
        widen_u32_kernel<<<grid_for(m), 256, 0, st>>>(reinterpret_cast<const uint32_t*>(vals), m, wide.as<int64_t>());
        GD_HIP(hipGetLastError());
    }
    GD_HIP(hipMemsetAsync(wide.as<int64_t>() + m, 0, 8, st));
    exclusive_scan_i64(ctx, wide.as<int64_t>(), cw.as<int64_t>(), (size_t)(m + 1));
    out.counts.alloc(out.n * 4 + 4, st);
    if (out.n) {
        run_totals_kernel<<<(int)ceil_div(out.n, 256), 256, 0, st>>>(start.as<int64_t>(), out.n, m, cw.as<int64_t>(),
                                                                      out.counts.as<uint32_t>());
        GD_HIP(hipGetLastError());
    }
    GD_HIP(hipStreamSynchronize(st));
}

}  // namespace

// Summary of sets [0, nsets): chunked sort + run-length, then merge.
void local_summary(gdist_ctx* ctx, const gdist_sets* s, Summary& out) {
    hipStream_t st = ctx->stream;
    const int cbits = std::min(64, code_bits(s->kind, s->k, s->flags));
    if (!s->pack_sum.empty()) {
        // the pack's chunk summaries (code-major pack sort): merge, no code sort
        if (s->pack_sum.size() == 1) {
            const Summary& p = s->pack_sum[0];
            out.n = p.n;
            out.codes.alloc(p.n * 8 + 8, st);
            out.counts.alloc(p.n * 4 + 4, st);
            if (p.n) {
                GD_HIP(hipMemcpyAsync(out.codes.p, p.codes.p, p.n * 8, hipMemcpyDeviceToDevice, st));
                GD_HIP(hipMemcpyAsync(out.counts.p, p.counts.p, p.n * 4, hipMemcpyDeviceToDevice, st));
            }
            GD_HIP(hipStreamSynchronize(st));
            return;
        }
        std::vector<SummaryView> parts;
        for (auto& p : s->pack_sum) parts.push_back({p.codes.as<uint64_t>(), p.counts.as<uint32_t>(), p.n});
        merge_parts(ctx, parts, out, cbits);
        return;
    }
    std::vector<Summary> chunks;
    int64_t s0 = 0;
    while (s0 < s->nsets) {
        int64_t s1 = s0 + 1;
        while (s1 < s->nsets && s->h_off[s1 + 1] - s->h_off[s0] <= kBitsChunk) s1++;
        const int64_t b = s->h_off[s0], n = s->h_off[s1] - b;
        DevBuf kA(n * 8 + 8, st), kB(n * 8 + 8, st);
        if (n) GD_HIP(hipMemcpyAsync(kA.p, s->codes.as<uint64_t>() + b, n * 8, hipMemcpyDeviceToDevice, st));
        uint64_t* keys = kA.as<uint64_t>(); uint64_t* alt = kB.as<uint64_t>();
        sort_keys_u64(ctx, keys, alt, (size_t)n, 0, cbits);
        Summary c;
        DevBuf flag, pos, start;
        runs_of(ctx, keys, n, flag, pos, c.codes, start, c.n);
        c.counts.alloc(c.n * 4 + 4, st);
        if (c.n) {   // codes are unique per set: run length = number of sets
            run_totals_kernel<<<(int)ceil_div(c.n, 256), 256, 0, st>>>(start.as<int64_t>(), c.n, n, nullptr,
                                                                        c.counts.as<uint32_t>());
            GD_HIP(hipGetLastError());
        }
        GD_HIP(hipStreamSynchronize(st));
        chunks.push_back(std::move(c));
        s0 = s1;
    }
    if (chunks.size() == 1) {
        out.codes = std::move(chunks[0].codes);
        out.counts = std::move(chunks[0].counts);
        out.n = chunks[0].n;
        return;
    }
    std::vector<SummaryView> parts;
    for (auto& c : chunks) parts.push_back({c.codes.as<uint64_t>(), c.counts.as<uint32_t>(), c.n});
    merge_parts(ctx, parts, out);
}

namespace {
// hist[c] += number of summary entries with count c (c <= nsets); small
// counts (the singletons dominate) go through an LDS histogram first
constexpr int kHistLds = 4096;
__global__ void count_hist_kernel(const uint32_t* __restrict__ cnt, int64_t n, int64_t nsets,
                                  unsigned long long* __restrict__ hist) {
    __shared__ unsigned int h[kHistLds];
    for (int t = threadIdx.x; t < kHistLds; t += blockDim.x) h[t] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t c = cnt[i] < (uint32_t)nsets ? (int64_t)cnt[i] : nsets;
        if (c < kHistLds) atomicAdd(&h[c], 1u);
        else atomicAdd(&hist[c], 1ull);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kHistLds && t <= nsets; t += blockDim.x)
        if (h[t]) atomicAdd(&hist[t], (unsigned long long)h[t]);
}

}  // namespace

// Dictionary tiers from merged summaries: dense = codes held by >= T sets
// (all codes with keep_singletons), rare = codes held by 2..T-1 sets.
// rare_mass = number of (code, set) records the rare tier will produce.
void dictionary_from(gdist_ctx* ctx, const std::vector<SummaryView>& parts, bool keep, int64_t& T, int64_t nsets,
                     DevBuf& dict, int64_t& U, DevBuf& rare, int64_t& Ur, int64_t& rare_mass, DevBuf* dcounts) {
    hipStream_t st = ctx->stream;
    Summary all;
    SummaryView m = parts.size() == 1 ? parts[0] : SummaryView{nullptr, nullptr, 0};
    if (parts.size() != 1) {
        merge_parts(ctx, parts, all);
        m = {all.codes.as<uint64_t>(), all.counts.as<uint32_t>(), all.n};
    }
    const int64_t n = m.n;
    if (keep) T = 0;
    if (T < 0) {
        if (ctx->has_option(OPT_RARE_T)) {
            T = ctx->option(OPT_RARE_T, -1);
        } else {
            DevBuf dh((nsets + 1) * 8, st);
            GD_HIP(hipMemsetAsync(dh.p, 0, (nsets + 1) * 8, st));
            if (n) {
                count_hist_kernel<<<grid_for(n, 256, 256 * 16), 256, 0, st>>>(m.counts, n, nsets,
                                                                             dh.as<unsigned long long>());
                GD_HIP(hipGetLastError());
            }
            std::vector<uint64_t> hist(nsets + 1);
            d2h(hist.data(), dh.p, (nsets + 1) * 8, st);
            GD_HIP(hipStreamSynchronize(st));
            T = choose_rare_threshold(hist, nsets);
        }
    }
    U = Ur = rare_mass = 0;
    DevBuf df(n * 4 + 4, st), rf(n * 4 + 4, st), dpos(n * 8 + 8, st), rpos(n * 8 + 8, st), mass(n * 8 + 8, st),
        cmass(n * 8 + 8, st);
    if (n) {
        rare_flag_kernel<<<grid_for(n), 256, 0, st>>>(m.counts, n, T, keep ? 1 : 0, df.as<int32_t>(), rf.as<int32_t>(),
                                                      mass.as<int64_t>());
        GD_HIP(hipGetLastError());
        exclusive_scan_i32_to_i64(ctx, df.as<int32_t>(), dpos.as<int64_t>(), (size_t)n);
        exclusive_scan_i32_to_i64(ctx, rf.as<int32_t>(), rpos.as<int64_t>(), (size_t)n);
        exclusive_scan_i64(ctx, mass.as<int64_t>(), cmass.as<int64_t>(), (size_t)n);
        int64_t h[6];
        int32_t hf[2];
        d2h(&h[0], dpos.as<int64_t>() + n - 1, 8, st);
        d2h(&h[1], rpos.as<int64_t>() + n - 1, 8, st);
        d2h(&h[2], cmass.as<int64_t>() + n - 1, 8, st);
        d2h(&h[3], mass.as<int64_t>() + n - 1, 8, st);
        d2h(&hf[0], df.as<int32_t>() + n - 1, 4, st);
        d2h(&hf[1], rf.as<int32_t>() + n - 1, 4, st);
        U = h[0] + hf[0];
        Ur = h[1] + hf[1];
        rare_mass = h[2] + h[3];
    }
    dict.alloc(U * 8 + 8, st);
    rare.alloc(Ur * 8 + 8, st);
    if (dcounts) dcounts->alloc(U * 4 + 4, st);
    if (n) {
        compact_u64_kernel<<<grid_for(n), 256, 0, st>>>(m.codes, df.as<int32_t>(), dpos.as<int64_t>(), n,
                                                        dict.as<uint64_t>());
        if (dcounts)
            compact_u32_kernel<<<grid_for(n), 256, 0, st>>>(m.counts, df.as<int32_t>(), dpos.as<int64_t>(), n,
                                                            dcounts->as<uint32_t>());
        compact_u64_kernel<<<grid_for(n), 256, 0, st>>>(m.codes, rf.as<int32_t>(), rpos.as<int64_t>(), n,
                                                        rare.as<uint64_t>());
        GD_HIP(hipGetLastError());
    }
    GD_HIP(hipStreamSynchronize(st));
}

namespace {
__global__ void local_mass_kernel(const uint64_t* __restrict__ codes, const uint32_t* __restrict__ cnt, int64_t n,
                                  const uint64_t* __restrict__ rare, int64_t Ur, unsigned long long* __restrict__ out) {
    unsigned long long acc = 0;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t k = codes[i];
        int64_t lo = 0, hi = Ur;
        while (lo < hi) {
            int64_t mid = (lo + hi) >> 1;
            if (rare[mid] < k) lo = mid + 1; else hi = mid;
        }
        if (lo < Ur && rare[lo] == k) acc += cnt[i];
    }
    if (acc) atomicAdd(out, acc);
}

// over the posting lists: sum of m(m-1)/2 (the rare tier's pair increments)
// -> out[0], the longest list -> out[1], the increments of kLongList+ lists
// -> out[2]. One atomic of each kind per workgroup.
__global__ __launch_bounds__(256) void rare_incs_kernel(const int64_t* __restrict__ post_off, int64_t n,
                                                        unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[3][4];
    unsigned long long acc = 0, mx = 0, lng = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < n; l += stride) {
        const unsigned long long m = (unsigned long long)(post_off[l + 1] - post_off[l]);
        const unsigned long long inc = m * (m - 1) / 2;
        acc += inc;
        if (m >= (unsigned long long)kLongList) lng += inc;
        mx = m > mx ? m : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        lng += __shfl_xor(lng, o, 64);
        const unsigned long long om = __shfl_xor(mx, o, 64);
        mx = om > mx ? om : mx;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[0][w] = acc; part[1][w] = mx; part[2][w] = lng; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < (int)(blockDim.x >> 6); v++) {
            acc += part[0][v]; lng += part[2][v];
            mx = part[1][v] > mx ? part[1][v] : mx;
        }
        if (acc) atomicAdd(out, acc);
        if (mx) atomicMax(out + 1, mx);
        if (lng) atomicAdd(out + 2, lng);
    }
}

}  // namespace

// records the local sets contribute to the rare tier (local counts of rare codes)
int64_t local_rare_mass(gdist_ctx* ctx, const Summary& local, const uint64_t* rare, int64_t Ur) {
    hipStream_t st = ctx->stream;
    if (Ur == 0 || local.n == 0) return 0;
    DevBuf c(8, st);
    GD_HIP(hipMemsetAsync(c.p, 0, 8, st));
    local_mass_kernel<<<grid_for(local.n), 256, 0, st>>>(local.codes.as<uint64_t>(), local.counts.as<uint32_t>(),
                                                         local.n, rare, Ur, c.as<unsigned long long>());
    GD_HIP(hipGetLastError());
    int64_t h = 0;
    d2h(&h, c.p, 8, st);
    return h;
}

int64_t bitset_words(int64_t dict_size) {
    return std::max<int64_t>(KC, ceil_div(ceil_div(dict_size, 64), KC) * KC);
}

int64_t auto_rare_threshold(int64_t nsets) {
    // Fixed heuristic (before the histogram model): a dense entry costs one
    // bit column over all N^2/2 pairs, a rare entry held by m sets m(m-1)/2
    // pair increments; ~N/80 balances them for C2-like collections.
    return std::max<int64_t>(2, nsets / 80);
}

int64_t choose_rare_threshold(const std::vector<uint64_t>& hist, int64_t nsets) {
    // cost(T) = pairs * W(dense kmers with count >= T) / dense rate
    //         + the cheaper rare kernel on the lists of kmers with 2 <= count < T
    // over the whole triangle, for every T in [2, nsets+1]; T = 2 is dense-only.
    const double pairs = 0.5 * (double)nsets * (double)(nsets - 1);
    const int64_t top = (int64_t)hist.size() - 1;
    std::vector<double> dense_ge(top + 2, 0.0);
    for (int64_t c = top; c >= 2; c--) dense_ge[c] = dense_ge[c + 1] + (double)hist[c];
    RareTier t;
    double best = -1.0;
    int64_t bestT = 2;
    for (int64_t T = 2; T <= top + 1; T++) {
        if (T > 2) {
            const double c = (double)(T - 1), h = (double)hist[T - 1], inc = h * c * (c - 1.0) / 2.0;
            t.incs += inc;
            if (T - 1 >= kLongList) t.incs_long += inc;
            t.records += h * c;
            t.lists += h;
        }
        const double U = T <= top ? dense_ge[T] : 0.0;
        const double cost = pairs * (double)bitset_words((int64_t)U) / kDenseWordPairsPerS + rare_choice(t, 1.0, 1.0).cost();
        if (best < 0 || cost < best) { best = cost; bestT = T; }
    }
    return bestT;
}

// ---- identical posting lists ------------------------------------------
// Every kmer covering one variant that several sets share has the same
// holders, so the rare tier is full of identical posting lists (C2: 42 per
// shared substitution, 21 windows x 2 strands). Such lists are merged into
// one list whose weight is their number: the kernels add the weight instead
// of 1, and do the work of one list. Lists are grouped by a 64-bit content
// hash and merged only after a member-by-member comparison with the group's
// first list, so a hash collision costs compression, never exactness.
namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void list_hash_kernel(const int64_t* __restrict__ poff, const uint32_t* __restrict__ psets, int64_t nl,
                                 uint64_t* __restrict__ h, int32_t* __restrict__ ids) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nl; l += stride) {
        const int64_t b = poff[l], e = poff[l + 1];
        uint64_t x = mix64(0x9E3779B97F4A7C15ull * (uint64_t)(e - b + 1));
        for (int64_t y = b; y < e; y++) x = mix64(x ^ (0x632BE59BD9B4E019ull + psets[y]));
        h[l] = x;
        ids[l] = (int32_t)l;
    }
}

// sorted (hash, list) -> keep[list] = 0 if its contents equal the run's first
// list (merged into it), else 1; weight[the list it counts for] += 1
__global__ void list_merge_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ flag,
                                  const int64_t* __restrict__ pos, const int64_t* __restrict__ start, int64_t n,
                                  const int64_t* __restrict__ poff, const uint32_t* __restrict__ psets,
                                  int32_t* __restrict__ keep, uint32_t* __restrict__ weight) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t hd = start[pos[i] + flag[i] - 1];
        const int32_t l = ids[i], h = ids[hd];
        bool same = false;
        if (i != hd) {
            const int64_t lb = poff[l], le = poff[l + 1], hb = poff[h], he = poff[h + 1];
            same = le - lb == he - hb;
            for (int64_t y = 0; same && y < le - lb; y++) same = psets[lb + y] == psets[hb + y];
        }
        keep[l] = same ? 0 : 1;
        atomicAdd(weight + (same ? h : l), 1u);
    }
}

__global__ void record_keep_kernel(const uint64_t* __restrict__ recs, int64_t n, const int32_t* __restrict__ keep,
                                   int32_t* __restrict__ rk) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t y = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; y < n; y += stride) rk[y] = keep[recs[y] >> 32];
}

// kept lists' records, renumbered: member sets in list order, and the same
// records keyed by set (set << 32 | new list) for the set -> rare CSR
__global__ void list_compact_kernel(const uint64_t* __restrict__ recs, int64_t n, const int32_t* __restrict__ keep,
                                    const int64_t* __restrict__ newid, const int64_t* __restrict__ rpos,
                                    uint32_t* __restrict__ out_sets, uint64_t* __restrict__ out_recs) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t y = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; y < n; y += stride) {
        const int64_t l = (int64_t)(recs[y] >> 32);
        if (!keep[l]) continue;
        const uint32_t set = (uint32_t)recs[y];
        out_sets[rpos[y]] = set;
        out_recs[rpos[y]] = ((uint64_t)set << 32) | (uint64_t)newid[l];
    }
}

__global__ void list_offsets_kernel(const int64_t* __restrict__ poff, int64_t nl, const int32_t* __restrict__ keep,
                                    const int64_t* __restrict__ newid, const int64_t* __restrict__ rpos,
                                    const uint32_t* __restrict__ weight, int64_t* __restrict__ out_off,
                                    uint32_t* __restrict__ out_w) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nl; l += stride)
        if (keep[l]) { out_off[newid[l]] = rpos[poff[l]]; out_w[newid[l]] = weight[l]; }
}

__global__ void narrow_u16_kernel(const uint32_t* __restrict__ in, int64_t n, uint16_t* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (uint16_t)in[i];
}

__global__ void fill_u32_kernel(uint32_t* __restrict__ p, int64_t n, uint32_t v) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

// set-side weights: the weight of each entry's list
__global__ void entry_weights_kernel(const uint64_t* __restrict__ keys, int64_t n, const uint32_t* __restrict__ pw,
                                     uint32_t* __restrict__ sw) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) sw[i] = pw[(uint32_t)keys[i]];
}

// the heaviest row of the set side: max over sets of the sum of their
// entries' list weights (a pair's rare count is at most its row's)
__global__ void row_weight_max_kernel(const int64_t* __restrict__ soff, const uint32_t* __restrict__ sw,
                                      int64_t nsets, unsigned long long* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long mx = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nsets; i += stride) {
        unsigned long long t = 0;
        for (int64_t x = soff[i]; x < soff[i + 1]; x++) t += sw[x];
        mx = t > mx ? t : mx;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(mx, o, 64);
        mx = v > mx ? v : mx;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(out, mx);
}

}  // namespace

// rare records (rank << 32 | set) -> posting lists CSR on `s`, identical
// lists merged (GDIST_RARE_DEDUP=0 keeps one list per kmer, A/B)
void build_postings(gdist_ctx* ctx, gdist_sets* s, unsigned long long* recs, int64_t n, int64_t Ur) {
    hipStream_t st = ctx->stream;
    Trace tr(st, ctx->trace());
    s->n_rare = Ur;
    s->rare_kmers = Ur;
    s->rare_records = n;
    s->post_off.alloc((Ur + 1) * 8, st);
    s->post_sets.alloc(n * 4 + 16, st);          // padded: the row walk reads 16 bytes at a time
    s->rare_incs = s->rare_max_list = s->rare_incs_long = 0;
    s->rare_row_wmax = 0;
    if (Ur == 0 || n == 0) {
        GD_HIP(hipMemsetAsync(s->post_off.p, 0, (Ur + 1) * 8, st));
        s->post_w.alloc(Ur * 4 + 4, st);
        s->srare_off.alloc((s->nsets + 1) * 8, st);
        GD_HIP(hipMemsetAsync(s->srare_off.p, 0, (s->nsets + 1) * 8, st));
        s->srare_ent.alloc(8, st);
        s->srare_w.alloc(4, st);
        s->srare_skip.alloc(8, st);
        s->n_rare = 0;
        s->rare_records = 0;
        GD_HIP(hipStreamSynchronize(st));
        return;
    }
    GD_REQUIRE(Ur < (int64_t(1) << 31), "rare tier: too many lists");
    DevBuf alt(n * 8, st);
    uint64_t* keys = reinterpret_cast<uint64_t*>(recs);
    uint64_t* kalt = alt.as<uint64_t>();
    int rbits = 1;
    while ((int64_t(1) << rbits) < Ur) rbits++;
    sort_keys_u64(ctx, keys, kalt, (size_t)n, 0, std::min(64, 32 + rbits));
    posting_offsets_kernel<<<(int)ceil_div(Ur + 1, 256), 256, 0, st>>>(keys, n, Ur, s->post_off.as<int64_t>());
    posting_sets_kernel<<<grid_for(n), 256, 0, st>>>(keys, n, s->post_sets.as<uint32_t>());
    GD_HIP(hipGetLastError());
    tr.mark("postings: lists");
    int64_t nl = Ur, nrec = n;
    if (ctx->option(OPT_RARE_DEDUP, 1) != 0) {
        DevBuf hA(Ur * 8, st), hB(Ur * 8, st), iA(Ur * 4, st), iB(Ur * 4, st);
        list_hash_kernel<<<grid_for(Ur), 256, 0, st>>>(s->post_off.as<int64_t>(), s->post_sets.as<uint32_t>(), Ur,
                                                       hA.as<uint64_t>(), iA.as<int32_t>());
        GD_HIP(hipGetLastError());
        uint64_t* hk = hA.as<uint64_t>(); uint64_t* hkalt = hB.as<uint64_t>();
        int32_t* iv = iA.as<int32_t>(); int32_t* ivalt = iB.as<int32_t>();
        sort_pairs_u64_i32(ctx, hk, hkalt, iv, ivalt, (size_t)Ur, 0, 64);
        DevBuf flag, pos, uniq, start;
        int64_t nruns = 0;
        runs_of(ctx, hk, Ur, flag, pos, uniq, start, nruns);
        DevBuf keep(Ur * 4 + 4, st), weight(Ur * 4 + 4, st), newid(Ur * 8 + 8, st);
        GD_HIP(hipMemsetAsync(weight.p, 0, Ur * 4, st));
        list_merge_kernel<<<grid_for(Ur), 256, 0, st>>>(iv, flag.as<int32_t>(), pos.as<int64_t>(), start.as<int64_t>(),
                                                        Ur, s->post_off.as<int64_t>(), s->post_sets.as<uint32_t>(),
                                                        keep.as<int32_t>(), weight.as<uint32_t>());
        GD_HIP(hipGetLastError());
        exclusive_scan_i32_to_i64(ctx, keep.as<int32_t>(), newid.as<int64_t>(), (size_t)Ur);
        DevBuf rk(n * 4 + 4, st), rpos(n * 8 + 8, st);
        record_keep_kernel<<<grid_for(n), 256, 0, st>>>(keys, n, keep.as<int32_t>(), rk.as<int32_t>());
        GD_HIP(hipGetLastError());
        exclusive_scan_i32_to_i64(ctx, rk.as<int32_t>(), rpos.as<int64_t>(), (size_t)n);
        int64_t h[2];
        int32_t hf[2];
        d2h(&h[0], newid.as<int64_t>() + Ur - 1, 8, st);
        d2h(&h[1], rpos.as<int64_t>() + n - 1, 8, st);
        d2h(&hf[0], keep.as<int32_t>() + Ur - 1, 4, st);
        d2h(&hf[1], rk.as<int32_t>() + n - 1, 4, st);
        nl = h[0] + hf[0];
        nrec = h[1] + hf[1];
        DevBuf noff((nl + 1) * 8, st), nsets(nrec * 4 + 16, st);
        s->post_w.alloc(nl * 4 + 4, st);
        list_offsets_kernel<<<grid_for(Ur), 256, 0, st>>>(s->post_off.as<int64_t>(), Ur, keep.as<int32_t>(),
                                                          newid.as<int64_t>(), rpos.as<int64_t>(),
                                                          weight.as<uint32_t>(), noff.as<int64_t>(),
                                                          s->post_w.as<uint32_t>());
        list_compact_kernel<<<grid_for(n), 256, 0, st>>>(keys, n, keep.as<int32_t>(), newid.as<int64_t>(),
                                                         rpos.as<int64_t>(), nsets.as<uint32_t>(), kalt);
        GD_HIP(hipGetLastError());
        h2d(noff.as<int64_t>() + nl, &nrec, 8, st);
        s->post_off = std::move(noff);
        s->post_sets = std::move(nsets);
        tr.mark("postings: merge identical lists");
    } else {
        s->post_w.alloc(Ur * 4 + 4, st);
        fill_u32_kernel<<<grid_for(Ur), 256, 0, st>>>(s->post_w.as<uint32_t>(), Ur, 1u);
        // the same records keyed by set: set -> rare CSR for the row-major kernels
        swap_halves_kernel<<<grid_for(n), 256, 0, st>>>(keys, n, kalt);
        GD_HIP(hipGetLastError());
    }
    s->n_rare = nl;
    s->rare_records = nrec;
    // kalt: (set << 32 | list) records, sorted by set (into `keys`, then swapped back)
    int sbits = 1;
    while ((int64_t(1) << sbits) < s->nsets) sbits++;
    sort_keys_u64(ctx, kalt, keys, (size_t)nrec, 0, std::min(64, 32 + sbits));
    // packed entries: 40-bit list start, 24-bit length (a rare list has < T <= N + 1 sets)
    GD_REQUIRE(nrec < (int64_t(1) << 40) && s->nsets < (int64_t(1) << 24), "rare tier too large for packed list entries");
    s->srare_off.alloc((s->nsets + 1) * 8, st);
    s->srare_ent.alloc(nrec * 8 + 8, st);
    s->srare_w.alloc(nrec * 4 + 4, st);
    posting_offsets_kernel<<<(int)ceil_div(s->nsets + 1, 256), 256, 0, st>>>(kalt, nrec, s->nsets,
                                                                             s->srare_off.as<int64_t>());
    rare_entries_kernel<<<grid_for(nrec), 256, 0, st>>>(kalt, nrec, s->post_off.as<int64_t>(),
                                                        s->srare_ent.as<uint64_t>());
    entry_weights_kernel<<<grid_for(nrec), 256, 0, st>>>(kalt, nrec, s->post_w.as<uint32_t>(),
                                                         s->srare_w.as<uint32_t>());
    s->srare_skip.alloc(nrec * 2 + 8, st);
    rare_skip_kernel<<<grid_for(nrec), 256, 0, st>>>(kalt, nrec, s->post_off.as<int64_t>(), s->post_sets.as<uint32_t>(),
                                                     s->srare_skip.as<uint16_t>());
    GD_HIP(hipGetLastError());
    // 2-byte members for the row-major walk (collections of <= 65,536 sets;
    // option rare_u16 = 0 keeps the 4-byte ones)
    s->post_sets16.release();
    if (s->nsets <= 65536 && ctx->option(OPT_RARE_U16, 1) != 0) {
        s->post_sets16.alloc(nrec * 2 + 16, st);
        GD_HIP(hipMemsetAsync(s->post_sets16.as<uint16_t>() + nrec, 0, 16, st));
        narrow_u16_kernel<<<grid_for(nrec), 256, 0, st>>>(s->post_sets.as<uint32_t>(), nrec,
                                                          s->post_sets16.as<uint16_t>());
        GD_HIP(hipGetLastError());
    }
    // pair increments of the tier (cost model, kernel choice)
    DevBuf d_incs(24, st);
    GD_HIP(hipMemsetAsync(d_incs.p, 0, 24, st));
    rare_incs_kernel<<<grid_for(nl, 256, 4096), 256, 0, st>>>(s->post_off.as<int64_t>(), nl,
                                                              d_incs.as<unsigned long long>());
    GD_HIP(hipGetLastError());
    unsigned long long hi[3] = {0, 0, 0};
    d2h(hi, d_incs.p, 24, st);
    GD_HIP(hipStreamSynchronize(st));
    s->rare_incs = (int64_t)hi[0];
    s->rare_max_list = (int64_t)hi[1];
    s->rare_incs_long = (int64_t)hi[2];
    {
        DevBuf wm(8, st);
        GD_HIP(hipMemsetAsync(wm.p, 0, 8, st));
        row_weight_max_kernel<<<grid_for(s->nsets, 256, 4096), 256, 0, st>>>(
            s->srare_off.as<int64_t>(), s->srare_w.as<uint32_t>(), s->nsets, wm.as<unsigned long long>());
        GD_HIP(hipGetLastError());
        unsigned long long h = 0;
        d2h(&h, wm.p, 8, st);
        s->rare_row_wmax = (int64_t)h;
    }
    tr.mark("postings: set side");
}

void build_bitsets(gdist_ctx* ctx, gdist_sets* s, unsigned flags, int64_t rare_threshold) {
    const bool keep = (flags & GDIST_BITSET_KEEP_SINGLETONS) != 0;
    int64_t T = keep ? 0 : rare_threshold;     // < 0: cost-optimal from the count histogram
    // a rebuild replaces every tier: the old variant lists, sparse words,
    // plans and FP4 operand must not survive into the new representation
    // (a two-tier rebuild of a variant collection would add its stale
    // variant counts on top of the new bits); synchronises both streams
    free_bitsets(s);
    Trace tr(ctx->stream, ctx->trace());
    const auto t_build = std::chrono::steady_clock::now();
    BuildSplit sp = build_split(ctx, s);
    // the build's wall time and its split stages (gdist_sets_build_timing)
    struct BuildClock {
        gdist_sets* s; BuildSplit& sp; hipStream_t st; std::chrono::steady_clock::time_point t0;
        AllocStats a0;
        bool trace;
        ~BuildClock() {
            (void)hipStreamSynchronize(st);
            if (trace) {
                const AllocStats& a = alloc_stats();
                fprintf(stderr, "gdist: build allocations: %lld fresh blocks, %.2f GB, %.1f ms in hipMalloc; %lld cache trims\n",
                        (long long)(a.fresh - a0.fresh), (a.fresh_bytes - a0.fresh_bytes) / 1e9, a.fresh_ms - a0.fresh_ms,
                        (long long)(a.trims - a0.trims));
            }
            s->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            s->build_shares = sp.R;
            s->build_split_ms = s->build_share_max_ms = 0;
            for (double v : sp.share_ms) {
                s->build_split_ms += v;
                s->build_share_max_ms = std::max(s->build_share_max_ms, v);
            }
        }
    } clock{s, sp, ctx->stream, t_build, alloc_stats(), ctx->trace()};
    Summary sum;
    // a collection without pack summaries and too many codes for one sort
    // (a gathered 8-GPU collection: C4's 2e10 codes) is counted by code
    // ranges, singletons dropped as they are counted (option range_summary);
    // a split build counts by ranges (its shares are code ranges)
    const int64_t rs_opt = ctx->option(OPT_RANGE_SUMMARY, -1);
    const bool by_range = rs_opt > 0 || (rs_opt < 0 && ((s->pack_sum.empty() && s->total > kRangeSummaryMin) || sp.R > 1));
    if (by_range) range_summary(ctx, s, keep ? 1 : 2, sum, sp);
    else local_summary(ctx, s, sum);
    tr.mark("bitsets: summary");
    DevBuf dict, rare, dcnt;
    int64_t U = 0, Ur = 0, mass = 0;
    const int64_t T_in = T;
    dictionary_from(ctx, {SummaryView{sum.codes.as<uint64_t>(), sum.counts.as<uint32_t>(), sum.n}}, keep, T, s->nsets,
                    dict, U, rare, Ur, mass, &dcnt);
    tr.mark("bitsets: dictionary");
    // the variant tier when kmers held by T .. Dmin - 1 sets dominate the
    // dictionary (variant.hip); its rare threshold is at most kVariantMaxT
    // unless given: kmers shared by a few sets stay posting lists, the rest
    // of the non-dense kmers form the variant words
    if (!keep) {
        // the variant tier's rare threshold: the model's T (which prices the
        // kmers below Dmin as dense words or posting lists only) capped at
        // kVariantMaxT unless given; its share of the summary decides
        const int64_t dmin = variant_dmin(ctx, s->nsets);
        const int64_t Tv = (T_in >= 0 || ctx->has_option(OPT_RARE_T)) ? T : std::min<int64_t>(T, kVariantMaxT);
        const int64_t mid = count_in_range(ctx, sum.counts.as<uint32_t>(), sum.n, Tv, dmin);
        const int64_t ge = count_in_range(ctx, sum.counts.as<uint32_t>(), sum.n, Tv, INT64_MAX);
        if (variant_wanted(ctx, s->nsets, mid, ge)) {
            if (Tv != T) {
                T = Tv;
                dictionary_from(ctx, {SummaryView{sum.codes.as<uint64_t>(), sum.counts.as<uint32_t>(), sum.n}}, false,
                                T, s->nsets, dict, U, rare, Ur, mass, &dcnt);
            }
            sum.codes.release();
            sum.counts.release();
            // 47-kmer words (option variant_bits, default): a substitution's k
            // windows on each strand fit one word when k x strands <= 47, and
            // with < 2^17 sets a list member packs into 8 bytes (C4: 42 kmers
            // a substitution, 100,000 sets); else 64-kmer words of 12-byte members
            const int strands = (s->kind == GDIST_DNA && (s->flags & GDIST_STRAND_MASK) == GDIST_STRAND_BOTH) ? 2 : 1;
            const int64_t vb = ctx->option(OPT_VARIANT_BITS, (s->nsets < (int64_t(1) << 17) &&
                                                              (int64_t)s->k * strands <= 47) ? 47 : 64);
            build_variant_bitsets(ctx, s, dict, dcnt, U, rare, Ur, mass, T, sp, -1, vb == 47 ? 47 : 64);
            return;
        }
        // The grouped rare tier (round 5, option rare_group): the kmers of 2 ..
        // T - 1 sets as variant words of 16 kmers, one substitution a word
        // (its k windows held by nearly the same sets), walked a thread an
        // entry from packed (set | mask << 16) lists. C3: 71.9 M posting
        // records (Σ m(m−1)/2 ≈ 0.5 G increments of 2-byte members, each record
        // a random line) become 22.7 M entries and 0.28 G products. By default
        // for 4,096 .. 65,536 sets with locus guides and many rare records; the
        // dense tier keeps its threshold T (option variant = 0 keeps the two
        // tiers unless rare_group = 1).
        const int64_t rg = ctx->option(OPT_RARE_GROUP, -1);
        const bool group = s->nsets <= 65536 && T > 2 && mass > 0 &&
                           (rg > 0 || (rg < 0 && ctx->option(OPT_VARIANT, -1) != 0 && s->nsets >= kVariantMinSets &&
                                       s->n_guide > 0 && locus_order_enabled(ctx) && mass >= 64 * s->nsets));
        if (group) {
            const int64_t dmin = T;
            T = 2;
            dictionary_from(ctx, {SummaryView{sum.codes.as<uint64_t>(), sum.counts.as<uint32_t>(), sum.n}}, false, T,
                            s->nsets, dict, U, rare, Ur, mass, &dcnt);
            // (probing by default and with rare_group = 2; 1 forces the tier)
            if (build_variant_bitsets(ctx, s, dict, dcnt, U, rare, Ur, mass, T, sp, dmin, 16, rg <= 0 || rg == 2)) {
                sum.codes.release();
                sum.counts.release();
                return;
            }
            // keyless kmers dominate (no substitution structure): the two tiers
            T = dmin;
            dictionary_from(ctx, {SummaryView{sum.codes.as<uint64_t>(), sum.counts.as<uint32_t>(), sum.n}}, false, T,
                            s->nsets, dict, U, rare, Ur, mass, &dcnt);
        }
    }
    const int64_t W = bitset_words(U);
    DevBuf perm;
    if (s->n_guide > 0 && locus_order_enabled(ctx)) {
        DevBuf key;
        locus_keys(ctx, s, dict.as<uint64_t>(), dcnt.as<uint32_t>(), U, 0, key);
        locus_perm(ctx, key, U, perm);
        tr.mark("bitsets: locus order");
    }
    s->fp4.release();                    // the MFMA operand expanded the old bits
    s->fp4_W = 0;
    // rows of R equal shares (split build): slot r of the in-place all-gather
    const int64_t mrows = BuildSplit::ceil_div_h(s->nsets, sp.R);
    s->bits.alloc((size_t)sp.R * mrows * W * 8 + 8, ctx->stream);
    DevBuf recs(mass * 8 + 8, ctx->stream);
    int64_t written = 0;
    tr.mark("bitsets: alloc");
    for (int r = sp.first(); r < sp.last(); r++) {
        ShareClock clk(sp, r, ctx->stream);
        int64_t w = 0;
        fill_bits(ctx, s, dict.as<uint64_t>(), U, W, s->bits.as<unsigned long long>(), rare.as<uint64_t>(), Ur, 0,
                  recs.as<unsigned long long>() + written, mass - written, &w, perm.as<uint32_t>(), FillHook(),
                  sp.set_lo(r, s->nsets), sp.set_hi(r, s->nsets));
        written += w;
    }
    if (sp.real) {
        comm_allgather_inplace(ctx, s->bits.p, (size_t)mrows * W * 8);
        written = allgather_concat(ctx, recs, written, 8);
    }
    tr.mark("bitsets: fill");
    GD_REQUIRE(written == mass, "rare-tier record count mismatch");
    build_postings(ctx, s, recs.as<unsigned long long>(), written, Ur);
    tr.mark("bitsets: postings");
    s->W = W;
    s->dict_size = U;
    s->rare_T = T;
    s->bits_keep_singletons = keep;
    build_sparse_words(ctx, s);
}

void free_bitsets(gdist_sets* s) {
    free_sparse(s);                      // (synchronises both streams, clears plans and graphs)
    free_variant(s);
    s->fp4.release();
    s->fp4_W = 0;
    s->bits.release();
    s->post_off.release();
    s->post_sets.release();
    s->post_sets16.release();
    s->post_w.release();
    s->srare_off.release();
    s->srare_ent.release();
    s->srare_w.release();
    s->srare_skip.release();
    s->W = s->dict_size = 0;
    s->n_rare = s->rare_T = s->rare_records = s->rare_incs = s->rare_max_list = s->rare_incs_long = 0;
    s->rare_row_wmax = 0;
    s->rare_kmers = 0;
}

}  // namespace gdist
