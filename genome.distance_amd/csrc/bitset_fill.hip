// bitset_fill.hip — the fill of the bitset build: every code of every set
// looked up in the dense dictionary (its bit set in the set's row, at its
// locus position through perm) and in the rare codes (a (rare rank << 32 |
// set) record appended); singletons are in neither.
//
// The device's form of SequenceKmers filling its kmer set as it reads a
// sequence (the sets FastaDistanceProcessor.java:177-186 then intersects).
// fill_bits chooses among five generations (option fill_sort): the default
// two passes without global atomics (fill_window_kernel + fill_merge_kernel
// write each code's bit position, pos_bits_kernel ORs a row slice in LDS and
// stores it whole; bits_from_positions is pass 2 alone), the same with one
// wave a segment (fill_pos_kernel), the one-pass windowed searches with global
// atomics (fill_search_kernel), the chunked pairs sort with run ranks
// (run_rank_kernel + scatter_bits_kernel), and the hash fill for sets sparse
// against the dictionary (variant.hip hash_fill).
#include <algorithm>

#include "gdist_internal.hpp"

namespace gdist {
namespace {

__global__ void set_ids_kernel(const int64_t* __restrict__ off, int64_t s0, int64_t s1, int32_t* __restrict__ ids) {
    const int64_t base = off[s0];
    const int64_t n = off[s1] - base;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int64_t i = base + e;
        int64_t lo = s0, hi = s1;   // upper_bound(off, i) - 1
        while (hi - lo > 1) {
            int64_t mid = (lo + hi) >> 1;
            if (off[mid] <= i) lo = mid; else hi = mid;
        }
        ids[e] = (int32_t)lo;
    }
}

// rank of each run's code: r >= 0 in the dense dictionary, -(r + 2) in the
// rare dictionary, -1 in neither
__global__ void run_rank_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ start, int64_t nruns,
                                const uint64_t* __restrict__ dict, int64_t U, const uint64_t* __restrict__ rare,
                                int64_t Ur, int64_t* __restrict__ rank) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nruns) return;
    const uint64_t k = keys[start[r]];
    int64_t lo = 0, hi = U;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (dict[mid] < k) lo = mid + 1; else hi = mid;
    }
    if (lo < U && dict[lo] == k) { rank[r] = lo; return; }
    lo = 0; hi = Ur;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (rare[mid] < k) lo = mid + 1; else hi = mid;
    }
    rank[r] = (lo < Ur && rare[lo] == k) ? -(lo + 2) : -1;
}

// dense ranks -> bits; rare ranks -> (rare rank << 32 | global set id) records
__global__ void scatter_bits_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ flag,
                                    const int64_t* __restrict__ pos, const int64_t* __restrict__ rank, int64_t n,
                                    int64_t W, unsigned long long* __restrict__ bits, int64_t id_base,
                                    unsigned long long* __restrict__ rare_out, unsigned long long* __restrict__ rare_cnt,
                                    int64_t rare_cap, const uint32_t* __restrict__ perm) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t run = pos[i] + flag[i] - 1;       // inclusive run index
        const int64_t r = rank[run];
        if (r >= 0) {
            const int64_t b = perm ? (int64_t)perm[r] : r;   // bit position (locus order)
            atomicOr(bits + (int64_t)ids[i] * W + (b >> 6), 1ull << (b & 63));
        } else if (r <= -2) {
            const unsigned long long slot = atomicAdd(rare_cnt, 1ull);
            if ((int64_t)slot < rare_cap)
                rare_out[slot] = ((unsigned long long)(-r - 2) << 32) | (unsigned long long)(uint32_t)(ids[i] + id_base);
        }
    }
}

}  // namespace

// The fill without a sort: each set's codes are sorted (pack), and so are
// the dense dictionary and the rare codes, so a wave takes a segment of
// kFillSeg consecutive codes of ONE set, finds the segment's window in the
// dictionary and in the rare codes (four binary searches, one lane each),
// and each lane then searches its codes inside those windows (L1-resident).
// Dense codes set their bit (locus position through perm), rare codes append
// a (rare rank << 32 | set) record; singletons are skipped. Segments that
// straddle a set boundary are cut there, so a window is always monotone.
constexpr int kFillSeg = 2048;
__device__ __forceinline__ int64_t lower_bound_u64(const uint64_t* __restrict__ a, int64_t lo, int64_t hi, uint64_t k) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(256) void fill_search_kernel(
    const uint64_t* __restrict__ codes, const int64_t* __restrict__ off, const int64_t* __restrict__ seg,
    int64_t nseg, const uint64_t* __restrict__ dict, int64_t U, const uint64_t* __restrict__ rare, int64_t Ur,
    int64_t W, unsigned long long* __restrict__ bits, int64_t id_base, unsigned long long* __restrict__ rare_out,
    unsigned long long* __restrict__ rare_cnt, int64_t rare_cap, const uint32_t* __restrict__ perm) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave >= nseg) return;
    // segment: (set << 40 | first code index) packed, its end the next segment's start or its set's end
    const uint64_t sd = (uint64_t)seg[wave];
    const int64_t set = (int64_t)(sd >> 40), b = (int64_t)(sd & ((1ull << 40) - 1));
    const int64_t e = std::min<int64_t>(b + kFillSeg, off[set + 1]);
    if (e <= b) return;
    const uint64_t kfirst = codes[b], klast = codes[e - 1];
    // lanes 0-3: the windows [lower_bound(first), upper_bound(last)) in dict and rare
    int64_t w = 0;
    if (lane == 0) w = lower_bound_u64(dict, 0, U, kfirst);
    else if (lane == 1) w = lower_bound_u64(dict, 0, U, klast + 1 == 0 ? klast : klast + 1) + (klast == ~0ull);
    else if (lane == 2) w = lower_bound_u64(rare, 0, Ur, kfirst);
    else if (lane == 3) w = lower_bound_u64(rare, 0, Ur, klast + 1 == 0 ? klast : klast + 1) + (klast == ~0ull);
    const int64_t dlo = __shfl((long long)w, 0, 64), dhi = std::min<int64_t>(U, __shfl((long long)w, 1, 64));
    const int64_t rlo = __shfl((long long)w, 2, 64), rhi = std::min<int64_t>(Ur, __shfl((long long)w, 3, 64));
    unsigned long long* row = bits + set * W;
    for (int64_t i = b + lane; i < e; i += 64) {
        const uint64_t k = codes[i];
        const int64_t r = lower_bound_u64(dict, dlo, dhi, k);
        if (r < dhi && dict[r] == k) {
            const int64_t pos = perm ? (int64_t)perm[r] : r;     // bit position (locus order)
            atomicOr(row + (pos >> 6), 1ull << (pos & 63));
            continue;
        }
        const int64_t q = lower_bound_u64(rare, rlo, rhi, k);
        if (q < rhi && rare[q] == k) {
            const unsigned long long slot = atomicAdd(rare_cnt, 1ull);
            if ((int64_t)slot < rare_cap)
                rare_out[slot] = ((unsigned long long)q << 32) | (unsigned long long)(uint32_t)(set + id_base);
        }
    }
}

// The default fill, in two passes so that no bit is set by a global atomic
// (a wave's 64 atomicOr land in 64 different rows' cache lines, the slow
// case of the L2 atomic unit: the one-pass fill above spends 0.27 s of C2's
// setup on them).
// Pass 1 (fill_window_kernel + fill_pos_kernel): segments of up to kPosSeg
// consecutive codes of one set (shorter for sets much smaller than the
// dictionary, so that a segment's window fits in LDS). One thread per
// (segment, bound) finds the segment's windows [dlo, dhi) in the dense codes
// and [rlo, rhi) in the rare codes and writes them beside the segment's
// bounds - independent searches, instead of a dependent chain inside the
// wave that uses them. A wave (one per block) then stages its dense window in
// LDS with coalesced loads (codes and their bit positions perm[]), loads its
// codes up front, and each lane binary-searches its codes in LDS. Misses
// (about 1 code in 100 on C2) are listed in LDS and looked up together after
// the dense pass: a search over LDS fences (every 8th rare code of the
// window) and one 64-byte load of the 8-code bucket, so a segment waits on
// one global latency for its rare codes, not one per round. Each code's bit
// position (u32; ~0 outside the dense tier) goes to a position array
// parallel to the codes; rare-tier codes append their records (one atomic
// per wave and round). A window over the LDS caps (a set sparse against the
// dictionary) falls back to a wave walk over global memory.
// (The one-pass fill's per-lane binary searches in global memory chain ~20
// dependent loads per code: it is latency-bound at 0.27 s for C2.)
// Pass 2 (pos_bits_kernel): a workgroup owns one set's row slice of
// kPosSlice 32-bit words in LDS, streams the set's positions, ORs the ones in
// its slice into LDS (ds_or) and stores the slice whole: every row word is
// written once, coalesced, and the row needs no memset.
constexpr int kPosSeg = 512;       // codes per segment (at most)
constexpr int kWinDense = 768;     // LDS dense-window cap (entries)
constexpr int kRareBucket = 8;     // rare codes per LDS fence
constexpr int kRareFences = 256;   // LDS fence cap (a rare window of up to 2048 codes)
constexpr int kPosSlice = 32768;   // 32-bit row words per workgroup (128 KiB of LDS)
constexpr int64_t kFillPosChunk = int64_t(1) << 30;   // codes per position-array chunk (4 GiB)

__device__ __forceinline__ int64_t upper_bound_u64(const uint64_t* __restrict__ a, int64_t lo, int64_t hi, uint64_t k) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] <= k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// per segment 8 int64: dlo, dhi, rlo, rhi, (set << 40 | b), e
__global__ __launch_bounds__(256) void fill_window_kernel(const uint64_t* __restrict__ codes,
                                                          const int64_t* __restrict__ off, const int64_t* __restrict__ seg,
                                                          int64_t ns, const uint64_t* __restrict__ dict, int64_t U,
                                                          const uint64_t* __restrict__ rare, int64_t Ur,
                                                          int64_t* __restrict__ win) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ns * 4) return;
    const int64_t sg = t >> 2;
    const uint64_t sd = (uint64_t)seg[sg];
    const int64_t set = (int64_t)(sd >> 40), b = (int64_t)(sd & ((1ull << 40) - 1));
    int64_t e = off[set + 1];   // the next segment's start within the set
    if (sg + 1 < ns) {
        const uint64_t nx = (uint64_t)seg[sg + 1];
        if ((int64_t)(nx >> 40) == set) e = (int64_t)(nx & ((1ull << 40) - 1));
    }
    const int which = (int)(t & 3);
    const uint64_t* a = which < 2 ? dict : rare;
    const int64_t n = which < 2 ? U : Ur;
    win[sg * 8 + which] = (which & 1) ? upper_bound_u64(a, 0, n, codes[e - 1]) : lower_bound_u64(a, 0, n, codes[b]);
    if (which == 0) {
        win[sg * 8 + 4] = (int64_t)sd;
        win[sg * 8 + 5] = e;
    }
}

// Ranks of the active lanes' codes k (sorted across lanes) in a[P, hi) of
// global memory (the fallback walk): rk = lower bound, hit = a[rk] == k. P is
// uniform and only moves forward; on return it is the largest active rank.
__device__ __forceinline__ void wave_rank(const uint64_t* __restrict__ a, int64_t& P, int64_t hi, uint64_t k,
                                          bool active, int64_t& rk, bool& hit) {
    const int lane = threadIdx.x & 63;
    bool pend = active;
    rk = hi;
    hit = false;
    for (int round = 0; __ballot(pend); round++) {
        const int nb = (int)std::min<int64_t>(64, hi - P);
        if (nb <= 0) break;   // pending lanes: past the end (rk = hi, no hit)
        const uint64_t B = lane < nb ? a[P + lane] : ~0ull;
        int c = 0;   // # block codes < k
#pragma unroll
        for (int st = 32; st >= 1; st >>= 1) {
            const uint64_t v = (uint64_t)__shfl((long long)B, c + st - 1, 64);
            if (c + st <= nb && v < k) c += st;
        }
        const uint64_t v = (uint64_t)__shfl((long long)B, c & 63, 64);
        if (c < nb && v < k) c++;
        const uint64_t m = (uint64_t)__shfl((long long)B, c & 63, 64);
        if (pend && (c < nb || P + nb >= hi)) {
            rk = P + c;
            hit = c < nb && m == k;
            pend = false;
        }
        const unsigned long long left = __ballot(pend);
        if (!left) break;
        const uint64_t kmin = (uint64_t)__shfl((long long)k, __ffsll((long long)left) - 1, 64);
        P += nb;
        if (round >= 1) P = lower_bound_u64(a, P, hi, kmin);   // uniform: a gap, search it
    }
    const unsigned long long act = __ballot(active);
    if (act) P = __shfl((long long)rk, 63 - __clzll((long long)act), 64);
}

// lower bound of k in LDS a[0, n)
__device__ __forceinline__ int lds_lower_bound(const uint64_t* a, int n, uint64_t k) {
    int lo = 0;
    for (int len = n; len > 0;) {
        const int half = len >> 1;
        if (a[lo + half] < k) { lo += half + 1; len -= half + 1; } else len = half;
    }
    return lo;
}

// Rare-tier records of a one-wave block, staged in LDS and appended to the
// output with ONE atomic per kRareBuf records: C2's fill appended ~17 records
// a segment with one atomic each on a single counter (2 M per launch), and
// same-address atomics run at ~0.1 G/s — 84 of the fill's 112 ms.
constexpr int kRareBuf = 256;
struct WaveRareBuf {
    unsigned long long* buf;              // LDS [cap]
    int n;                                // records staged (wave-uniform)
    int cap;
};
__device__ __forceinline__ void rare_flush(WaveRareBuf& rb, unsigned long long* __restrict__ rare_out,
                                           unsigned long long* __restrict__ rare_cnt, int64_t rare_cap) {
    if (!rb.n) return;
    __builtin_amdgcn_wave_barrier();
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const int lane = threadIdx.x & 63;
    unsigned long long g = 0;
    if (lane == 0) g = atomicAdd(rare_cnt, (unsigned long long)rb.n);
    g = (unsigned long long)__shfl((long long)g, 0, 64);
    for (int j = lane; j < rb.n; j += 64)
        if ((int64_t)(g + j) < rare_cap) rare_out[g + j] = rb.buf[j];
    __builtin_amdgcn_wave_barrier();
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    rb.n = 0;
}
__device__ __forceinline__ void append_rare(bool rhit, int64_t q, int64_t set, int64_t id_base, WaveRareBuf& rb,
                                            unsigned long long* __restrict__ rare_out,
                                            unsigned long long* __restrict__ rare_cnt, int64_t rare_cap) {
    const unsigned long long m = __ballot(rhit);
    if (!m) return;
    const int c = __popcll(m);
    if (rb.n + c > rb.cap) rare_flush(rb, rare_out, rare_cnt, rare_cap);
    if (rhit) {
        const int lane = threadIdx.x & 63;
        rb.buf[rb.n + __popcll(m & ((1ull << lane) - 1))] =
            ((unsigned long long)q << 32) | (unsigned long long)(uint32_t)(set + id_base);
    }
    rb.n += c;
}

// one wave per block; the blocks take the segments in turn (their rare
// records staged across segments, above)
__global__ __launch_bounds__(64) void fill_pos_kernel(
    const uint64_t* __restrict__ codes, const int64_t* __restrict__ win, int64_t ns, const uint64_t* __restrict__ dict,
    const uint64_t* __restrict__ rare, int64_t base, uint32_t* __restrict__ pos_out, int64_t id_base,
    unsigned long long* __restrict__ rare_out, unsigned long long* __restrict__ rare_cnt, int64_t rare_cap,
    const uint32_t* __restrict__ perm) {
    __shared__ uint64_t s_d[kWinDense];
    __shared__ uint32_t s_p[kWinDense];
    __shared__ uint64_t s_f[kRareFences];
    __shared__ uint64_t s_mk[kPosSeg];
    __shared__ unsigned long long s_rb[kRareBuf];
    const int lane = threadIdx.x;
    WaveRareBuf rb{s_rb, 0, kRareBuf};
    for (int64_t sg = blockIdx.x; sg < ns; sg += gridDim.x) {
    __syncthreads();                                      // the previous segment's LDS reads are done
    const int64_t wv = lane < 6 ? win[sg * 8 + lane] : 0;
    int64_t dlo = __shfl((long long)wv, 0, 64), dhi = __shfl((long long)wv, 1, 64);
    int64_t rlo = __shfl((long long)wv, 2, 64), rhi = __shfl((long long)wv, 3, 64);
    const uint64_t sd = (uint64_t)__shfl((long long)wv, 4, 64);
    const int64_t e = __shfl((long long)wv, 5, 64);
    const int64_t set = (int64_t)(sd >> 40), b = (int64_t)(sd & ((1ull << 40) - 1));
    const int64_t nd = dhi - dlo, nr = rhi - rlo, nf = (nr + kRareBucket - 1) / kRareBucket;
    if (nd <= kWinDense && nf <= kRareFences) {
        // lane l takes the segment's codes [8 l, 8 l + 8): one binary search
        // for the first, then (codes ascending) a short forward walk per code
        // from the previous code's rank
        constexpr int PL = kPosSeg / 64;
        const int64_t i0 = b + (int64_t)PL * lane;
        uint64_t kk[PL];
#pragma unroll
        for (int j = 0; j < PL; j++) kk[j] = i0 + j < e ? codes[i0 + j] : 0;
        for (int j = lane; j < nd; j += 64) {
            s_d[j] = dict[dlo + j];
            s_p[j] = perm ? perm[dlo + j] : (uint32_t)(dlo + j);
        }
        for (int j = lane; j < nf; j += 64) s_f[j] = rare[rlo + (int64_t)j * kRareBucket];
        __syncthreads();
        int nm = 0;   // misses listed (uniform)
        int r = i0 < e ? lds_lower_bound(s_d, (int)nd, kk[0]) : (int)nd;
#pragma unroll
        for (int j = 0; j < PL; j++) {
            const int64_t i = i0 + j;
            const bool valid = i < e;
            bool miss = false;
            if (valid) {
                const uint64_t k = kk[j];
                // forward from the previous rank: two steps, then a search of the rest
                if (r < nd && s_d[r] < k) {
                    r++;
                    if (r < nd && s_d[r] < k) r = r + 1 + lds_lower_bound(s_d + r + 1, (int)nd - r - 1, k);
                }
                const bool hit = r < nd && s_d[r] == k;
                pos_out[i - base] = hit ? s_p[r] : ~0u;
                miss = !hit;
            }
            const unsigned long long m = __ballot(miss);
            if (miss) s_mk[nm + __popcll(m & ((1ull << lane) - 1))] = kk[j];
            nm += __popcll(m);
        }
        __syncthreads();
        for (int t0 = 0; t0 < nm; t0 += 64) {
            bool rhit = false;
            int64_t q = 0;
            if (t0 + lane < nm && nf > 0) {
                const uint64_t k = s_mk[t0 + lane];
                const int g = lds_lower_bound(s_f, (int)nf, k + 1) - 1;   // last fence <= k (k = ~0: the last fence)
                if (g >= 0 || k == ~0ull) {
                    const int gg = g >= 0 ? g : (int)nf - 1;
                    const int64_t q0 = rlo + (int64_t)gg * kRareBucket;
                    uint64_t v[kRareBucket];
#pragma unroll
                    for (int u = 0; u < kRareBucket; u++) v[u] = q0 + u < rhi ? rare[q0 + u] : 0;
#pragma unroll
                    for (int u = 0; u < kRareBucket; u++)
                        if (q0 + u < rhi && v[u] == k) { rhit = true; q = q0 + u; }
                }
            }
            append_rare(rhit, q, set, id_base, rb, rare_out, rare_cnt, rare_cap);
        }
        continue;
    }
    // fallback: walk the windows in global memory
    for (int64_t i0 = b; i0 < e; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool valid = i < e;
        const uint64_t k = valid ? codes[i] : 0;
        int64_t r;
        bool hit;
        wave_rank(dict, dlo, dhi, k, valid, r, hit);
        if (valid) pos_out[i - base] = hit ? (perm ? perm[r] : (uint32_t)r) : ~0u;
        const bool miss = valid && !hit;
        if (__ballot(miss) && rlo < rhi) {
            int64_t q;
            bool rhit;
            wave_rank(rare, rlo, rhi, k, miss, q, rhit);
            append_rare(rhit, q, set, id_base, rb, rare_out, rare_cnt, rare_cap);
        }
    }
    }
    rare_flush(rb, rare_out, rare_cnt, rare_cap);
}

// The default pass 1 (round 4): a 256-thread workgroup per segment of up to
// kMSeg codes. fill_pos_kernel above runs one wave with 17 KiB of LDS, so a
// CU holds ~9 waves and each waits out its own global and LDS latency chains
// (C2: 21 ms per 2^30 codes). Here four waves share one staged window: the
// dense window (padded one entry in 8 so that lanes whose ranks sit ~8 apart
// spread over the banks instead of 16 to a bank) and the rare fences; a
// thread takes 8 consecutive codes (one search, then the forward walk), its
// bit positions are gathered from perm[] in global memory (8 independent
// loads, no LDS copy), and each wave lists its misses as 16-bit offsets
// (one list per wave: it cannot overflow) and stages its rare records in its
// own buffer. ~37 KiB a workgroup: four workgroups, 16 waves, per CU.
constexpr int kMNT = 256;
constexpr int kMPT = 8;
constexpr int kMSeg = kMNT * kMPT;           // 2048 codes
constexpr int kMWin = 2560;                  // dense window cap
constexpr int kMFences = 1024;               // rare window cap kMFences x kRareBucket
constexpr int kMWaveRare = 128;              // rare records staged per wave
__device__ __forceinline__ int mpad(int r) { return r + (r >> 3); }
__device__ __forceinline__ int lds_lower_bound_pad(const uint64_t* a, int lo, int n, uint64_t k) {
    for (int len = n - lo; len > 0;) {
        const int half = len >> 1;
        if (a[mpad(lo + half)] < k) { lo += half + 1; len -= half + 1; } else len = half;
    }
    return lo;
}
__global__ __launch_bounds__(kMNT) void fill_merge_kernel(
    const uint64_t* __restrict__ codes, const int64_t* __restrict__ win, int64_t ns, const uint64_t* __restrict__ dict,
    const uint64_t* __restrict__ rare, int64_t base, uint32_t* __restrict__ pos_out, int64_t id_base,
    unsigned long long* __restrict__ rare_out, unsigned long long* __restrict__ rare_cnt, int64_t rare_cap,
    const uint32_t* __restrict__ perm) {
    constexpr int NW = kMNT / 64, WC = kMSeg / NW;
    __shared__ uint64_t s_d[kMWin + kMWin / 8];
    __shared__ uint64_t s_f[kMFences];
    __shared__ uint16_t s_mi[NW][WC];
    __shared__ unsigned long long s_rb[NW][kMWaveRare];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    WaveRareBuf rb{s_rb[wv], 0, kMWaveRare};
    for (int64_t sg = blockIdx.x; sg < ns; sg += gridDim.x) {
        const int64_t* w = win + sg * 8;
        const int64_t dlo = w[0], dhi = w[1], rlo = w[2], rhi = w[3];
        const uint64_t sd = (uint64_t)w[4];
        const int64_t e = w[5];
        const int64_t set = (int64_t)(sd >> 40), b = (int64_t)(sd & ((1ull << 40) - 1));
        const int64_t nd = dhi - dlo, nr = rhi - rlo, nf = (nr + kRareBucket - 1) / kRareBucket;
        __syncthreads();                                  // the previous segment's LDS reads are done
        if (nd <= kMWin && nf <= kMFences && e - b <= kMSeg) {
            const int64_t i0 = b + (int64_t)kMPT * threadIdx.x;
            uint64_t kk[kMPT];
#pragma unroll
            for (int j = 0; j < kMPT; j++) kk[j] = i0 + j < e ? codes[i0 + j] : 0;
            for (int j = threadIdx.x; j < nd; j += kMNT) s_d[mpad(j)] = dict[dlo + j];
            for (int j = threadIdx.x; j < nf; j += kMNT) s_f[j] = rare[rlo + (int64_t)j * kRareBucket];
            __syncthreads();
            const int n = (int)nd;
            int r = i0 < e ? lds_lower_bound_pad(s_d, 0, n, kk[0]) : n;
            int nm = 0;                                   // the wave's misses (uniform)
            int rk[kMPT];
            bool hit[kMPT];
#pragma unroll
            for (int j = 0; j < kMPT; j++) {
                const bool valid = i0 + j < e;
                hit[j] = false;
                if (valid) {
                    const uint64_t k = kk[j];
                    if (r < n && s_d[mpad(r)] < k) {
                        r++;
                        if (r < n && s_d[mpad(r)] < k) r = lds_lower_bound_pad(s_d, r + 1, n, k);
                    }
                    hit[j] = r < n && s_d[mpad(r)] == k;
                }
                rk[j] = r;
                const bool miss = valid && !hit[j];
                const unsigned long long m = __ballot(miss);
                if (miss) s_mi[wv][nm + __popcll(m & ((1ull << lane) - 1))] = (uint16_t)(i0 + j - b);
                nm += __popcll(m);
            }
            uint32_t pv[kMPT];
#pragma unroll
            for (int j = 0; j < kMPT; j++)
                pv[j] = hit[j] ? (perm ? perm[dlo + rk[j]] : (uint32_t)(dlo + rk[j])) : ~0u;
#pragma unroll
            for (int j = 0; j < kMPT; j++)
                if (i0 + j < e) pos_out[i0 + j - base] = pv[j];
            __builtin_amdgcn_wave_barrier();
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            for (int t0 = 0; t0 < nm; t0 += 64) {
                bool rhit = false;
                int64_t q = 0;
                if (t0 + lane < nm && nf > 0) {
                    const uint64_t k = codes[b + s_mi[wv][t0 + lane]];
                    const int g = lds_lower_bound(s_f, (int)nf, k + 1) - 1;   // last fence <= k (k = ~0: the last fence)
                    if (g >= 0 || k == ~0ull) {
                        const int gg = g >= 0 ? g : (int)nf - 1;
                        const int64_t q0 = rlo + (int64_t)gg * kRareBucket;
                        uint64_t v[kRareBucket];
#pragma unroll
                        for (int u = 0; u < kRareBucket; u++) v[u] = q0 + u < rhi ? rare[q0 + u] : 0;
#pragma unroll
                        for (int u = 0; u < kRareBucket; u++)
                            if (q0 + u < rhi && v[u] == k) { rhit = true; q = q0 + u; }
                    }
                }
                append_rare(rhit, q, set, id_base, rb, rare_out, rare_cnt, rare_cap);
            }
            continue;
        }
        // fallback: each wave walks its share of the codes over the windows in global memory
        int64_t dp = dlo, rp = rlo;
        for (int64_t c0 = b + 64 * wv; c0 < e; c0 += kMNT) {
            const int64_t i = c0 + lane;
            const bool valid = i < e;
            const uint64_t k = valid ? codes[i] : 0;
            int64_t r;
            bool hit;
            wave_rank(dict, dp, dhi, k, valid, r, hit);
            if (valid) pos_out[i - base] = hit ? (perm ? perm[r] : (uint32_t)r) : ~0u;
            const bool miss = valid && !hit;
            if (__ballot(miss) && rp < rhi) {
                int64_t q;
                bool rhit;
                wave_rank(rare, rp, rhi, k, miss, q, rhit);
                append_rare(rhit, q, set, id_base, rb, rare_out, rare_cnt, rare_cap);
            }
        }
    }
    rare_flush(rb, rare_out, rare_cnt, rare_cap);
}

__device__ __forceinline__ void pos_or(uint32_t* lds, uint32_t p, uint32_t sb) {
    const uint32_t x = (p >> 5) - sb;   // ~0 positions and other slices wrap to >= kPosSlice
    if (x < (uint32_t)kPosSlice) atomicOr(lds + x, 1u << (p & 31));
}

// grid (slices, sets of the chunk); block 1024
__global__ __launch_bounds__(1024) void pos_bits_kernel(const uint32_t* __restrict__ pos, const int64_t* __restrict__ off,
                                                        int64_t s0, int64_t base, int64_t W, uint32_t* __restrict__ bits) {
    __shared__ uint32_t lds[kPosSlice];
    const int64_t set = s0 + blockIdx.y;
    const int64_t words = 2 * W;
    const uint32_t sb = blockIdx.x * (uint32_t)kPosSlice;
    const int n32 = (int)std::min<int64_t>(kPosSlice, words - sb);
    for (int j = threadIdx.x; j < kPosSlice; j += 1024) lds[j] = 0;
    __syncthreads();
    int64_t ob = off[set] - base;
    const int64_t oe = off[set + 1] - base;
    // head up to a 16-byte boundary, then 4 x uint4 per thread per pass, then the tail
    const int64_t ha = std::min<int64_t>(oe, (ob + 3) & ~int64_t(3));
    if (ob + threadIdx.x < ha) pos_or(lds, pos[ob + threadIdx.x], sb);
    ob = ha;
    const int64_t nv = (oe - ob) >> 2;   // whole uint4 in [ob, oe)
    const uint4* v = reinterpret_cast<const uint4*>(pos + ob);
    int64_t j = threadIdx.x;
    for (; j + 3 * 1024 < nv; j += 4 * 1024) {
        uint4 a[4];
#pragma unroll
        for (int u = 0; u < 4; u++) a[u] = v[j + u * 1024];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            pos_or(lds, a[u].x, sb); pos_or(lds, a[u].y, sb); pos_or(lds, a[u].z, sb); pos_or(lds, a[u].w, sb);
        }
    }
    for (; j < nv; j += 1024) {
        const uint4 a = v[j];
        pos_or(lds, a.x, sb); pos_or(lds, a.y, sb); pos_or(lds, a.z, sb); pos_or(lds, a.w, sb);
    }
    const int64_t t = ob + nv * 4 + threadIdx.x;
    if (t < oe) pos_or(lds, pos[t], sb);
    __syncthreads();
    uint32_t* row = bits + set * words + sb;
    for (int x = threadIdx.x; x < n32; x += 1024) row[x] = lds[x];
}

// bits of sets [0, nsets) against the dense dictionary (default: merged
// positions + LDS slices; option fill_sort 1: the chunked pairs sort + run
// ranks + scatter; 2: the one-pass windowed searches with global atomics);
// rare-tier records appended to rare_out (capacity cap)
void bits_from_positions(gdist_ctx* ctx, const gdist_sets* s, const uint32_t* pos, int64_t s0, int64_t s1,
                         int64_t base, int64_t W, unsigned long long* bits) {
    const unsigned nslice = (unsigned)ceil_div(2 * W, kPosSlice);
    if (W == 0) return;
    for (int64_t c0 = s0; c0 < s1; c0 += 65535) {
        const unsigned ny = (unsigned)std::min<int64_t>(65535, s1 - c0);
        pos_bits_kernel<<<dim3(nslice, ny), 1024, 0, ctx->stream>>>(pos, s->off.as<int64_t>(), c0, base, W,
                                                                     reinterpret_cast<uint32_t*>(bits));
        GD_HIP(hipGetLastError());
    }
}

void fill_bits(gdist_ctx* ctx, const gdist_sets* s, const uint64_t* dict, int64_t U, int64_t W,
               unsigned long long* bits, const uint64_t* rare, int64_t Ur, int64_t id_base,
               unsigned long long* rare_out, int64_t rare_cap, int64_t* rare_written, const uint32_t* perm,
               const FillHook& hook, int64_t sa, int64_t sb) {
    hipStream_t st = ctx->stream;
    if (sb < 0) sb = s->nsets;
    GD_REQUIRE(0 <= sa && sa <= sb && sb <= s->nsets, "fill set range outside the collection");
    // Sets sparse against the dictionary (C3: 33 K codes a set against tens of
    // millions) give the windowed fill's segments windows past its LDS caps
    // even at 64 codes (dictionary entries per code of a set >= 12 dense or
    // >= 32 rare): every segment would walk global memory. The hash fill
    // probes a table of the dictionary instead. Option fill_sort: 0 or 3 the
    // windows, 1 the sort, 2 the atomics, 4 the hash, 5 the windows one wave a
    // segment (round 3's pass 1).
    const int64_t total = s->h_off[s->nsets];
    const double per_set = (double)total / (double)std::max<int64_t>(1, s->nsets);
    const bool sparse_sets = (double)U > 12.0 * per_set || (double)Ur > 32.0 * per_set;
    const int64_t opt = ctx->option(OPT_FILL_SORT, -1);
    if (U + Ur > 0 && (opt == 4 || (opt < 0 && sparse_sets))) {
        hash_fill(ctx, s, dict, U, perm, rare, Ur, W, bits, id_base, rare_out, rare_cap, rare_written, hook, sa, sb);
        return;
    }
    const int cbits = std::min(64, code_bits(s->kind, s->k, s->flags));
    Trace tr(st, ctx->trace());
    GD_HIP(hipMemsetAsync(bits + (size_t)sa * W, 0, (size_t)(sb - sa) * W * 8, st));
    DevBuf rcnt(8, st);
    GD_HIP(hipMemsetAsync(rcnt.p, 0, 8, st));
    // the hook needs the position arrays; option 5: pass 1 by fill_pos_kernel (one wave a segment)
    const int64_t mode = hook || opt == 3 || opt == 5 || opt < 0 ? 0 : opt;
    const bool wave_fill = opt == 5;
    if (U + Ur > 0 && mode == 0) {
        GD_REQUIRE(s->nsets < (int64_t(1) << 23) && s->h_off[s->nsets] < (int64_t(1) << 40),
                   "collection too large for packed fill segments");
        GD_REQUIRE(U <= (int64_t(1) << 31), "dense tier too large for u32 positions");   // keeps ~0 out of every row
        // segment length per set: its windows should fit the LDS caps (window ~ length x dictionary / set size)
        std::vector<int64_t> seg, first(s->nsets + 1, 0);
        for (int64_t i = sa; i < sb; i++) {
            first[i] = (int64_t)seg.size();
            const double ni = (double)(s->h_off[i + 1] - s->h_off[i]);
            const double wd = wave_fill ? kWinDense : kMWin, wf = wave_fill ? kRareFences : kMFences;
            const double fit = 0.8 * std::min(wd * ni / (double)std::max<int64_t>(1, U),
                                              wf * kRareBucket * ni / (double)std::max<int64_t>(1, Ur));
            const int64_t L = std::max<int64_t>(64, std::min<int64_t>(wave_fill ? kPosSeg : kMSeg, (int64_t)(fit / 64) * 64));
            for (int64_t b = s->h_off[i]; b < s->h_off[i + 1]; b += L) seg.push_back((i << 40) | b);
        }
        first[sb] = (int64_t)seg.size();
        DevBuf dseg(std::max<int64_t>(1, (int64_t)seg.size()) * 8, st);
        if (!seg.empty()) h2d(dseg.p, seg.data(), seg.size() * 8, st);
        const unsigned nslice = (unsigned)ceil_div(2 * W, kPosSlice);
        int64_t s0 = sa;
        while (s0 < sb) {
            int64_t s1 = s0 + 1;
            while (s1 < sb && s->h_off[s1 + 1] - s->h_off[s0] <= kFillPosChunk) s1++;
            const int64_t base = s->h_off[s0], n = s->h_off[s1] - base, ns = first[s1] - first[s0];
            // sized like the summary's per-chunk key buffers (8 B a code) so that the caching
            // allocator hands back one of those blocks: a fresh 4 GiB block costs ~25 ms
            DevBuf pos(std::max<int64_t>(1, n) * 8 + 8, st);
            if (ns) {
                const int64_t* sg = dseg.as<int64_t>() + first[s0];
                DevBuf win(ns * 8 * 8, st);
                fill_window_kernel<<<(unsigned)ceil_div(ns * 4, 256), 256, 0, st>>>(
                    s->codes.as<uint64_t>(), s->off.as<int64_t>(), sg, ns, dict, U, rare, Ur, win.as<int64_t>());
                GD_HIP(hipGetLastError());
                GD_REQUIRE(ns < (int64_t(1) << 31), "too many fill segments in one chunk");
                // blocks take the segments in turn (a block's rare records staged across them)
                if (wave_fill) {
                    const int64_t nblk = std::min<int64_t>(ns, (int64_t)ctx->cus * 32);
                    fill_pos_kernel<<<(unsigned)nblk, 64, 0, st>>>(s->codes.as<uint64_t>(), win.as<int64_t>(), ns,
                                                                 dict, rare, base, pos.as<uint32_t>(), id_base,
                                                                 rare_out, rcnt.as<unsigned long long>(), rare_cap,
                                                                 perm);
                } else {
                    // persistent: exactly the resident workgroups (a block that only
                    // starts when a resident one exits would run its share at the end)
                    static int per_cu = 0;
                    if (!per_cu) {
                        GD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fill_merge_kernel, kMNT, 0));
                        per_cu = std::max(1, per_cu);
                    }
                    const int64_t nblk = std::min<int64_t>(ns, (int64_t)ctx->cus * per_cu);
                    fill_merge_kernel<<<(unsigned)nblk, kMNT, 0, st>>>(s->codes.as<uint64_t>(), win.as<int64_t>(),
                                                                       ns, dict, rare, base, pos.as<uint32_t>(),
                                                                       id_base, rare_out,
                                                                       rcnt.as<unsigned long long>(), rare_cap, perm);
                }
                GD_HIP(hipGetLastError());
            }
            tr.mark("fill: merged positions");
            if (hook) hook(pos.as<uint32_t>(), s0, s1, base);
            for (int64_t c0 = s0; c0 < s1; c0 += 65535) {
                const unsigned ny = (unsigned)std::min<int64_t>(65535, s1 - c0);
                pos_bits_kernel<<<dim3(nslice, ny), 1024, 0, st>>>(pos.as<uint32_t>(), s->off.as<int64_t>(), c0, base,
                                                                    W, reinterpret_cast<uint32_t*>(bits));
                GD_HIP(hipGetLastError());
            }
            GD_HIP(hipStreamSynchronize(st));
            tr.mark("fill: LDS row slices");
            s0 = s1;
        }
    } else if (U + Ur > 0 && mode == 2) {
        // segments of <= kFillSeg codes inside one set, built on the host from the offsets
        GD_REQUIRE(s->nsets < (int64_t(1) << 23) && s->h_off[s->nsets] < (int64_t(1) << 40),
                   "collection too large for packed fill segments");
        std::vector<int64_t> seg;
        for (int64_t i = sa; i < sb; i++)
            for (int64_t b = s->h_off[i]; b < s->h_off[i + 1]; b += kFillSeg) seg.push_back((i << 40) | b);
        const int64_t nseg = (int64_t)seg.size();
        if (nseg) {
            DevBuf dseg(nseg * 8, st);
            h2d(dseg.p, seg.data(), nseg * 8, st);
            const int64_t threads = nseg * 64;
            fill_search_kernel<<<(unsigned)ceil_div(threads, 256), 256, 0, st>>>(
                s->codes.as<uint64_t>(), s->off.as<int64_t>(), dseg.as<int64_t>(), nseg, dict, U, rare, Ur, W, bits,
                id_base, rare_out, rcnt.as<unsigned long long>(), rare_cap, perm);
            GD_HIP(hipGetLastError());
            GD_HIP(hipStreamSynchronize(st));
        }
        tr.mark("fill: windowed searches + scatter");
    } else if (U + Ur > 0) {
        int64_t s0 = sa;
        while (s0 < sb) {
            int64_t s1 = s0 + 1;
            while (s1 < sb && s->h_off[s1 + 1] - s->h_off[s0] <= kBitsChunk) s1++;
            const int64_t b = s->h_off[s0], n = s->h_off[s1] - b;
            if (n) {
                DevBuf kA(n * 8, st), kB(n * 8, st), vA(n * 4, st), vB(n * 4, st);
                GD_HIP(hipMemcpyAsync(kA.p, s->codes.as<uint64_t>() + b, n * 8, hipMemcpyDeviceToDevice, st));
                set_ids_kernel<<<grid_for(n), 256, 0, st>>>(s->off.as<int64_t>(), s0, s1, vA.as<int32_t>());
                GD_HIP(hipGetLastError());
                uint64_t* keys = kA.as<uint64_t>(); uint64_t* kalt = kB.as<uint64_t>();
                int32_t* ids = vA.as<int32_t>(); int32_t* ialt = vB.as<int32_t>();
                sort_pairs_u64_i32(ctx, keys, kalt, ids, ialt, (size_t)n, 0, cbits);
                DevBuf flag, pos, uniq, start;
                int64_t nruns = 0;
                runs_of(ctx, keys, n, flag, pos, uniq, start, nruns);
                DevBuf rank(nruns * 8 + 8, st);
                run_rank_kernel<<<(int)ceil_div(nruns, 256), 256, 0, st>>>(keys, start.as<int64_t>(), nruns, dict, U,
                                                                           rare, Ur, rank.as<int64_t>());
                GD_HIP(hipGetLastError());
                tr.mark("fill: copy+sort+runs+rank");
                scatter_bits_kernel<<<grid_for(n), 256, 0, st>>>(ids, flag.as<int32_t>(), pos.as<int64_t>(),
                                                                 rank.as<int64_t>(), n, W, bits, id_base, rare_out,
                                                                 rcnt.as<unsigned long long>(), rare_cap, perm);
                GD_HIP(hipGetLastError());
                GD_HIP(hipStreamSynchronize(st));
                tr.mark("fill: scatter");
            }
            s0 = s1;
        }
    }
    int64_t w = 0;
    d2h(&w, rcnt.p, 8, st);
    GD_REQUIRE(w <= rare_cap, "rare-tier record count exceeds its reservation");
    *rare_written = w;
}

}  // namespace gdist
