// pairs.hip — the distances of an arbitrary (id1, id2) pair list in one call.
//
// getDistance over a pair list (MethodTableProcessor.java:258-276; the lists
// of BasicPairsProcessor.java:71-89 and PairCreateProcessor.java:29-32): P
// intersections, one upload, one download. The rectangle kernels do not fit:
// a list of many first genomes with a handful of partners each fills no tile.
//
// Plan (on the device, no host round trip): the pair positions are sorted by
// row (sort_pairs_u64_i32, stable: positions ascend within a row); the runs of
// equal row are the groups. A run is cut into chunks of at most UNIT_COLS
// consecutive pairs, and a chunk whose codes (|A_i| plus its columns' sets)
// exceed the call's budget into several ranges of the segment index
// (sorted.hip build_segments): the units. The budget is the list's codes over
// UNITS_PER_CU units a CU, within [UNIT_CODES_MIN, UNIT_CODES_MAX]: a short
// list is cut finer. A unit adds its counts into a zeroed I with
// atomicAdd (integers: exact, order-free), so a few pairs of huge sets still
// fill the chip. plan_kernel counts the units of each chunk start, a scan
// places them, units_kernel writes them; the join kernel reads their number
// from device memory and strides over them.
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
#include <algorithm>
#include <cstring>

#include "gdist_internal.hpp"

namespace gdist {
namespace {

constexpr int UNIT_COLS = 64;               // pairs of one row a unit holds at most
// codes (row + columns) past which a unit is cut by segment range: the list's
// codes over UNITS_PER_CU units a CU, within [UNIT_CODES_MIN, UNIT_CODES_MAX]
constexpr int64_t UNIT_CODES_MIN = 1 << 14, UNIT_CODES_MAX = 1 << 18;
constexpr int UNITS_PER_CU = 8;
constexpr int NTP = 512;                    // threads of a join workgroup (8 waves)
constexpr int STAGE = 4096;                 // keys of A staged at a time (32 KiB)

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void pairs_keys_kernel(const int64_t* __restrict__ rows, int64_t n, uint64_t* __restrict__ keys,
                                  int32_t* __restrict__ vals) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    keys[p] = (uint64_t)rows[p];
    vals[p] = (int32_t)p;
}

// pairs of the run of keys[k] in [k, k + UNIT_COLS)
__device__ __forceinline__ int chunk_pairs(const uint64_t* __restrict__ keys, int64_t n, int64_t k) {
    const uint64_t key = keys[k];
    int c = 1;
    while (c < UNIT_COLS && k + c < n && keys[k + c] == key) c++;
    return c;
}

// counts[0] += the run heads (groups). With budget > 0: ucount[k] = the units
// of the chunk that starts at sorted position k (0: k starts no chunk).
__global__ void pairs_plan_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n,
                                  const int64_t* __restrict__ cols, const int64_t* __restrict__ off, int nseg,
                                  int64_t budget, int32_t* __restrict__ ucount,
                                  unsigned long long* __restrict__ counts) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t key = keys[k];
    if (k == 0 || keys[k - 1] != key) atomicAdd(&counts[0], 1ull);
    if (budget <= 0) return;
    int64_t lo = 0, hi = k;                 // the run's first position
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    int32_t u = 0;
    if (((k - lo) % UNIT_COLS) == 0) {
        const int c = chunk_pairs(keys, n, k);
        int64_t codes = off[key + 1] - off[key];
        for (int t = 0; t < c; t++) {
            const int64_t j = cols[vals[k + t]];
            codes += off[j + 1] - off[j];
        }
        const int64_t want = (codes + budget - 1) / budget;
        u = (int32_t)(want < 1 ? 1 : (want > nseg ? nseg : want));
    }
    ucount[k] = u;
}

// unit: {first sorted position, pairs, first segment, end segment}
__global__ void pairs_units_kernel(const uint64_t* __restrict__ keys, int64_t n, const int32_t* __restrict__ ucount,
                                   const int64_t* __restrict__ ubase, int nseg, int64_t cap, int4* __restrict__ units,
                                   unsigned long long* __restrict__ counts) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int u = ucount[k];
    const int64_t b = ubase[k];
    if (k == n - 1) {
        const int64_t tot = b + u;
        counts[1] = (unsigned long long)(tot < cap ? tot : cap);
    }
    if (!u) return;
    const int c = chunk_pairs(keys, n, k);
    for (int t = 0; t < u; t++) {
        if (b + t >= cap) return;           // defensive: the host's bound holds every unit
        units[b + t] = make_int4((int)k, c, (int)((int64_t)nseg * t / u), (int)((int64_t)nseg * (t + 1) / u));
    }
}

__global__ __launch_bounds__(NTP) void pairs_sorted_kernel(
    const uint64_t* __restrict__ codes, const int64_t* __restrict__ segoff, int nseg,
    const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, const int64_t* __restrict__ cols,
    const int4* __restrict__ units, const unsigned long long* __restrict__ counts, int32_t* __restrict__ I) {
    __shared__ unsigned long long sa[STAGE];
    __shared__ int32_t cnt[UNIT_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nunits = (int64_t)counts[1];
    const int64_t per = nseg + 1;
    for (int64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const int4 un = units[u];
        const int64_t k0 = un.x;
        const int ncol = un.y;
        const int64_t i = (int64_t)keys[k0];
        const int64_t* arow = segoff + i * per;
        if (tid < UNIT_COLS) cnt[tid] = 0;
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
                    c = wave_sum(c);
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
        acc = wave_sum(acc);
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
    const bool sorted = method == GDIST_METHOD_SORTED;
    const bool timed = ctx->option(OPT_TIME_KERNELS, 0) != 0;
    ctx->pairs_kernel_ms = -1.0;
    ctx->pairs_groups = ctx->pairs_units = 0;
    // one upload: rows, then cols
    std::vector<int64_t> hin((size_t)2 * n);
    std::copy(rows, rows + n, hin.begin());
    std::copy(cols, cols + n, hin.begin() + n);
    // the budget, and the most units the plan can make with it: a chunk per pair, and a cut per budget of the chunks' codes
    int64_t ucap = 0, budget = 0;
    if (sorted) {
        double codes = 0;
        for (int64_t p = 0; p < n; p++)
            codes += (double)(s->h_off[rows[p] + 1] - s->h_off[rows[p]] + s->h_off[cols[p] + 1] - s->h_off[cols[p]]);
        budget = std::max(UNIT_CODES_MIN,
                          std::min(UNIT_CODES_MAX, (int64_t)(codes / ((double)ctx->cus * UNITS_PER_CU))));
        ucap = n + (int64_t)(codes / (double)budget) + 1;
    }
    DevBuf din((size_t)2 * n * 8, st);
    DevBuf k0((size_t)n * 8, st), k1((size_t)n * 8, st), v0((size_t)n * 4, st), v1((size_t)n * 4, st);
    DevBuf ucount, ubase, units;
    if (sorted) {
        ucount.alloc((size_t)n * 4, st);
        ubase.alloc((size_t)n * 8, st);
        units.alloc((size_t)ucap * sizeof(int4), st);
    }
    // one download: {groups, units}, I, D
    const size_t i_at = 16, d_at = i_at + (((size_t)n * 4 + 7) & ~(size_t)7);
    const size_t out_bytes = d_at + (D_out ? (size_t)n * 8 : 0);
    DevBuf dout(out_bytes, st);
    auto* counts = dout.as<unsigned long long>();
    auto* dI = reinterpret_cast<int32_t*>(static_cast<char*>(dout.p) + i_at);
    double* dD = D_out ? reinterpret_cast<double*>(static_cast<char*>(dout.p) + d_at) : nullptr;
    const int64_t* drows = din.as<int64_t>();
    const int64_t* dcols = drows + n;
    h2d(din.p, hin.data(), (size_t)2 * n * 8, st);

    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() { for (int i = 0; i < 2; i++) if (e[i]) (void)hipEventDestroy(e[i]); }
    } guard{ev};
    if (timed) {
        for (auto& e : ev) GD_HIP(hipEventCreate(&e));
        GD_HIP(hipEventRecord(ev[0], st));
    }
    const unsigned g256 = (unsigned)ceil_div(n, 256);
    GD_HIP(hipMemsetAsync(dout.p, 0, d_at, st));           // the counts and I
    uint64_t *keys = k0.as<uint64_t>(), *kalt = k1.as<uint64_t>();
    int32_t *vals = v0.as<int32_t>(), *valt = v1.as<int32_t>();
    pairs_keys_kernel<<<g256, 256, 0, st>>>(drows, n, keys, vals);
    GD_HIP(hipGetLastError());
    int eb = 1;
    while (eb < 64 && (int64_t(1) << eb) < s->nsets) eb++;
    sort_pairs_u64_i32(ctx, keys, kalt, vals, valt, (size_t)n, 0, eb);
    pairs_plan_kernel<<<g256, 256, 0, st>>>(keys, vals, n, dcols, s->off.as<int64_t>(), s->nseg,
                                            budget, ucount.as<int32_t>(), counts);
    GD_HIP(hipGetLastError());
    if (sorted) {
        exclusive_scan_i32_to_i64(ctx, ucount.as<int32_t>(), ubase.as<int64_t>(), (size_t)n);
        pairs_units_kernel<<<g256, 256, 0, st>>>(keys, n, ucount.as<int32_t>(), ubase.as<int64_t>(), s->nseg, ucap,
                                                 units.as<int4>(), counts);
        GD_HIP(hipGetLastError());
        const unsigned grid = (unsigned)std::min<int64_t>(ucap, (int64_t)ctx->cus * 8);
        pairs_sorted_kernel<<<grid, NTP, 0, st>>>(s->codes.as<uint64_t>(), s->segoff.as<int64_t>(), s->nseg, keys, vals,
                                                  dcols, units.as<int4>(), counts, dI);
        GD_HIP(hipGetLastError());
    } else {
        const bool rare = s->n_rare > 0;
        const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n, 4), (int64_t)ctx->cus * 16);
        pairs_bitset_kernel<<<grid, 256, 0, st>>>(
            s->bits.as<unsigned long long>(), s->W, rare ? s->srare_off.as<int64_t>() : nullptr,
            s->srare_ent.as<uint64_t>(), s->srare_w.as<uint32_t>(), s->post_sets.as<uint32_t>(),
            s->variant ? s->vs_off.as<int64_t>() : nullptr, s->vs_ent.as<uint32_t>(), s->vw_set.as<uint32_t>(),
            s->vw_mask.as<unsigned long long>(), s->vw_beg.as<uint32_t>(), s->vw_end.as<uint32_t>(), keys, vals, dcols,
            n, dI);
        GD_HIP(hipGetLastError());
    }
    pairs_epilogue_kernel<<<g256, 256, 0, st>>>(s->off.as<int64_t>(), drows, dcols, n,
                                                (flags & GDIST_EMPTY_NAN) ? 1 : 0, dI, dD);
    GD_HIP(hipGetLastError());
    if (timed) GD_HIP(hipEventRecord(ev[1], st));
    std::vector<char> hout(out_bytes);
    d2h(hout.data(), dout.p, out_bytes, st);
    if (timed) {
        float ms = 0;
        GD_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        ctx->pairs_kernel_ms = ms;
    }
    const auto* hc = reinterpret_cast<const unsigned long long*>(hout.data());
    ctx->pairs_groups = (int64_t)hc[0];
    ctx->pairs_units = sorted ? (int64_t)hc[1] : n;   // bitset path: a wave's worth of work a pair
    if (I_out) std::memcpy(I_out, hout.data() + i_at, (size_t)n * 4);
    if (D_out) std::memcpy(D_out, hout.data() + d_at, (size_t)n * 8);
}

}  // namespace gdist
