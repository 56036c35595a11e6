// pair_list.hip — the plan of a pair list on the device (struct PairList,
// gdist_internal.hpp): what gdist_pairs, gdist_cross_pairs and
// gdist_sketch_pairs do alike.
//
// The pair positions are sorted by row (sort_pairs_u64_i32, stable: positions
// ascend within a row); the runs of equal row are the groups, cut into chunks
// of at most kPairUnit consecutive pairs (pair_list.hpp). pl_plan_kernel
// counts the groups and the units of each chunk head, a scan places them,
// pl_units_kernel writes them; the consumer reads their number from device
// memory and strides over them. The two calls differ by their Cut: how many units a
// chunk makes and what a unit record holds.
#include <cstring>

#include "gdist_internal.hpp"
#include "pair_list.hpp"

namespace gdist {
namespace {

// a chunk is a unit (sketches: a signature is at most `width` hashes, a pair is never split)
struct ChunkCut {
    using Unit = int2;
    __device__ int units(const uint64_t*, const int32_t*, int64_t, int64_t) const { return 1; }
    __device__ int2 unit(int k, int c, int, int) const { return make_int2(k, c); }
};

// a chunk whose codes exceed the budget is cut into ranges of the segment index;
// the row's size from roff, the columns' from coff (one collection: the same)
struct SegmentCut {
    using Unit = int4;
    const int64_t *cols, *roff, *coff;
    int nseg;
    int64_t budget;
    __device__ int units(const uint64_t* keys, const int32_t* vals, int64_t n, int64_t k) const {
        const uint64_t key = keys[k];
        const int c = pl_unit_pairs(keys, n, k);
        int64_t codes = roff[key + 1] - roff[key];
        for (int t = 0; t < c; t++) {
            const int64_t j = cols[vals[k + t]];
            codes += coff[j + 1] - coff[j];
        }
        return pl_chunk_units(codes, budget, nseg);
    }
    __device__ int4 unit(int k, int c, int t, int u) const {
        return make_int4(k, c, pl_unit_seg(nseg, t, u), pl_unit_seg(nseg, t + 1, u));
    }
};

__global__ void pl_keys_kernel(const int64_t* __restrict__ rows, int64_t n, uint64_t* __restrict__ keys,
                               int32_t* __restrict__ vals) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    keys[p] = (uint64_t)rows[p];
    vals[p] = (int32_t)p;
}

// counts[0] += the group heads. With ucount: ucount[k] = the units of the
// chunk that starts at sorted position k (0: k starts no chunk).
template <class Cut>
__global__ void pl_plan_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n,
                               Cut cut, int32_t* __restrict__ ucount, unsigned long long* __restrict__ counts) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (pl_group_head(keys, k)) atomicAdd(&counts[0], 1ull);
    if (!ucount) return;
    ucount[k] = pl_unit_head(keys, k) ? cut.units(keys, vals, n, k) : 0;
}

// counts[1] = the units: at most the host's cap (pl_unit_cap; n when a chunk is a unit)
template <class Cut>
__global__ void pl_units_kernel(const uint64_t* __restrict__ keys, int64_t n, const int32_t* __restrict__ ucount,
                                const int64_t* __restrict__ ubase, Cut cut, typename Cut::Unit* __restrict__ units,
                                unsigned long long* __restrict__ counts) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int u = ucount[k];
    const int64_t b = ubase[k];
    if (k == n - 1) counts[1] = (unsigned long long)(b + u);
    if (!u) return;
    const int c = pl_unit_pairs(keys, n, k);
    for (int t = 0; t < u; t++) units[b + t] = cut.unit((int)k, c, t, u);
}

// cap: the most units the cut can make (0: the groups only, no scan and no units kernel)
template <class Cut>
void plan(PairList& pl, const Cut& cut, int64_t cap) {
    gdist_ctx* ctx = pl.ctx;
    hipStream_t st = ctx->stream;
    const int64_t n = pl.n;
    if (cap) {
        pl.ucount.alloc((size_t)n * 4, st);
        pl.ubase.alloc((size_t)n * 8, st);
        pl.units.alloc((size_t)cap * sizeof(typename Cut::Unit), st);
        pl.ucap = cap;
    }
    if (pl.timed) {
        for (auto& e : pl.ev) GD_HIP(hipEventCreate(&e));
        GD_HIP(hipEventRecord(pl.ev[0], st));
    }
    const unsigned g256 = (unsigned)ceil_div(n, 256);
    GD_HIP(hipMemsetAsync(pl.out.p, 0, pl.zero_I ? pl.d_at : pl.i_at, st));   // the counts (and I)
    uint64_t *keys = pl.k0.as<uint64_t>(), *kalt = pl.k1.as<uint64_t>();
    int32_t *vals = pl.v0.as<int32_t>(), *valt = pl.v1.as<int32_t>();
    pl_keys_kernel<<<g256, 256, 0, st>>>(pl.rows, n, keys, vals);
    GD_HIP(hipGetLastError());
    int eb = 1;
    while (eb < 64 && (int64_t(1) << eb) < pl.nsets) eb++;
    sort_pairs_u64_i32(ctx, keys, kalt, vals, valt, (size_t)n, 0, eb);
    pl.keys = keys;
    pl.vals = vals;
    pl_plan_kernel<<<g256, 256, 0, st>>>(keys, vals, n, cut, pl.ucount.as<int32_t>(), pl.counts);
    GD_HIP(hipGetLastError());
    if (!cap) return;
    exclusive_scan_i32_to_i64(ctx, pl.ucount.as<int32_t>(), pl.ubase.as<int64_t>(), (size_t)n);
    pl_units_kernel<<<g256, 256, 0, st>>>(keys, n, pl.ucount.as<int32_t>(), pl.ubase.as<int64_t>(), cut,
                                          pl.units.as<typename Cut::Unit>(), pl.counts);
    GD_HIP(hipGetLastError());
}

}  // namespace

PairList::PairList(gdist_ctx* c, int64_t nsets_, int64_t n_, const int64_t* hrows, const int64_t* hcols, int32_t* I_out_,
                   double* D_out_, bool need_I)
    : ctx(c), n(n_), nsets(nsets_), I_out(I_out_), D_out(D_out_), zero_I(need_I),
      timed(c->option(OPT_TIME_KERNELS, 0) != 0) {
    hipStream_t st = ctx->stream;
    // one upload: rows, then cols
    std::vector<int64_t> hin((size_t)2 * n);
    std::copy(hrows, hrows + n, hin.begin());
    std::copy(hcols, hcols + n, hin.begin() + n);
    in.alloc((size_t)2 * n * 8, st);
    k0.alloc((size_t)n * 8, st);
    k1.alloc((size_t)n * 8, st);
    v0.alloc((size_t)n * 4, st);
    v1.alloc((size_t)n * 4, st);
    // one download: {groups, units}, I, D
    i_at = 16;
    d_at = i_at + ((need_I || I_out) ? ((size_t)n * 4 + 7) & ~(size_t)7 : 0);
    out.alloc(d_at + (D_out ? (size_t)n * 8 : 0), st);
    counts = out.as<unsigned long long>();
    I = d_at > i_at ? reinterpret_cast<int32_t*>(static_cast<char*>(out.p) + i_at) : nullptr;
    D = D_out ? reinterpret_cast<double*>(static_cast<char*>(out.p) + d_at) : nullptr;
    rows = in.as<int64_t>();
    cols = rows + n;
    h2d(in.p, hin.data(), (size_t)2 * n * 8, st);
}

PairList::~PairList() {
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
}

void PairList::plan_groups() { plan(*this, ChunkCut{}, 0); }

void PairList::plan_units() { plan(*this, ChunkCut{}, n); }   // a chunk holds a pair at least

void PairList::plan_segment_units(const gdist_sets* r, const gdist_sets* s, double codes) {
    const int64_t budget = pl_budget(codes, ctx->cus);
    plan(*this, SegmentCut{cols, r->off.as<int64_t>(), s->off.as<int64_t>(), s->nseg, budget},
         pl_unit_cap(n, codes, budget));
}

void PairList::finish() {
    hipStream_t st = ctx->stream;
    if (timed) GD_HIP(hipEventRecord(ev[1], st));
    std::vector<char> hout(out.bytes);
    d2h(hout.data(), out.p, out.bytes, st);
    float ms = -1.0f;
    if (timed) GD_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    const auto* hc = reinterpret_cast<const unsigned long long*>(hout.data());
    ctx->pairs_kernel_ms = ms;
    ctx->pairs_groups = (int64_t)hc[0];
    ctx->pairs_units = ucap ? (int64_t)hc[1] : n;   // no units: a wave's worth of work a pair
    if (I_out) std::memcpy(I_out, hout.data() + i_at, (size_t)n * 4);
    if (D_out) std::memcpy(D_out, hout.data() + d_at, (size_t)n * 8);
}

}  // namespace gdist
