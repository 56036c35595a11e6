// closest.hip — exact nearest-neighbour query on the device (gdist_closest).
//
// getClosest(kmers, n, maxDist) (MashProcessor.java:150, FindProcessor.java:110)
// answered exhaustively: for every query row the n smallest (d, column) among
// the columns with d <= max_dist. The driver walks row blocks x column chunks
// in ascending column order; per step the matrix kernels leave the block's
// intersection counts I (kmer sets) or distances D (sketches) in device
// memory and closest_select_kernel folds them into the rows' running lists,
// so neither I nor D leaves HBM and for kmer sets D is never written.
//
// A list entry is a 96-bit key: the fp64 bits of d (d is in [0, 1] and never
// -0.0, so the unsigned bit pattern orders it) and the u32 global column.
// One wave owns one row. Its LDS region holds 2 L keys, L = max(128, the next
// power of two >= n): the sorted list in [0, L) and a staging area in
// [L, 2 L). Candidates passing d <= tau are compacted into staging; when
// staging cannot take another 64, and at the end of the chunk, the 2 L keys
// are bitonic-sorted, the first n kept, and tau drops to the n-th best d.
// (L >= 128: staging takes a full wave of candidates and then some, so a
// merge is paid once per 65+ survivors, not once per 64 columns that hold one.)
// Once the list is full a candidate must have d < tau: a later column with
// d == tau loses the (d, column) tie against every listed one because the
// chunks arrive in ascending column order. The lists persist between chunks
// in a device state buffer; the last chunk's launch writes idx / d / count.
#include <algorithm>

#include "gdist_internal.hpp"

namespace gdist {
namespace {

constexpr unsigned long long kNoKey = ~0ull;   // a NaN pattern: no distance has it; sorts last

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ascending bitonic sort of the T keys (kd, kc) of one wave (T a power of two >= 128)
__device__ __forceinline__ void wave_sort(unsigned long long* kd, uint32_t* kc, int T, int lane) {
    for (int k = 2; k <= T; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (T >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const bool up = (i & k) == 0;
                const unsigned long long da = kd[i], db = kd[p];
                const uint32_t ca = kc[i], cb = kc[p];
                const bool gt = da > db || (da == db && ca > cb);
                if (gt == up) {
                    kd[i] = db; kd[p] = da;
                    kc[i] = cb; kc[p] = ca;
                }
            }
            wave_sync();
        }
    }
}

// Rows [q0, q0 + nrows) against the chunk's columns [c0, c0 + nc).
//  FromCounts: src is I (int32, row a / column b at src[a * ld + b]) and d is
//  the Java expression of epilogue_kernel (matrix_step.hip), fp64, no contraction,
//  with the row's size from roff and the column's from coff (one collection:
//  the same array; gdist_cross_closest: the queries' and the subjects');
//  else src is D (double, the same layout).
// State per row: st_n (list length), st_d / st_c (L keys). `last`: write the
// block's outputs (idx / d: [nrows][n], count: [nrows]).
template <bool FromCounts>
__global__ __launch_bounds__(256) void closest_select_kernel(
    const void* __restrict__ src, int64_t ld, const int64_t* __restrict__ roff, const int64_t* __restrict__ coff,
    int empty_nan, int64_t q0,
    int64_t nrows, int64_t c0, int64_t nc, int keep_self, int n, int L, double max_dist,
    unsigned long long* __restrict__ st_d, uint32_t* __restrict__ st_c, int32_t* __restrict__ st_n, int last,
    int64_t* __restrict__ idx_out, double* __restrict__ d_out, int32_t* __restrict__ count_out) {
#pragma clang fp contract(off)
    extern __shared__ unsigned long long closest_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t a = (int64_t)blockIdx.x * 4 + wave;
    if (a >= nrows) return;   // no workgroup barrier below: a wave may leave alone
    const int T = 2 * L;
    unsigned long long* kd = closest_lds + (size_t)wave * T;
    uint32_t* kc = reinterpret_cast<uint32_t*>(closest_lds + (size_t)4 * T) + (size_t)wave * T;

    int cnt = st_n[a];
    for (int i = lane; i < L; i += 64) {
        const bool held = i < cnt;
        kd[i] = held ? st_d[a * L + i] : kNoKey;
        kc[i] = held ? st_c[a * L + i] : ~0u;
    }
    wave_sync();
    bool full = cnt == n;
    double tau = full ? __longlong_as_double((long long)kd[n - 1]) : max_dist;
    int ns = 0;   // staged candidates

    const int64_t q = q0 + a;
    int64_t na = 0;
    if (FromCounts) na = roff[q + 1] - roff[q];
    const int32_t* Ir = static_cast<const int32_t*>(src) + a * ld;
    const double* Dr = static_cast<const double*>(src) + a * ld;

    constexpr int U = 4;   // 64-column steps whose loads are in flight together
    for (int64_t g0 = 0; g0 < nc; g0 += 64 * U) {
        double dv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t b = g0 + u * 64 + lane;
            double d = __builtin_nan("");   // past the ragged end: never qualifies
            if (b < nc) {
                if (FromCounts) {
                    const int64_t j = c0 + b;
                    const int64_t inter = Ir[b];
                    const int64_t nb = coff[j + 1] - coff[j];
                    if (inter > 0) {
                        const double uni = (double)(na + nb - inter);
                        d = 1.0 - (double)inter / uni;
                    } else {
                        d = (empty_nan && na + nb == 0) ? __builtin_nan("") : 1.0;
                    }
                } else {
                    d = Dr[b];
                }
            }
            dv[u] = d;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (g0 + u * 64 >= nc) break;   // wave-uniform
            const int64_t j = c0 + g0 + u * 64 + lane;
            const double d = dv[u];
            const bool ok = (full ? d < tau : d <= tau) && (keep_self || j != q);   // NaN fails both
            const unsigned long long m = __ballot(ok);
            if (m == 0ull) continue;
            if (ok) {
                const int r = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                kd[L + ns + r] = (unsigned long long)__double_as_longlong(d);
                kc[L + ns + r] = (uint32_t)j;
            }
            ns += __popcll(m);
            if (ns + 64 > L) {
                for (int i = L + ns + lane; i < T; i += 64) { kd[i] = kNoKey; kc[i] = ~0u; }
                wave_sync();
                wave_sort(kd, kc, T, lane);
                cnt = min(n, cnt + ns);
                ns = 0;
                full = cnt == n;
                if (full) tau = __longlong_as_double((long long)kd[n - 1]);
                wave_sync();   // every lane has read tau before the list's tail is cleared
                for (int i = cnt + lane; i < L; i += 64) { kd[i] = kNoKey; kc[i] = ~0u; }
                wave_sync();
            }
        }
    }
    if (ns > 0) {
        for (int i = L + ns + lane; i < T; i += 64) { kd[i] = kNoKey; kc[i] = ~0u; }
        wave_sync();
        wave_sort(kd, kc, T, lane);
        cnt = min(n, cnt + ns);
    }
    for (int i = lane; i < cnt; i += 64) {
        st_d[a * L + i] = kd[i];
        st_c[a * L + i] = kc[i];
    }
    if (lane == 0) st_n[a] = cnt;
    if (last) {
        for (int r = lane; r < n; r += 64) {
            const bool held = r < cnt;
            idx_out[a * n + r] = held ? (int64_t)kc[r] : -1;
            d_out[a * n + r] = held ? __longlong_as_double((long long)kd[r]) : 1.0;
        }
        if (lane == 0) count_out[a] = cnt;
    }
}

}  // namespace

// Block sizes of the walk: rows a block, columns a chunk. One step's I (4 B a
// pair) or D (8 B) stays within 1 GiB, the matrix kernels' own scratch and
// the lists beside it within the ~1.5 GiB greedy_reps works in.
void closest_blocks(const gdist_ctx* ctx, int64_t nr, int64_t nc, size_t elem, int64_t* rows, int64_t* cols) {
    int64_t R = std::min<int64_t>(4096, ceil_div(std::max<int64_t>(nr, 1), 128) * 128);
    if (ctx->has_option(OPT_CLOSEST_ROWS)) R = std::max<int64_t>(1, ctx->option(OPT_CLOSEST_ROWS, R));
    R = std::min<int64_t>(R, std::max<int64_t>(nr, 1));
    int64_t W = std::max<int64_t>(128, ((int64_t(1) << 30) / (int64_t)elem / R) / 128 * 128);
    if (ctx->has_option(OPT_CLOSEST_COLS)) W = std::max<int64_t>(1, ctx->option(OPT_CLOSEST_COLS, W));
    W = std::min<int64_t>(W, std::max<int64_t>(nc, 1));
    *rows = R;
    *cols = W;
}

SelfSource::SelfSource(gdist_ctx* c, const gdist_sets* sets, int m, unsigned flags)
    : ctx(c), s(sets), method(m), mflags(flags & (GDIST_EMPTY_NAN | GDIST_SKETCH_JACCARD)) {
    from_counts = s->kind != GDIST_SKETCH;
    keep_self = (flags & GDIST_CLOSEST_KEEP_SELF) ? 1 : 0;
    upper = (flags & GDIST_UPPER_TRIANGLE) ? 1 : 0;
    empty_nan = (flags & GDIST_EMPTY_NAN) ? 1 : 0;
    roff = coff = from_counts ? s->off.as<int64_t>() : nullptr;
    nrsets = ncsets = s->nsets;
    timed = ctx->option(OPT_TIME_KERNELS, 0) != 0;
}

void SelfSource::fill(int64_t b0, int64_t b1, int64_t k0, int64_t k1, void* blk) {
    const int64_t nk = k1 - k0;
    if (!from_counts) {
        sketch_matrix(ctx, s, b0, b1, k0, k1, mflags, nullptr, static_cast<double*>(blk), nk);
    } else if (method == GDIST_METHOD_BITSET) {
        zero_counts(ctx, b0, b1, k0, k1, false, static_cast<int32_t*>(blk), nk);
        bitset_matrix(ctx, s, b0, b1, k0, k1, false, static_cast<int32_t*>(blk), nk);
    } else {
        sorted_matrix(ctx, s, b0, b1, k0, k1, false, static_cast<int32_t*>(blk), nk);
    }
}

// Ascending columns: the select's d < tau rule needs them. The lists are
// empty when a row block's first chunk is selected (zeroed outside the timed
// span: select_ms is the kernel's) and downloaded after its last.
void closest_select(gdist_ctx* ctx, WalkSource& src, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int n,
                    double max_dist, int64_t* idx_out, double* d_out, int32_t* count_out) {
    hipStream_t st = ctx->stream;
    int L = 128;
    while (L < n) L <<= 1;
    int64_t R, W;
    closest_blocks(ctx, r1 - r0, c1 - c0, src.elem(), &R, &W);
    Walk walk(ctx, src, R, W);
    DevBuf sd((size_t)R * L * 8 + 8, st), sc((size_t)R * L * 4 + 4, st), sn((size_t)R * 4 + 4, st);
    DevBuf oi((size_t)R * n * 8 + 8, st), od((size_t)R * n * 8 + 8, st), oc((size_t)R * 4 + 4, st);
    const size_t lds = (size_t)4 * 2 * L * 12;
    GD_HIP(hipMemsetAsync(sn.p, 0, (size_t)R * 4, st));
    walk.run(r0, r1, c0, c1, false, [&](const WalkStep& t) {
        const auto kernel = src.from_counts ? closest_select_kernel<true> : closest_select_kernel<false>;
        kernel<<<(unsigned)ceil_div(t.nb, 4), 256, lds, st>>>(
            walk.blk.p, t.nk, src.roff, src.coff, src.empty_nan, t.b0, t.nb, t.k0, t.nk, src.keep_self, n, L, max_dist,
            sd.as<unsigned long long>(), sc.as<uint32_t>(), sn.as<int32_t>(), t.last, oi.as<int64_t>(),
            od.as<double>(), oc.as<int32_t>());
        GD_HIP(hipGetLastError());
    }, [&](const WalkStep& t) {
        if (!t.last) return;
        d2h(idx_out + (t.b0 - r0) * n, oi.p, (size_t)t.nb * n * 8, st);
        d2h(d_out + (t.b0 - r0) * n, od.p, (size_t)t.nb * n * 8, st);
        d2h(count_out + (t.b0 - r0), oc.p, (size_t)t.nb * 4, st);
        if (t.b0 + t.nb < r1) GD_HIP(hipMemsetAsync(sn.p, 0, (size_t)R * 4, st));   // the next row block's
    });
}

// method: SORTED or BITSET (resolved by the caller); ignored for sketches
void closest(gdist_ctx* ctx, gdist_sets* s, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int method,
             unsigned flags, int n, double max_dist, int64_t* idx_out, double* d_out, int32_t* count_out) {
    SelfSource src(ctx, s, method, flags);
    ctx->closest_matrix_ms = ctx->closest_select_ms = -1.0;
    closest_select(ctx, src, r0, r1, c0, c1, n, max_dist, idx_out, d_out, count_out);
    // option time_kernels: the intersect (or sketch) kernels and the select
    // kernel of every step apart, HIP events on the stream (gdist_ctx_closest_timing)
    if (src.timed) {
        ctx->closest_matrix_ms = src.fill_ms;
        ctx->closest_select_ms = src.consume_ms;
    }
}

}  // namespace gdist
