// sketch_cross.hip — query sketches against a resident sketch collection
// (gdist_cross_* on two GDIST_SKETCH collections).
//
// The request is the reference's getClosest per incoming genome
// (FindProcessor.java:94-110, MashProcessor.java:150) on a MinHash database:
// one or a few tens of query rows against 10^4 .. 10^6 subjects of width
// ~1000. sketch.hip's kernels give a lane a pair (about 2 s dependent steps at
// data-dependent addresses); one query row leaves them 1 lane in 32. Here a
// WAVE takes a pair and its 64 lanes merge 64 segments of it
// (skx_pair_merge, sketch_wave_merge.hpp): ~2 s / 64 steps and a binary search
// a lane.
//
// sketch_cross_kernel: a workgroup of 16 waves owns a run of `st` consecutive
// subjects of the step's columns and meets them with EVERY query row of the
// step's row block, so a subject is read from HBM once a step.
//   LDS variant: the run's signatures, consecutive in the collection's CSR,
//   are staged once as they lie (one flat coalesced copy by the whole
//   workgroup), then the query rows pass through in tiles of kQT, staged the
//   same way; the waves take the tile's (query, subject) pairs in turn. The
//   merge is a chain of dependent LDS reads, so what hides its latency is
//   waves: two workgroups a CU are 8 waves a SIMD.
//   Global variant (a run of kMinRun signatures and the query tile past the
//   LDS budget): the same walk, searching and merging straight from global
//   memory.
// Lane 0 stores the pair's common count and / or distance: plain stores into
// the step's block, row stride nk.
#include "gdist_internal.hpp"
#include "sketch_wave_merge.hpp"

namespace gdist {
namespace {

constexpr int kNT = 1024, kNW = kNT / 64;  // threads, waves of a workgroup
constexpr int kQT = 4;                     // query rows staged at a time
constexpr int kMinRun = 4, kMaxRun = 64;   // subjects a workgroup holds
constexpr int kLdsDwords = 16000;          // 62.5 KiB of signatures: two workgroups a CU

// Sets [first, first + n) of a CSR collection into LDS as they lie: their
// hashes sig[off[first] .. off[first + n]) to dst (at most cap dwords), and
// rel[0 .. n] their bounds relative to off[first], clamped to cap. Called by
// the whole workgroup; the caller's barrier publishes both.
__device__ __forceinline__ void stage_sets(const int32_t* __restrict__ sig, const int64_t* __restrict__ off,
                                           int64_t first, int n, int cap, int32_t* dst, int32_t* rel) {
    const int64_t base = off[first];
    if ((int)threadIdx.x <= n) {
        const int64_t r = off[first + threadIdx.x] - base;
        rel[threadIdx.x] = (int32_t)(r < cap ? r : cap);
    }
    const int64_t all = off[first + n] - base;
    const int total = (int)(all < cap ? all : cap);
    const int32_t* src = sig + base;
    constexpr int U = 4;   // loads in flight a thread
    for (int i0 = threadIdx.x; i0 < total; i0 += kNT * U) {
        int32_t v[U];
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = i0 + u * kNT < total ? src[i0 + u * kNT] : 0;
#pragma unroll
        for (int u = 0; u < U; u++)
            if (i0 + u * kNT < total) dst[i0 + u * kNT] = v[u];
    }
}

// Query rows [b0, b0 + nb) of (qsig, qoff) against subject columns
// [k0, k0 + nk) of (ssig, soff); workgroup g owns columns [k0 + g st,
// k0 + (g + 1) st), st <= kMaxRun. common_out / D: [nb][nk], either may be
// null. LDS: sm holds (st + kQT) sw dwords, the subjects' first.
template <bool LDS>
__global__ __launch_bounds__(kNT) void sketch_cross_kernel(
    const int32_t* __restrict__ qsig, const int64_t* __restrict__ qoff, const int32_t* __restrict__ ssig,
    const int64_t* __restrict__ soff, int width, int sw, int st, int64_t b0, int64_t nb, int64_t k0, int64_t nk,
    int jaccard, int empty_nan, int32_t* __restrict__ common_out, double* __restrict__ D) {
    extern __shared__ int32_t sm[];
    __shared__ int32_t s_rel[kMaxRun + 1], q_rel[kQT + 1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t j0 = (int64_t)blockIdx.x * st;          // relative to k0
    if (j0 >= nk) return;
    const int run = (int)(nk - j0 < st ? nk - j0 : st);   // <= kMaxRun
    int32_t* qm = sm + st * sw;

    if (LDS) stage_sets(ssig, soff, k0 + j0, run, st * sw, sm, s_rel);
    const int64_t tile = LDS ? kQT : nb;
    for (int64_t t0 = 0; t0 < nb; t0 += tile) {
        const int nq = (int)(nb - t0 < tile ? nb - t0 : tile);
        if (LDS) {
            __syncthreads();   // the previous tile's pairs are done with the query rows
            stage_sets(qsig, qoff, b0 + t0, nq, kQT * sw, qm, q_rel);
            __syncthreads();
        }
        const int npairs = nq * run;
        for (int p = wave; p < npairs; p += kNW) {
            const int r = p / run, s = p - r * run;
            const int32_t *Q, *S;
            int lq, ls;
            if (LDS) {
                Q = qm + q_rel[r];
                S = sm + s_rel[s];
                lq = q_rel[r + 1] - q_rel[r];
                ls = s_rel[s + 1] - s_rel[s];
            } else {
                const int64_t qb = qoff[b0 + t0 + r], sb = soff[k0 + j0 + s];
                Q = qsig + qb;
                S = ssig + sb;
                lq = (int)(qoff[b0 + t0 + r + 1] - qb);
                ls = (int)(soff[k0 + j0 + s + 1] - sb);
            }
            int common;
            double d;
            skx_pair_merge(Q, lq, S, ls, width, jaccard, empty_nan, lane, &common, &d);
            if (lane == 0) {
                const int64_t o = (t0 + r) * nk + j0 + s;
                if (common_out) common_out[o] = common;
                if (D) D[o] = d;
            }
        }
    }
}

}  // namespace

SketchCrossSource::SketchCrossSource(gdist_ctx* c, const gdist_sets* queries, const gdist_sets* subjects,
                                     unsigned flags)
    : ctx(c), q(queries), s(subjects), jaccard((flags & GDIST_SKETCH_JACCARD) ? 1 : 0) {
    from_counts = false;
    empty_nan = (flags & GDIST_EMPTY_NAN) ? 1 : 0;
    nrsets = q->nsets;
    ncsets = s->nsets;
    timed = ctx->option(OPT_TIME_KERNELS, 0) != 0;
}

void SketchCrossSource::fill(int64_t b0, int64_t b1, int64_t k0, int64_t k1, void* blk) {
    const int64_t nb = b1 - b0, nk = k1 - k0;
    if (nb <= 0 || nk <= 0) return;
    // no signature is longer than the width (uploads are validated, built
    // sketches are cut), so a run of st fits st sw dwords as it lies
    const int width = std::max(1, s->width), sw = width;
    // enough workgroups for four a CU before a run grows past kMinRun subjects
    const int64_t spread = std::max<int64_t>(kMinRun, ceil_div(nk, (int64_t)4 * std::max(ctx->cus, 1)));
    const int64_t fit = (int64_t)kLdsDwords / sw - kQT;
    const bool lds = fit >= kMinRun;
    const int st = (int)std::min<int64_t>(spread, lds ? std::min<int64_t>(fit, kMaxRun) : kMinRun);
    const unsigned grid = (unsigned)ceil_div(nk, st);
    // cross_matrix: the counts into the block and D beside it; else D is the block
    int32_t* dc = matrix ? (want_common ? static_cast<int32_t*>(blk) : nullptr) : nullptr;
    double* dd = matrix ? d_to : static_cast<double*>(blk);
    if (lds) {
        const size_t bytes = (size_t)(st + kQT) * sw * 4;
        sketch_cross_kernel<true><<<grid, kNT, bytes, ctx->stream>>>(
            q->codes.as<int32_t>(), q->off.as<int64_t>(), s->codes.as<int32_t>(), s->off.as<int64_t>(), width, sw, st,
            b0, nb, k0, nk, jaccard, empty_nan, dc, dd);
    } else {
        sketch_cross_kernel<false><<<grid, kNT, 0, ctx->stream>>>(
            q->codes.as<int32_t>(), q->off.as<int64_t>(), s->codes.as<int32_t>(), s->off.as<int64_t>(), width, sw, st,
            b0, nb, k0, nk, jaccard, empty_nan, dc, dd);
    }
    GD_HIP(hipGetLastError());
    pairs += nb * nk;
}

void SketchCrossSource::report() const {
    ctx->cross_units = pairs;
    if (timed) {
        ctx->cross_join_ms = fill_ms;
        ctx->cross_select_ms = matrix ? 0.0 : consume_ms;
    }
}

}  // namespace gdist
