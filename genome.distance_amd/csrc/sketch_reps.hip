// sketch_reps.hip — greedy representative selection on a sketch collection
// (gdist_sketch_greedy_reps). The contract is gdist_greedy_reps's
// (DistanceRepsProcessor.java:185-200 and :227-237) with d the sketch
// distance, bit for bit gdist_sketch_matrix's cell under the same flags.
//
// Device state: rep_idx, the representatives chosen so far, compact, in
// selection order (int64[N], R of them).
//
// Pass 1, per row block [b0, b1): the ring kernel over a column list
// (sketch.hip, sketch_matrix_cols) fills D1[nb][R], the block's rows against
// the representatives only; cover_cols_kernel flags the rows one of them
// covers; sketch_matrix fills the upper triangle of the in-block tile
// [b0, b1)^2 (the distance is symmetric bit for bit), downloaded dense;
// the host resolves the block's order (reps_resolve.hpp) and the new
// representatives are appended to rep_idx. No distance to an earlier set that
// is not a representative is computed: N (R + B / 2) cells at most where reps.hip's
// scheme (every earlier set) would merge N^2 / 2 pairs.
//
// Pass 2 (rep_of / rep_dist asked for): every block against the final list
// through the same launch; argmin_cols_kernel takes the least (d, tie rank)
// over the representatives with d < 1.0, closest_rep_kernel's rule (reps.hip).
//
// A gathered or replicated collection is answered whole on every rank.
#include <algorithm>
#include <vector>

#include "gdist_internal.hpp"
#include "reps_resolve.hpp"

namespace gdist {
namespace {

// cov[k] = 1 if some column c < ncols has D[k][c] <= t (one wave per row);
// NaN compares false
__global__ __launch_bounds__(256) void cover_cols_kernel(const double* __restrict__ D, int64_t ldD, int64_t nrows,
                                                         int64_t ncols, double t, int32_t* __restrict__ cov) {
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= nrows) return;
    const double* row = D + k * ldD;
    bool hit = false;
    for (int64_t c = lane; c < ncols && !hit; c += 64) hit = row[c] <= t;
    const unsigned long long any = __ballot(hit);
    if (lane == 0) cov[k] = any != 0ull;
}

// closest representative of each row: min (d, rank) over the columns with
// d < 1.0, column c the set rep_idx[c], its rank rank[rep_idx[c]] (null: the
// set index); best[k] = that set, -1 / 1.0 when none (one wave per row)
__global__ __launch_bounds__(256) void argmin_cols_kernel(const double* __restrict__ D, int64_t ldD, int64_t nrows,
                                                          int64_t ncols, const int64_t* __restrict__ rep_idx,
                                                          const int64_t* __restrict__ rank,
                                                          int64_t* __restrict__ best, double* __restrict__ best_d) {
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= nrows) return;
    const double* row = D + k * ldD;
    double bd = 1.0;
    int64_t br = INT64_MAX, bi = -1;
    for (int64_t c = lane; c < ncols; c += 64) {
        const double d = row[c];
        const int64_t g = rep_idx[c];
        const int64_t rk = rank ? rank[g] : g;
        if (d < bd || (d == bd && d < 1.0 && rk < br)) { bd = d; br = rk; bi = g; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o, 64);
        const int64_t orr = __shfl_xor(br, o, 64), oi = __shfl_xor(bi, o, 64);
        if (od < bd || (od == bd && orr < br)) { bd = od; br = orr; bi = oi; }
    }
    if (lane == 0) {
        best[k] = bi;
        best_d[k] = bi < 0 ? 1.0 : bd;
    }
}

}  // namespace

void sketch_greedy_reps(gdist_ctx* ctx, const gdist_sets* sk, double t, unsigned flags, const int64_t* tie_rank,
                        int32_t* is_rep, int64_t* rep_of, double* rep_dist, int64_t* nreps) {
    hipStream_t st = ctx->stream;
    const int64_t n = sk->nsets;
    int64_t* info = ctx->reps_info;
    // row block: reps.hip's rule, B x N distances within its budget, so the
    // representatives' columns of a block never need chunking
    int64_t B = std::max<int64_t>(128, std::min<int64_t>(4096, ((int64_t(1) << 27) / n) / 128 * 128));
    B = std::min<int64_t>(B, ceil_div(n, 128) * 128);
    if (ctx->has_option(OPT_REPS_BLOCK)) B = std::max<int64_t>(1, ctx->option(OPT_REPS_BLOCK, B));
    B = std::min(B, n);
    DevBuf drep(n * 8 + 8, st), dcov(B * 4 + 4, st), dtile((size_t)B * B * 8 + 8, st), dD1;
    int64_t cap = 0;   // columns D1 holds: grown with the list, never past n
    auto room = [&](int64_t R) {
        if (R <= cap) return;
        cap = std::min(n, std::max<int64_t>(2 * R, 256));
        dD1.alloc((size_t)B * cap * 8 + 8, st);
    };
    std::vector<int32_t> cov(B);
    std::vector<double> tile((size_t)B * B);
    std::vector<int64_t> fresh(B);
    int64_t R = 0;
    for (int64_t b0 = 0; b0 < n; b0 += B) {
        const int64_t b1 = std::min(n, b0 + B), nb = b1 - b0;
        std::fill(cov.begin(), cov.begin() + nb, 0);
        if (R > 0) {
            room(R);
            info[3] += sketch_matrix_cols(ctx, sk, b0, b1, drep.as<int64_t>(), R, flags, nullptr, dD1.as<double>(), R);
            info[1] += nb * R;
            cover_cols_kernel<<<(unsigned)ceil_div(nb, 4), 256, 0, st>>>(dD1.as<double>(), R, nb, R, t,
                                                                         dcov.as<int32_t>());
            GD_HIP(hipGetLastError());
        }
        // the in-block tile, dense on the device, one linear download (reps.hip);
        // its upper triangle only: d(k, j) for j < k is read as d(j, k)
        sketch_matrix(ctx, sk, b0, b1, b0, b1, flags | GDIST_UPPER_TRIANGLE, nullptr, dtile.as<double>(), nb);
        if (R > 0) d2h(cov.data(), dcov.p, nb * 4, st);
        d2h(tile.data(), dtile.p, (size_t)nb * nb * 8, st);
        const int64_t added = reps_resolve_block(b0, nb, cov.data(), tile.data(), t, is_rep, fresh.data());
        h2d(drep.as<int64_t>() + R, fresh.data(), added * 8, st);
        R += added;
        info[0]++;
    }
    if (nreps) *nreps = R;
    if (!rep_of && !rep_dist) return;
    DevBuf drank, dbest(B * 8 + 8, st), dbd(B * 8 + 8, st);
    if (tie_rank) {
        drank.alloc(n * 8, st);
        h2d(drank.p, tie_rank, n * 8, st);
    }
    std::vector<int64_t> hb(B);
    std::vector<double> hd(B);
    room(R);
    for (int64_t b0 = 0; b0 < n; b0 += B) {
        const int64_t b1 = std::min(n, b0 + B), nb = b1 - b0;
        info[3] += sketch_matrix_cols(ctx, sk, b0, b1, drep.as<int64_t>(), R, flags, nullptr, dD1.as<double>(), R);
        info[2] += nb * R;
        argmin_cols_kernel<<<(unsigned)ceil_div(nb, 4), 256, 0, st>>>(
            dD1.as<double>(), R, nb, R, drep.as<int64_t>(), tie_rank ? drank.as<int64_t>() : nullptr,
            dbest.as<int64_t>(), dbd.as<double>());
        GD_HIP(hipGetLastError());
        d2h(hb.data(), dbest.p, nb * 8, st);
        d2h(hd.data(), dbd.p, nb * 8, st);
        reps_assign_block(b0, nb, is_rep, hb.data(), hd.data(), rep_of, rep_dist);
    }
}

}  // namespace gdist
