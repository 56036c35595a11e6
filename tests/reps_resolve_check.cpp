// reps_resolve_check.cpp — csrc/reps_resolve.hpp against a brute-force loop.
// A stand-alone host program (tests/test_reps_resolve.py compiles it with
// -fsanitize=address,undefined): a random symmetric distance matrix is walked
// in row blocks the way sketch_reps.hip walks it, the device's two answers
// (cov[] of the earlier blocks' representatives, the closest representative)
// computed here by plain loops, and the result compared with the sequential
// definition of gdist_greedy_reps over the whole matrix.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "reps_resolve.hpp"

namespace {

int failures = 0, checks = 0;

void expect(bool ok, const char* what, int64_t n, int64_t B, double t) {
    checks++;
    if (ok) return;
    failures++;
    std::printf("FAIL %s: n=%lld B=%lld t=%g\n", what, (long long)n, (long long)B, t);
}

// the definition: sets in index order, a representative unless an earlier one has d <= t
std::vector<int32_t> brute_reps(const std::vector<double>& D, int64_t n, double t) {
    std::vector<int32_t> is_rep(n, 0);
    for (int64_t k = 0; k < n; k++) {
        bool covered = false;
        for (int64_t r = 0; r < k && !covered; r++) covered = is_rep[r] && D[k * n + r] <= t;
        is_rep[k] = !covered;
    }
    return is_rep;
}

// the walk of sketch_reps.hip with the device's parts as loops
void walk(const std::vector<double>& D, int64_t n, int64_t B, double t, const std::vector<int64_t>& rank) {
    const std::vector<int32_t> want = brute_reps(D, n, t);
    std::vector<int32_t> is_rep(n, -7);
    std::vector<int64_t> reps;
    for (int64_t b0 = 0; b0 < n; b0 += B) {
        const int64_t nb = std::min(n, b0 + B) - b0;
        std::vector<int32_t> cov(nb, 0);
        std::vector<double> tile((size_t)nb * nb);
        std::vector<int64_t> fresh(nb, -1);
        for (int64_t k = 0; k < nb; k++) {
            for (int64_t r : reps) cov[k] |= D[(b0 + k) * n + r] <= t;
            // the upper triangle only, as the device fills it; the rest is poison that
            // would cover everything if it were read
            for (int64_t j = 0; j < nb; j++) tile[k * nb + j] = j > k ? D[(b0 + k) * n + b0 + j] : -1.0;
        }
        const int64_t added = gdist::reps_resolve_block(b0, nb, cov.data(), tile.data(), t, is_rep.data(),
                                                        fresh.data());
        for (int64_t a = 0; a < added; a++) {
            expect(fresh[a] >= b0 && fresh[a] < b0 + nb && (a == 0 || fresh[a] > fresh[a - 1]), "new reps ascending",
                   n, B, t);
            reps.push_back(fresh[a]);
        }
    }
    expect(is_rep == want, "is_rep", n, B, t);
    int64_t count = 0;
    for (int64_t k = 0; k < n; k++) count += want[k];
    expect((int64_t)reps.size() == count, "rep count", n, B, t);
    // pass 2: the closest representative by (d, rank), d < 1.0, as the device kernel
    std::vector<int64_t> rep_of(n, -9);
    std::vector<double> rep_d(n, -9.0);
    for (int64_t b0 = 0; b0 < n; b0 += B) {
        const int64_t nb = std::min(n, b0 + B) - b0;
        std::vector<int64_t> best(nb);
        std::vector<double> best_d(nb);
        for (int64_t k = 0; k < nb; k++) {
            int64_t bi = -1, br = std::numeric_limits<int64_t>::max();
            double bd = 1.0;
            for (int64_t r : reps) {
                const double d = D[(b0 + k) * n + r];
                if (d < bd || (d == bd && d < 1.0 && rank[r] < br)) { bd = d; br = rank[r]; bi = r; }
            }
            best[k] = bi;
            best_d[k] = bd;
        }
        gdist::reps_assign_block(b0, nb, is_rep.data(), best.data(), best_d.data(), rep_of.data(), rep_d.data());
        gdist::reps_assign_block(b0, nb, is_rep.data(), best.data(), best_d.data(), nullptr, nullptr);
    }
    bool ok = true;
    for (int64_t k = 0; k < n && ok; k++) {
        if (want[k]) {
            ok = rep_of[k] == k && rep_d[k] == 0.0;
            continue;
        }
        int64_t bi = -1;
        double bd = 1.0;
        for (int64_t r = 0; r < n; r++) {
            if (!want[r]) continue;
            const double d = D[k * n + r];
            if (!(d < 1.0)) continue;
            if (bi < 0 || d < bd || (d == bd && rank[r] < rank[bi])) { bi = r; bd = d; }
        }
        ok = rep_of[k] == bi && rep_d[k] == (bi < 0 ? 1.0 : bd);
    }
    expect(ok, "assignment", n, B, t);
}

}  // namespace

int main() {
    std::mt19937_64 rng(12345);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t n : {1, 2, 3, 7, 33, 70}) {
        // distances on a grid of 1/8 (so ties at t and between representatives
        // occur), some NaN, some 1.0; symmetric, 0 on the diagonal
        std::vector<double> D((size_t)n * n, 0.0);
        for (int64_t i = 0; i < n; i++)
            for (int64_t j = i + 1; j < n; j++) {
                const unsigned v = (unsigned)(rng() % 12);
                D[i * n + j] = D[j * n + i] = v == 11 ? nan : v >= 8 ? 1.0 : v / 8.0;
            }
        std::vector<int64_t> index(n), reversed(n);
        for (int64_t i = 0; i < n; i++) { index[i] = i; reversed[i] = n - 1 - i; }
        // t = -1: no row covered; 0.375: a distance that occurs (ties at t);
        // 1.0: everything but NaN covers; +inf likewise (NaN <= inf is false)
        for (double t : {-1.0, 0.0, 0.375, 0.4, 1.0, std::numeric_limits<double>::infinity()})
            for (int64_t B : {(int64_t)1, (int64_t)2, (int64_t)5, (int64_t)32, n, n + 3}) {   // 5, 32: ragged last block
                walk(D, n, B, t, index);
                walk(D, n, B, t, reversed);
            }
        // every row covered by set 0: all distances 0
        std::vector<double> Z((size_t)n * n, 0.0);
        for (int64_t B : {(int64_t)1, (int64_t)2, (int64_t)5}) walk(Z, n, B, 0.0, index);
    }
    std::printf("reps_resolve_check: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
