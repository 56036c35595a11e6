// Stand-alone check of balanced_bounds (genome.distance_amd/csrc/sparse_bounds.hpp):
// host code only, built by tests/test_sparse_bounds.py with
// -fsanitize=address,undefined. Prints one line per failed check and exits 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sparse_bounds.hpp"

using gdist::balanced_bounds;
using gdist::kCostGranule;
using gdist::range_cost;

static int failures = 0;
static void fail(const std::string& name, const char* what, long long a = 0, long long b = 0) {
    std::printf("FAIL %s: %s (%lld, %lld)\n", name.c_str(), what, a, b);
    failures++;
}

struct Profile {
    const char* name;
    int64_t Ws;
    std::vector<double> cost;
};

static Profile make(const char* name, int64_t Ws, int kind) {
    Profile p{name, Ws, std::vector<double>((size_t)((Ws + kCostGranule - 1) / kCostGranule), 0.0)};
    const int64_t G = (int64_t)p.cost.size();
    for (int64_t g = 0; g < G; g++) {
        const int64_t words = std::min<int64_t>(kCostGranule, Ws - g * kCostGranule);
        double c = 1275.0 * (double)words;                       // z = 51: z (z - 1) / 2 a word
        if (kind == 1 && g >= G - (G + 19) / 20) c *= 20.0;      // the last 5 % of the granules 20 x heavier
        if (kind == 2 && g == G / 3) c *= 1.0e6;                 // one huge granule
        if (kind == 3) c = 0.0;                                  // nothing to balance
        p.cost[(size_t)g] = c;
    }
    return p;
}

int main() {
    const int64_t cap = 1015;
    std::vector<Profile> profiles;
    for (int64_t Ws : {int64_t(62500), int64_t(4099), int64_t(37)}) {
        profiles.push_back(make("flat", Ws, 0));
        profiles.push_back(make("heavy_tail", Ws, 1));
        profiles.push_back(make("huge_granule", Ws, 2));
        profiles.push_back(make("zero", Ws, 3));
    }
    int cases = 0;
    for (const Profile& p : profiles) {
        const int64_t G = (int64_t)p.cost.size();
        double total = 0.0, gmax = 0.0;
        for (double c : p.cost) { total += c; gmax = std::max(gmax, c); }
        for (int64_t n : {int64_t(1), int64_t(2), int64_t(7), int64_t(62), G + 5}) {
            for (int64_t slabs : {int64_t(0), int64_t(2), n}) {
                for (int pred = 0; pred < 2; pred++) {
                    // pred 0: every long range is exact (the cap never binds);
                    // pred 1: every range longer than the cap is refused
                    std::vector<std::pair<int64_t, int64_t>> refused;
                    auto exact = [&](int64_t b0, int64_t b1, int64_t c) {
                        if (b1 - b0 <= cap) fail(p.name, "predicate asked about a range within the cap", b0, b1);
                        if (c < 0) fail(p.name, "negative chunk index", c);
                        if (pred == 0) return true;
                        refused.push_back({b0, b1});
                        return false;
                    };
                    const std::vector<int32_t> b = balanced_bounds(p.cost, p.Ws, n, slabs, cap, exact);
                    const std::string name = std::string(p.name) + " Ws " + std::to_string(p.Ws) + " n " +
                                             std::to_string(n) + " slabs " + std::to_string(slabs) + " pred " +
                                             std::to_string(pred);
                    cases++;
                    const int64_t want = std::max<int64_t>(std::max(n, slabs), 1);
                    const int64_t got = (int64_t)b.size() - 1;
                    if (b.front() != 0 || b.back() != p.Ws) fail(name, "bounds do not cover [0, Ws]", b.front(), b.back());
                    bool mono = true, longer = false;
                    for (size_t k = 0; k + 1 < b.size(); k++) {
                        mono = mono && (want <= p.Ws ? b[k] < b[k + 1] : b[k] <= b[k + 1]);   // more chunks than words: empty ones
                        longer = longer || b[k + 1] - b[k] > cap;
                    }
                    if (!mono) fail(name, "bounds not increasing");
                    if (pred == 0 && got != want) fail(name, "chunk count differs from the one asked", got, want);
                    if (pred == 1 && got < want) fail(name, "fewer chunks than asked", got, want);
                    if (pred == 1 && got > want && refused.empty()) fail(name, "more chunks without a refusal", got, want);
                    if (pred == 1 && longer) fail(name, "a refused long range was not split to the cap");
                    if (got < slabs) fail(name, "fewer chunks than fold slabs", got, slabs);
                    // equal cost to within a granule, wherever no split was forced
                    if (refused.empty()) {
                        double mx = 0.0;
                        for (size_t k = 0; k + 1 < b.size(); k++) mx = std::max(mx, range_cost(p.cost, p.Ws, b[k], b[k + 1]));
                        const double mean = total / (double)got;
                        if (mx > mean + gmax * (1.0 + 1e-9))
                            fail(name, "max chunk cost above mean + a granule (x 1000)", (long long)(mx * 1e3 / (mean + gmax)));
                    }
                }
            }
        }
    }
    // the heavy tail moves the bounds: with equal counts the last of 62 chunks
    // would hold 1 / 62 of the words and ~ 10 x the mean cost
    {
        const Profile p = make("heavy_tail", 62500, 1);
        auto yes = [](int64_t, int64_t, int64_t) { return true; };
        const std::vector<int32_t> b = balanced_bounds(p.cost, p.Ws, 62, 0, cap, yes);
        const std::vector<int32_t> e = gdist::equal_count_bounds(p.Ws, 62);
        if (b == e) fail("heavy_tail", "balanced bounds equal the equal-count ones");
        if (!(b[61] > e[61])) fail("heavy_tail", "the last chunk did not shrink", b[61], e[61]);
    }
    // weighted chunks (the plan's taper): chunk k holds weight[k] / sum of the
    // total to within a granule; a weight list of another length is ignored
    {
        const Profile p = make("heavy_tail", 62500, 1);
        auto yes = [](int64_t, int64_t, int64_t) { return true; };
        double total = 0.0, gmax = 0.0;
        for (double c : p.cost) { total += c; gmax = std::max(gmax, c); }
        const int n = 48;
        std::vector<double> w;
        for (int k = 0; k < n; k++) w.push_back(1.8 - 1.6 * k / (n - 1));
        const std::vector<int32_t> b = balanced_bounds(p.cost, p.Ws, n, 2, cap, yes, w);
        if ((int)b.size() != n + 1 || b.front() != 0 || b.back() != p.Ws) fail("weighted", "count or cover");
        for (int k = 0; k < n && (int)b.size() == n + 1; k++) {
            if (b[k] >= b[k + 1]) fail("weighted", "bounds not increasing", k);
            const double c = range_cost(p.cost, p.Ws, b[k], b[k + 1]), want = total * w[k] / (double)n;   // mean weight 1
            if (c > want + gmax * (1.0 + 1e-9) || c < want - gmax * (1.0 + 1e-9)) fail("weighted", "chunk cost off its share", k);
        }
        w.pop_back();
        if (balanced_bounds(p.cost, p.Ws, n, 2, cap, yes, w) != balanced_bounds(p.cost, p.Ws, n, 2, cap, yes))
            fail("weighted", "a weight list of the wrong length changed the bounds");
    }
    // granule costs from z
    {
        const std::vector<int32_t> z{3, 0, 1, 10};
        const std::vector<double> c = gdist::sparse_granule_costs(z.data(), 4);
        if (c.size() != 1 || c[0] != 3.0 + 0.0 + 0.0 + 45.0) fail("granule_costs", "wrong sum");
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
