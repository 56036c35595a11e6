// Stand-alone check of csrc/sketch_cross_merge.hpp (the wave-per-pair
// segmented merge of two sketch signatures): built by
// tests/test_sketch_cross_merge.py with the host compiler under
// AddressSanitizer + UBSan, no device.
//
// pair_by_lanes() does what a wave of sketch_cross_kernel does, its 64 lanes
// in a loop: the segment cut, the per-lane merge, the prefix sum of the unions
// and the capped merge of the lane that straddles the cap. Its (common, taken)
// must equal a plain two-pointer merge's for both flag settings. The
// signatures live in exactly sized vectors, so a read past either end is an
// AddressSanitizer report.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "sketch_cross_merge.hpp"

using Sig = std::vector<int32_t>;

static long checks = 0, failures = 0;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

// n distinct ascending values; span > 0: from [lo, lo + span), else any int32
static Sig random_sig(int n, int64_t lo, int64_t span) {
    std::set<int32_t> s;
    while ((int)s.size() < n) s.insert(span > 0 ? (int32_t)(lo + (int64_t)(rnd() % (uint64_t)span)) : (int32_t)rnd());
    return Sig(s.begin(), s.end());
}

struct Result {
    int common, taken;
};

// the reference: one two-pointer merge over the first `width` union elements (Mash) or all (Jaccard)
static Result plain(const Sig& a, const Sig& b, int width, int jaccard) {
    size_t i = 0, j = 0;
    int common = 0, taken = 0;
    while ((i < a.size() || j < b.size()) && (jaccard || taken < width)) {
        if (j == b.size() || (i < a.size() && a[i] < b[j])) i++;
        else if (i == a.size() || b[j] < a[i]) j++;
        else { common++; i++; j++; }
        taken++;
    }
    return Result{common, taken};
}

static Result pair_by_lanes(const Sig& q, const Sig& s, int width, int jaccard) {
    using namespace gdist;
    const bool qa = q.size() >= s.size();
    const Sig& SA = qa ? q : s;
    const Sig& SB = qa ? s : q;
    // data() of an empty vector may be null: nothing may be read through it
    const int32_t *A = SA.data(), *B = SB.data();
    const int na = (int)SA.size(), nb = (int)SB.size();
    const int ca = skx_chunk(na);
    int a0[kSkxLanes], a1[kSkxLanes], b0[kSkxLanes], b1[kSkxLanes], c[kSkxLanes], uni[kSkxLanes];
    uint64_t mask[kSkxLanes];
    int total = 0, csum = 0;
    for (int t = 0; t < kSkxLanes; t++) {
        skx_a_range(na, ca, t, &a0[t], &a1[t]);
        b0[t] = skx_b_begin(A, na, B, nb, ca, t);
        b1[t] = t + 1 < kSkxLanes ? skx_b_begin(A, na, B, nb, ca, t + 1) : nb;
        c[t] = skx_merge(A, a0[t], a1[t], B, b0[t], b1[t], &mask[t]);
        uni[t] = (a1[t] - a0[t]) + (b1[t] - b0[t]) - c[t];
        total += uni[t];
        csum += c[t];
    }
    if (jaccard) return Result{csum, skx_taken(total, width, 1)};
    const int T = skx_taken(total, width, 0);
    int common = 0, before = 0;
    for (int t = 0; t < kSkxLanes; t++) {
        common += skx_lane_common(A, a0[t], a1[t], B, b0[t], b1[t], before, uni[t], c[t], mask[t], T);
        before += uni[t];
    }
    return Result{common, T};
}

static void check_pair(const char* what, const Sig& a, const Sig& b, int width) {
    for (int jaccard = 0; jaccard < 2; jaccard++) {
        for (int swap = 0; swap < 2; swap++) {
            const Sig& x = swap ? b : a;
            const Sig& y = swap ? a : b;
            const Result want = plain(x, y, width, jaccard), got = pair_by_lanes(x, y, width, jaccard);
            checks++;
            if (want.common != got.common || want.taken != got.taken) {
                failures++;
                std::printf("FAIL %s: |a| %zu |b| %zu width %d jaccard %d: common %d taken %d, expected %d %d\n", what,
                            x.size(), y.size(), width, jaccard, got.common, got.taken, want.common, want.taken);
            }
            // the distance is a function of these alone; NaN only for two empty signatures
            const double d = gdist::skx_distance(got.common, got.taken, (int)x.size(), (int)y.size(), jaccard, 1);
            checks++;
            if ((d != d) != (x.empty() && y.empty())) {
                failures++;
                std::printf("FAIL %s: NaN mismatch\n", what);
            }
        }
    }
}

// every cap from 1 to past the union: the cap on a common element, one before
// it, one after it, on a segment's first and last element
static void sweep_caps(const char* what, const Sig& a, const Sig& b) {
    const int uni = (int)(a.size() + b.size());
    for (int w = 1; w <= uni + 1; w++) check_pair(what, a, b, w);
}

int main() {
    const int widths[] = {1, 2, 3, 63, 64, 65, 127, 128, 130, 1000};
    for (int width : widths) {
        const int lens_raw[] = {0, 1, 2, 5, width / 2, width};
        std::set<int> lens;
        for (int l : lens_raw) lens.insert(l < width ? l : width);
        // random pairs: dense values (many common elements), then any int32
        for (int la : lens)
            for (int lb : lens)
                for (int rep = 0; rep < 3; rep++) {
                    check_pair("random dense", random_sig(la, -width, 3 * (int64_t)width + 2),
                               random_sig(lb, -width, 3 * (int64_t)width + 2), width);
                    check_pair("random int32", random_sig(la, 0, 0), random_sig(lb, 0, 0), width);
                }
        // identical
        const Sig full = random_sig(width, 0, 0);
        check_pair("identical", full, full, width);
        // disjoint: all of one below all of the other (check_pair runs both orders)
        Sig low = random_sig(width, -5000000, 4000000), high = random_sig(width, 1000, 4000000);
        check_pair("disjoint", low, high, width);
        check_pair("disjoint short", Sig(low.begin(), low.begin() + (width + 1) / 2), high, width);
        // interleaved: evens against odds, and evens against multiples of three
        Sig ev, od, th;
        for (int i = 0; i < width; i++) { ev.push_back(2 * i); od.push_back(2 * i + 1); th.push_back(3 * i); }
        check_pair("interleaved", ev, od, width);
        check_pair("interleaved common", ev, th, width);
        // INT_MIN and INT_MAX are hashes like any other
        Sig ext = random_sig(width > 2 ? width - 2 : 0, 0, 0), ext2 = random_sig(width > 1 ? width - 1 : 0, 0, 0);
        {
            std::set<int32_t> s(ext.begin(), ext.end());
            s.insert(INT_MIN);
            s.insert(INT_MAX);
            while ((int)s.size() > width) s.erase(std::next(s.begin()));
            ext.assign(s.begin(), s.end());
            std::set<int32_t> s2(ext2.begin(), ext2.end());
            s2.insert(INT_MAX);
            while ((int)s2.size() > width) s2.erase(s2.begin());
            ext2.assign(s2.begin(), s2.end());
        }
        check_pair("extremes both", ext, ext, width);
        check_pair("extremes", ext, ext2, width);
        check_pair("extremes vs random", ext, full, width);
        check_pair("INT_MAX alone", Sig{INT_MAX}, ext, width);
        check_pair("INT_MIN alone", Sig{INT_MIN}, ext, width);
        check_pair("INT_MIN vs INT_MAX", Sig{INT_MIN}, Sig{INT_MAX}, width);
    }
    // na < 64 < nb, and the shorter side on either side of a lane's chunk
    for (int la : {1, 2, 5, 33, 63})
        for (int lb : {65, 100, 130, 1000}) {
            check_pair("short vs long", random_sig(la, 0, 3000), random_sig(lb, 0, 3000), 1000);
            check_pair("short vs long", random_sig(la, 0, 0), random_sig(lb, 0, 0), lb);
        }
    // the cap at every position of the union
    sweep_caps("caps 130", random_sig(130, 0, 400), random_sig(130, 0, 400));
    sweep_caps("caps 130/40", random_sig(130, 0, 400), random_sig(40, 0, 400));
    sweep_caps("caps 65/64", random_sig(65, 0, 150), random_sig(64, 0, 150));
    sweep_caps("caps 5/3", random_sig(5, 0, 8), random_sig(3, 0, 8));
    {
        Sig a = random_sig(200, 0, 500);
        sweep_caps("caps identical", a, a);
        Sig ev, th;
        for (int i = 0; i < 128; i++) { ev.push_back(2 * i); th.push_back(3 * i); }
        sweep_caps("caps interleaved", ev, th);
    }
    // long signatures: a lane's segment holds more than 64 union elements, the
    // lane that straddles the cap past them merges again
    {
        const Sig a = random_sig(4500, 0, 12000), b = random_sig(4000, 0, 12000), c = random_sig(70, 0, 12000);
        for (int w = 1; w <= 8600; w += 37) {
            check_pair("long", a, b, w);
            check_pair("long vs short", a, c, w);
        }
        for (int w = 60; w <= 70; w++) check_pair("long, cap about 64", a, b, w);
    }
    // named cap cases on a known pair: common element 30 is union element 7 (0-based)
    {
        const Sig a{0, 10, 20, 30, 40, 50}, b{5, 15, 25, 28, 30, 60};
        // union: 0 5 10 15 20 25 28 30 40 50 60
        for (int w : {7, 8, 9}) {
            const Result r = pair_by_lanes(a, b, w, 0);
            checks++;
            if (r.common != (w >= 8 ? 1 : 0) || r.taken != w) {
                failures++;
                std::printf("FAIL cap at the common element: width %d common %d taken %d\n", w, r.common, r.taken);
            }
        }
    }
    // widths 1 .. 200, random lengths
    for (int width = 1; width <= 200; width++)
        for (int rep = 0; rep < 20; rep++) {
            const int la = (int)(rnd() % (uint64_t)(width + 1)), lb = (int)(rnd() % (uint64_t)(width + 1));
            check_pair("random widths", random_sig(la, 0, 2 * width + 2), random_sig(lb, 0, 2 * width + 2), width);
        }
    std::printf("%ld checks, %ld failures\n", checks, failures);
    return failures ? 1 : 0;
}
