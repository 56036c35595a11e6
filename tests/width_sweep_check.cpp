// Stand-alone check of csrc/width_sweep.hpp (one walk of a sketch pair's
// merged union that yields the common count at every sketch size): built by
// tests/test_width_sweep_host.py with the host compiler under
// AddressSanitizer + UBSan, no device.
//
// sweep_by_lanes() does what a wave of width_sweep_kernel does for a pair, its
// 64 lanes in a loop: the cut of the signatures at the last size, the segment
// cut, the lanes' walks into the per-size counters, the prefix sum of the
// unions (Mash) and of the counters. Its (common, taken) at every size must
// equal a plain two-pointer merge of the two size-s prefixes, for both flag
// settings. The signatures live in exactly sized vectors, so a read past
// either end is an AddressSanitizer report.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "width_sweep.hpp"

using Sig = std::vector<int32_t>;

static long checks = 0, failures = 0;

static uint64_t rng_state = 0x13198A2E03707344ull;
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
    double d;   // sweep_by_lanes: the distance the kernel forms at this size
};

// the reference at one size: the two prefixes, one two-pointer merge over the
// first `size` union elements (Mash) or all of them (Jaccard)
static Result plain(const Sig& fa, const Sig& fb, int size, int jaccard) {
    const Sig a(fa.begin(), fa.begin() + std::min<size_t>(fa.size(), (size_t)size));
    const Sig b(fb.begin(), fb.begin() + std::min<size_t>(fb.size(), (size_t)size));
    size_t i = 0, j = 0;
    int common = 0, taken = 0;
    while ((i < a.size() || j < b.size()) && (jaccard || taken < size)) {
        if (j == b.size() || (i < a.size() && a[i] < b[j])) i++;
        else if (i == a.size() || b[j] < a[i]) j++;
        else { common++; i++; j++; }
        taken++;
    }
    return Result{common, taken, 0.0};
}

static std::vector<Result> sweep_by_lanes(const Sig& q, const Sig& s, const std::vector<int32_t>& sizes, int jaccard) {
    using namespace gdist;
    const int nsizes = (int)sizes.size(), smax = sizes.back();
    const int lq = std::min((int)q.size(), smax), ls = std::min((int)s.size(), smax);
    const bool qa = lq >= ls;
    // data() of an empty vector may be null: nothing may be read through it
    const int32_t *A = qa ? q.data() : s.data(), *B = qa ? s.data() : q.data();
    const int na = qa ? lq : ls, nb = qa ? ls : lq;
    const int ca = skx_chunk(na);
    std::vector<int32_t> counter(sizes.size(), 0);   // exactly sized: a slot past the list is a report
    int a0[kSkxLanes], a1[kSkxLanes], b0[kSkxLanes], b1[kSkxLanes], uni[kSkxLanes];
    uint64_t mask[kSkxLanes];
    int total = 0;
    for (int t = 0; t < kSkxLanes; t++) {
        skx_a_range(na, ca, t, &a0[t], &a1[t]);
        b0[t] = skx_b_begin(A, na, B, nb, ca, t);
        b1[t] = t + 1 < kSkxLanes ? skx_b_begin(A, na, B, nb, ca, t + 1) : nb;
        if (jaccard) {
            wsw_walk_jaccard(A, a0[t], a1[t], B, b0[t], b1[t], sizes.data(), nsizes, counter.data());
        } else {
            const int c = skx_merge(A, a0[t], a1[t], B, b0[t], b1[t], &mask[t]);
            uni[t] = (a1[t] - a0[t]) + (b1[t] - b0[t]) - c;
            total += uni[t];
        }
    }
    if (!jaccard) {
        int before = 0;
        for (int t = 0; t < kSkxLanes; t++) {
            wsw_walk_mash(A, a0[t], a1[t], B, b0[t], b1[t], before, uni[t], mask[t], sizes.data(), nsizes,
                          counter.data());
            before += uni[t];
        }
    }
    std::vector<Result> out;
    int common = 0;
    for (int k = 0; k < nsizes; k++) {
        common += counter[k];
        const int size = sizes[k];
        out.push_back(Result{common, jaccard ? std::min(lq, size) + std::min(ls, size) - common
                                             : skx_taken(total, size, 0),
                             wsw_distance(common, size, lq, ls, total, jaccard)});
    }
    return out;
}

static void check_pair(const char* what, const Sig& a, const Sig& b, const std::vector<int32_t>& sizes) {
    for (int jaccard = 0; jaccard < 2; jaccard++) {
        for (int swap = 0; swap < 2; swap++) {
            const Sig& x = swap ? b : a;
            const Sig& y = swap ? a : b;
            const std::vector<Result> got = sweep_by_lanes(x, y, sizes, jaccard);
            for (size_t k = 0; k < sizes.size(); k++) {
                const Result want = plain(x, y, sizes[k], jaccard);
                checks++;
                if (want.common != got[k].common || want.taken != got[k].taken) {
                    failures++;
                    if (failures < 50)
                        std::printf("FAIL %s: |a| %zu |b| %zu size %d (%zu of %zu) jaccard %d: common %d taken %d, "
                                    "expected %d %d\n", what, x.size(), y.size(), sizes[k], k, sizes.size(), jaccard,
                                    got[k].common, got[k].taken, want.common, want.taken);
                }
                // the distance is the one-size distance of the two prefixes
                const int px = std::min((int)x.size(), sizes[k]), py = std::min((int)y.size(), sizes[k]);
                const double e = gdist::skx_distance(want.common, want.taken, px, py, jaccard, 0);
                checks++;
                if (got[k].d != e) {
                    failures++;
                    if (failures < 50) std::printf("FAIL %s: distance at size %d jaccard %d\n", what, sizes[k], jaccard);
                }
            }
        }
    }
}

// `count` strictly increasing sizes within [1, width]: 1 and width among them when count >= 2
static std::vector<int32_t> size_list(int count, int width) {
    std::set<int32_t> s;
    count = std::min(count, width);
    if (count >= 1) s.insert(width);
    if (count >= 2) s.insert(1);
    while ((int)s.size() < count) s.insert(1 + (int32_t)(rnd() % (uint64_t)width));
    return std::vector<int32_t>(s.begin(), s.end());
}

static void check_lists(const char* what, const Sig& a, const Sig& b, int width) {
    for (int count : {1, 2, 7, 64, 65, 130}) check_pair(what, a, b, size_list(count, width));
}

int main() {
    const int widths[] = {1, 2, 3, 63, 64, 65, 127, 128, 130, 1000};
    for (int width : widths) {
        const int lens_raw[] = {0, 1, 2, 5, width / 2, width};
        std::set<int> lens;
        for (int l : lens_raw) lens.insert(l < width ? l : width);
        // random pairs: dense values (many common elements), then any int32
        for (int la : lens)
            for (int lb : lens) {
                check_lists("random dense", random_sig(la, -width, 3 * (int64_t)width + 2),
                            random_sig(lb, -width, 3 * (int64_t)width + 2), width);
                check_lists("random int32", random_sig(la, 0, 0), random_sig(lb, 0, 0), width);
            }
        const Sig full = random_sig(width, 0, 0);
        check_lists("identical", full, full, width);
        // disjoint: all of one below all of the other (check_pair runs both orders)
        Sig low = random_sig(width, -5000000, 4000000), high = random_sig(width, 1000, 4000000);
        check_lists("disjoint", low, high, width);
        check_lists("disjoint short", Sig(low.begin(), low.begin() + (width + 1) / 2), high, width);
        // interleaved: evens against odds, and evens against multiples of three
        Sig ev, od, th;
        for (int i = 0; i < width; i++) { ev.push_back(2 * i); od.push_back(2 * i + 1); th.push_back(3 * i); }
        check_lists("interleaved", ev, od, width);
        check_lists("interleaved common", ev, th, width);
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
        check_lists("extremes both", ext, ext, width);
        check_lists("extremes", ext, ext2, width);
        check_lists("extremes vs random", ext, full, width);
        check_lists("INT_MAX alone", Sig{INT_MAX}, ext, width);
        check_lists("INT_MIN alone", Sig{INT_MIN}, ext, width);
        check_lists("INT_MIN vs INT_MAX", Sig{INT_MIN}, Sig{INT_MAX}, width);
    }
    // na < 64 < nb, and the shorter side on either side of a lane's chunk
    for (int la : {1, 2, 5, 33, 63})
        for (int lb : {65, 100, 130, 1000}) {
            check_lists("short vs long", random_sig(la, 0, 3000), random_sig(lb, 0, 3000), 1000);
            check_lists("short vs long", random_sig(la, 0, 0), random_sig(lb, 0, 0), lb);
        }
    // every size 1 .. 130 (more than 64 and more than 128 sizes), and sizes above both lengths
    {
        std::vector<int32_t> all;
        for (int s = 1; s <= 130; s++) all.push_back(s);
        check_pair("every size", random_sig(130, 0, 400), random_sig(130, 0, 400), all);
        check_pair("every size 130/40", random_sig(130, 0, 400), random_sig(40, 0, 400), all);
        check_pair("sizes above both lengths", random_sig(20, 0, 60), random_sig(9, 0, 60), all);
        check_pair("sizes above both lengths", random_sig(20, 0, 60), random_sig(9, 0, 60), {50, 51, 1000});
        check_pair("both empty", Sig{}, Sig{}, all);
        check_pair("one empty", Sig{}, random_sig(77, 0, 0), all);
        Sig a = random_sig(130, 0, 300);
        check_pair("every size identical", a, a, all);
    }
    // signatures wider than the last size: the collection was built at a larger width
    for (int rep = 0; rep < 20; rep++) {
        const Sig a = random_sig(600 + (int)(rnd() % 400), 0, 2500), b = random_sig((int)(rnd() % 1000), 0, 2500);
        check_pair("wider than the sizes", a, b, size_list(40, 300));
        check_pair("wider than the sizes", a, b, {1});
    }
    // long signatures: a lane's segment holds more than 64 union elements and is walked again
    {
        const Sig a = random_sig(20000, 0, 60000), b = random_sig(17000, 0, 60000), c = random_sig(70, 0, 60000);
        check_pair("long", a, b, {1, 64, 4097, 20000});
        check_pair("long", a, b, size_list(130, 20000));
        check_pair("long vs short", a, c, {1, 64, 4097, 20000});
        check_pair("long identical", a, a, {1, 64, 4097, 20000});
    }
    // a named case: common element 30 is union element 8 (1-based), index 3 in a and 4 in b
    {
        const Sig a{0, 10, 20, 30, 40, 50}, b{5, 15, 25, 28, 30, 60};
        const std::vector<int32_t> sizes{4, 5, 7, 8};
        const std::vector<Result> m = sweep_by_lanes(a, b, sizes, 0), j = sweep_by_lanes(a, b, sizes, 1);
        const int want_m[] = {0, 0, 0, 1}, want_j[] = {0, 1, 1, 1};
        for (int k = 0; k < 4; k++) {
            checks++;
            if (m[k].common != want_m[k] || j[k].common != want_j[k]) {
                failures++;
                std::printf("FAIL threshold of the common element: size %d mash %d jaccard %d\n", sizes[k], m[k].common,
                            j[k].common);
            }
        }
    }
    // widths 1 .. 300, random lengths, random size lists
    for (int width = 1; width <= 300; width++)
        for (int rep = 0; rep < 6; rep++) {
            const int la = (int)(rnd() % (uint64_t)(width + 1)), lb = (int)(rnd() % (uint64_t)(width + 1));
            check_pair("random widths", random_sig(la, 0, 2 * width + 2), random_sig(lb, 0, 2 * width + 2),
                       size_list(1 + (int)(rnd() % 20), width));
        }
    std::printf("%ld checks, %ld failures\n", checks, failures);
    return failures ? 1 : 0;
}
