// Stand-alone check of csrc/group_stats_host.hpp (the host arithmetic of
// gdist_group_stats): built by tests/test_group_host.py with the host compiler
// under AddressSanitizer + UBSan, no device and no HIP. Covers the limb add
// and carry, the digit fold of the device's carry-save slots, the 256-bit
// product and variance numerator, and the n = 0 / 1 / 2 forms.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "group_stats_host.hpp"

using namespace gdist::gstats;

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            failures++;                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                             \
    } while (0)

static gdist_group_side side(int64_t n, uint64_t s0, uint64_t s1, uint64_t q0, uint64_t q1, uint64_t q2, double mn,
                             double mx) {
    gdist_group_side s;
    std::memset(&s, 0, sizeof(s));
    s.n = n;
    s.sum[0] = s0;
    s.sum[1] = s1;
    s.sumsq[0] = q0;
    s.sumsq[1] = q1;
    s.sumsq[2] = q2;
    s.min = mn;
    s.max = mx;
    s.mean = -7.0;   // garbage: finish() must overwrite both
    s.sdev = -7.0;
    return s;
}

int main() {
    const uint64_t ALL = ~0ull, P53 = 1ull << 53;

    // add / sub with carries through every limb
    U256 a, b;
    a.w[0] = a.w[1] = a.w[2] = ALL;
    b.w[0] = 1;
    CHECK(add(a, b) == 0 && a.w[0] == 0 && a.w[1] == 0 && a.w[2] == 0 && a.w[3] == 1);
    CHECK(sub(a, b) == 0 && a.w[0] == ALL && a.w[1] == ALL && a.w[2] == ALL && a.w[3] == 0);
    a.w[3] = ALL;
    CHECK(add(a, b) == 1 && a.is_zero());
    CHECK(sub(a, b) == 1 && a.w[0] == ALL && a.w[3] == ALL);
    CHECK(cmp(a, b) == 1 && cmp(b, a) == -1 && cmp(a, a) == 0);

    // 64 x 64 -> 128
    uint64_t lo, hi;
    mul64(ALL, ALL, &lo, &hi);
    CHECK(lo == 1 && hi == ALL - 1);
    mul64(P53, P53, &lo, &hi);
    CHECK(lo == 0 && hi == (1ull << 42));

    // digit fold: 2^32 - 1 in every carry-save slot of a 6-digit number, then
    // slots holding more than 32 bits (sums of digits)
    U256 d;
    for (int i = 0; i < 6; i++) add_digit(d, 0xffffffffull, i);
    CHECK(d.w[0] == ALL && d.w[1] == ALL && d.w[2] == ALL && d.w[3] == 0);
    U256 e;
    add_digit(e, ALL, 1);            // (2^64 - 1) << 32
    CHECK(e.w[0] == 0xffffffff00000000ull && e.w[1] == 0xffffffffull);
    add_digit(e, ALL, 0);            // + 2^64 - 1: carries into limb 1
    CHECK(e.w[0] == 0xfffffffeffffffffull && e.w[1] == 0x100000000ull);
    U256 f;
    add_digit(f, ALL, 7);            // the top digit: the part past 256 bits is dropped
    CHECK(f.w[3] == 0xffffffff00000000ull);

    // 256-bit product: (2^128 - 1)^2 = 2^256 - 2^129 + 1
    U256 g;
    g.w[0] = g.w[1] = ALL;
    bool of = true;
    U256 p = mul(g, g, &of);
    CHECK(!of && p.w[0] == 1 && p.w[1] == 0 && p.w[2] == ALL - 1 && p.w[3] == ALL);
    g.w[2] = 1;
    mul(g, g, &of);
    CHECK(of);

    // long double of a 256-bit value: exact for 2^200 + 2^140
    U256 h;
    h.w[3] = 1ull << 8;
    h.w[2] = 1ull << 12;
    CHECK(to_ld(h) == std::ldexp(1.0L, 200) + std::ldexp(1.0L, 140));

    // n == 0: the placeholder form whatever the other fields held
    gdist_group_side z = side(0, 5, 6, 7, 8, 9, 0.25, 0.5);
    finish(&z);
    CHECK(z.n == 0 && z.min == 1.0 && z.max == 1.0 && z.mean == 1.0 && z.sdev == 0.0);
    CHECK(z.sum[0] == 0 && z.sum[1] == 0 && z.sumsq[0] == 0 && z.sumsq[1] == 0 && z.sumsq[2] == 0);

    // n == 1: d = 0.25 -> mean 0.25, sdev 0.0
    const uint64_t q = P53 / 4;
    mul64(q, q, &lo, &hi);
    gdist_group_side one = side(1, q, 0, lo, hi, 0, 0.25, 0.25);
    finish(&one);
    CHECK(one.mean == 0.25 && one.sdev == 0.0 && !std::signbit(one.sdev));

    // n == 2: d = 0.25 and 0.75 -> mean 0.5, variance 0.125
    const uint64_t r = 3 * (P53 / 4);
    uint64_t lo2, hi2;
    mul64(r, r, &lo2, &hi2);
    U256 Q;
    Q.w[0] = lo;
    Q.w[1] = hi;
    U256 Q2;
    Q2.w[0] = lo2;
    Q2.w[1] = hi2;
    add(Q, Q2);
    gdist_group_side two = side(2, q + r, 0, Q.w[0], Q.w[1], Q.w[2], 0.25, 0.75);
    finish(&two);
    CHECK(two.mean == 0.5 && two.sdev == std::sqrt(0.125));

    // equal values: the variance numerator is exactly 0
    gdist_group_side same = side(2, 2 * q, 0, 2 * lo, 2 * hi, 0, 0.25, 0.25);
    finish(&same);
    CHECK(same.mean == 0.25 && same.sdev == 0.0);

    // the 256-bit numerator: n = 2^33 values of which half are 0 and half are
    // 1 - 2^-53 (m = 2^53 - 1): mean = m / 2^54, variance = n m^2 / (4 (n - 1) 2^106)
    {
        const uint64_t n = 1ull << 33, m = P53 - 1;
        U256 S = mul(from_u64(n / 2), from_u64(m), nullptr);
        U256 M2 = mul(from_u64(m), from_u64(m), nullptr);
        U256 QQ = mul(M2, from_u64(n / 2), nullptr);
        CHECK(S.w[1] != 0 && QQ.w[2] != 0);
        gdist_group_side big = side((int64_t)n, S.w[0], S.w[1], QQ.w[0], QQ.w[1], QQ.w[2], 0.0, 1.0 - 0x1p-53);
        finish(&big);
        const long double lm = (long double)m;
        const long double mean = std::ldexp(lm, -54);
        const long double var = std::ldexp(lm * lm, -108) * ((long double)n / (long double)(n - 1));
        CHECK(std::fabs((long double)big.mean - mean) <= std::ldexp(1.0L, -54));
        CHECK(std::fabs((long double)big.sdev - std::sqrt(var)) <= std::ldexp(1.0L, -53));
    }

    // merge: carries out of sum[0], sumsq[0] and sumsq[1]; n == 0 on either side
    gdist_group_side acc = side(3, ALL, 0, ALL, ALL, 0, 0.125, 0.5);
    gdist_group_side part = side(2, 1, 0, 1, 0, 0, 0.0625, 0.25);
    acc.ones = 4;
    part.ones = 5;
    part.nans = 1;
    merge_side(&acc, &part);
    CHECK(acc.n == 5 && acc.ones == 9 && acc.nans == 1 && acc.min == 0.0625 && acc.max == 0.5);
    CHECK(acc.sum[0] == 0 && acc.sum[1] == 1 && acc.sumsq[0] == 0 && acc.sumsq[1] == 0 && acc.sumsq[2] == 1);
    gdist_group_side empty = side(0, 0, 0, 0, 0, 0, 1.0, 1.0);
    finish(&empty);
    gdist_group_side t1 = two, t2 = empty;
    merge_side(&t1, &empty);
    merge_side(&t2, &two);
    CHECK(std::memcmp(&t1, &two, sizeof(two)) == 0 && std::memcmp(&t2, &two, sizeof(two)) == 0);
    gdist_group_side t3 = empty;
    merge_side(&t3, &empty);
    CHECK(std::memcmp(&t3, &empty, sizeof(empty)) == 0);

    std::printf("group_stats_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
