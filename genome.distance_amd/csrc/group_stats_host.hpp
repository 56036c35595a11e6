// group_stats_host.hpp — the host arithmetic of gdist_group_stats: exact
// multi-limb sums and the mean / standard deviation derived from them.
//
// Host-only and free of HIP: gdist_api.hip and group.hip include it, and so
// does tests/group_stats_check.cpp, which the host compiler builds under
// AddressSanitizer + UBSan.
//
// Every summarised distance d is an integer multiple of 2^-53 in [0, 1), so
// m = d * 2^53 is an integer, S = sum m and Q = sum m * m are integers, and
//   mean     = S / (n 2^53)
//   variance = (n Q - S^2) / (n (n - 1) 2^106)     (bias-corrected)
// are quotients of integers. Numerator and denominator are formed exactly in
// 256 bits, each is rounded once to the 64-bit mantissa of long double, one
// division follows and one rounding to double: within 1 ulp of the exact
// quotient (three relative errors of 2^-64 under the final half ulp). The
// standard deviation takes the square root in long double before that last
// rounding, which keeps it within 2 ulp of the exact root.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/gdist.h"

namespace gdist {
namespace gstats {

#if !defined(__HIP_DEVICE_COMPILE__)
static_assert(LDBL_MANT_DIG >= 64, "group statistics need a 64-bit long double mantissa");
#endif

// 256-bit unsigned integer, little-endian limbs
struct U256 {
    uint64_t w[4] = {0, 0, 0, 0};
    bool is_zero() const { return (w[0] | w[1] | w[2] | w[3]) == 0; }
};

// a += b; returns the carry out of the top limb
inline unsigned add(U256& a, const U256& b) {
    unsigned c = 0;
    for (int i = 0; i < 4; i++) {
        const uint64_t s = a.w[i] + b.w[i];
        const unsigned c1 = s < a.w[i];
        const uint64_t t = s + c;
        const unsigned c2 = t < s;
        a.w[i] = t;
        c = c1 | c2;
    }
    return c;
}

// a -= b (a >= b); returns the borrow out of the top limb
inline unsigned sub(U256& a, const U256& b) {
    unsigned br = 0;
    for (int i = 0; i < 4; i++) {
        const uint64_t d = a.w[i] - b.w[i];
        const unsigned b1 = a.w[i] < b.w[i];
        const uint64_t t = d - br;
        const unsigned b2 = d < br;
        a.w[i] = t;
        br = b1 | b2;
    }
    return br;
}

inline int cmp(const U256& a, const U256& b) {
    for (int i = 3; i >= 0; i--)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}

// 64 x 64 -> 128 from 32-bit halves (no compiler extension)
inline void mul64(uint64_t a, uint64_t b, uint64_t* lo, uint64_t* hi) {
    const uint64_t a0 = a & 0xffffffffu, a1 = a >> 32, b0 = b & 0xffffffffu, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffu) + (p10 & 0xffffffffu);
    *lo = (p00 & 0xffffffffu) | (mid << 32);
    *hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// a += v << (32 * digit), digit 0..7: the carry-save digit sums of the
// device (each a uint64 holding a sum of 32-bit digits) fold in exactly
inline void add_digit(U256& a, uint64_t v, int digit) {
    U256 t;
    const int limb = digit >> 1;
    if (digit & 1) {
        t.w[limb] = v << 32;
        if (limb + 1 < 4) t.w[limb + 1] = v >> 32;
    } else {
        t.w[limb] = v;
    }
    add(a, t);
}

// the low 256 bits of a * b; *overflow is set when the product needs more
inline U256 mul(const U256& a, const U256& b, bool* overflow) {
    uint64_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        uint64_t carry = 0;
        for (int j = 0; j < 4; j++) {
            uint64_t lo, hi;
            mul64(a.w[i], b.w[j], &lo, &hi);
            const uint64_t s = r[i + j] + lo;
            hi += s < lo;
            const uint64_t t = s + carry;
            hi += t < s;
            r[i + j] = t;
            carry = hi;   // a b + r + carry <= 2^128 - 1: hi cannot wrap
        }
        r[i + 4] = carry;
    }
    U256 out;
    for (int i = 0; i < 4; i++) out.w[i] = r[i];
    if (overflow) *overflow = (r[4] | r[5] | r[6] | r[7]) != 0;
    return out;
}

inline U256 from_u64(uint64_t v) {
    U256 a;
    a.w[0] = v;
    return a;
}

// nearest-or-next long double: the leading 128 bits rounded once, the bits
// below them (under 2^-64 of the value) dropped
inline long double to_ld(const U256& a) {
    int top = 3;
    while (top > 0 && a.w[top] == 0) top--;
    if (top == 0) return (long double)a.w[0];
    const long double v = std::ldexp((long double)a.w[top], 64) + (long double)a.w[top - 1];
    return std::ldexp(v, 64 * (top - 1));
}

// mean and sdev of a side from its exact n, sum and sumsq (the n == 0 form:
// 1.0 / 0.0; n == 1: sdev 0.0, SummaryStatistics.getStandardDeviation)
inline void finish(gdist_group_side* s) {
    if (s->n <= 0) {
        s->n = 0;
        s->min = s->max = s->mean = 1.0;
        s->sdev = 0.0;
        s->sum[0] = s->sum[1] = 0;
        s->sumsq[0] = s->sumsq[1] = s->sumsq[2] = 0;
        return;
    }
    U256 S, Q;
    S.w[0] = s->sum[0];
    S.w[1] = s->sum[1];
    Q.w[0] = s->sumsq[0];
    Q.w[1] = s->sumsq[1];
    Q.w[2] = s->sumsq[2];
    const long double n = (long double)s->n;   // exact: n < 2^63
    s->mean = (double)(to_ld(S) / std::ldexp(n, 53));
    s->sdev = 0.0;
    if (s->n == 1) return;
    bool o1 = false, o2 = false;
    U256 num = mul(Q, from_u64((uint64_t)s->n), &o1);
    const U256 sq = mul(S, S, &o2);
    // n Q >= S^2 (Cauchy-Schwarz) and both fit 256 bits for n < 2^34 pairs
    // (n Q < 2^34 2^141, S^2 < 2^174); past that the quotient degrades to 0
    if (o1 || o2 || cmp(num, sq) <= 0) return;
    sub(num, sq);
    const long double den = n * (long double)(s->n - 1);   // one rounding
    s->sdev = (double)std::sqrt(std::ldexp(to_ld(num) / den, -106));
}

// acc += part, exactly: integer fields limb-wise with carries, min / max
// over the sides that hold values, then mean and sdev again
inline void merge_side(gdist_group_side* acc, const gdist_group_side* part) {
    if (part->n > 0) {
        acc->min = acc->n > 0 ? (part->min < acc->min ? part->min : acc->min) : part->min;
        acc->max = acc->n > 0 ? (part->max > acc->max ? part->max : acc->max) : part->max;
    }
    acc->n = (acc->n > 0 ? acc->n : 0) + (part->n > 0 ? part->n : 0);
    acc->ones += part->ones;
    acc->nans += part->nans;
    U256 a, b;
    a.w[0] = acc->sum[0];
    a.w[1] = acc->sum[1];
    b.w[0] = part->sum[0];
    b.w[1] = part->sum[1];
    add(a, b);
    acc->sum[0] = a.w[0];
    acc->sum[1] = a.w[1];
    U256 c, d;
    for (int i = 0; i < 3; i++) {
        c.w[i] = acc->sumsq[i];
        d.w[i] = part->sumsq[i];
    }
    add(c, d);
    for (int i = 0; i < 3; i++) acc->sumsq[i] = c.w[i];
    finish(acc);
}

}  // namespace gstats
}  // namespace gdist
