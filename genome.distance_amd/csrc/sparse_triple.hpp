// sparse_triple.hpp — the sparse tile kernel's counter addresses and its
// triple records (sparse.hip). Host and device code over plain integers:
// tests/sparse_triple_check.cpp runs the packing and the code derivation
// under the sanitizers without a device; the record build and the 3 x 3 walk
// call these same functions.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GDIST_ST_HD __host__ __device__ __forceinline__
#else
#define GDIST_ST_HD inline
#endif

namespace gdist {

// LDS counter of local pair (row a, column b), as a 16-bit slot t (dword
// t >> 1, half t & 1): row a owns dwords [64 a, 64 a + 64); column b sits in
// dword (b >> 1) ^ (a & 63) of it, half b & 1. The XOR rotation by the row
// spreads the products of one word (its rows x its columns) over the banks.
// The records carry the two halves of the address precomputed (entry_codes):
// a row entry's byte base with its rotation key, a column entry's byte offset
// and half shift, so a product's counter costs one XOR and one shift.
GDIST_ST_HD int cnt_index(int a, int b) { return ((a * 64 + ((b >> 1) ^ (a & 63))) << 1) | (b & 1); }
GDIST_ST_HD void cnt_pair(int t, int& a, int& b) {
    const int d = t >> 1;
    a = d >> 6;
    b = (((d & 63) ^ (a & 63)) << 1) | (t & 1);
}
// record codes of set s (0..127): row role = byte address of its row with the
// rotation key in bits 2-7 (row bytes 256 s, keys < 256); column role = shift
// (s & 1) << 4 in bits 0-4 and its dword's byte offset (s >> 1) << 2 in bits 16+
GDIST_ST_HD uint32_t row_code(int s) { return ((uint32_t)s << 8) | ((uint32_t)(s & 63) << 2); }
GDIST_ST_HD uint32_t col_code(int s) { return ((uint32_t)(s & 1) << 4) | (((uint32_t)(s >> 1) << 2) << 16); }

// A triple record: three entries of one (block, word) list in 32 bytes,
// 32-byte aligned, as eight dwords
//   {w0 lo, w0 hi, w1 lo, w1 hi | w2 lo, w2 hi, d6, d7}
// (each half one 16-byte load) with the codes of the three sets in d6 / d7:
//   d6 = row_code(s0) | row_code(s1) << 16
//   d7 = row_code(s2) | (s0 >> 1) << 18 | (s1 >> 1) << 26
// A row code is 15 bits with bits 0, 1 clear. The column role's byte offset
// (s >> 1) << 2 of entries 0 and 1 is a byte of d7; entry 2's, and every
// entry's half shift (s & 1) << 4, come out of the row code (s sits at its
// bit 8). A missing second or third entry is word 0 and set 0: its products
// are popcounts of 0, which add nothing, so the walk needs no count, flag
// or mask.
struct Triple {
    uint32_t d[8];
};
GDIST_ST_HD Triple triple_pack(const unsigned long long* w, const uint8_t* set, int n) {
    Triple t;
    int s[3];
    for (int k = 0; k < 3; k++) {
        const unsigned long long x = k < n ? w[k] : 0ull;
        s[k] = k < n ? (int)set[k] : 0;
        t.d[2 * k] = (uint32_t)x;
        t.d[2 * k + 1] = (uint32_t)(x >> 32);
    }
    t.d[6] = row_code(s[0]) | (row_code(s[1]) << 16);
    t.d[7] = row_code(s[2]) | ((uint32_t)(s[0] >> 1) << 18) | ((uint32_t)(s[1] >> 1) << 26);
    return t;
}
// entry k's row code, column byte offset (col_code >> 16) and column shift
// (col_code & 31) from d6 / d7; k is a compile-time constant where it matters
GDIST_ST_HD uint32_t triple_row(uint32_t d6, uint32_t d7, int k) {
    return k == 0 ? d6 & 0xFFFFu : k == 1 ? d6 >> 16 : d7 & 0xFFFFu;
}
GDIST_ST_HD uint32_t triple_coff(uint32_t d6, uint32_t d7, int k) {
    (void)d6;
    return k == 0 ? (d7 >> 16) & 0xFFu : k == 1 ? d7 >> 24 : (d7 >> 7) & 0xFCu;
}
GDIST_ST_HD uint32_t triple_shift(uint32_t d6, uint32_t d7, int k) {
    return ((k == 0 ? d6 >> 4 : k == 1 ? d6 >> 20 : d7 >> 4)) & 16u;
}

constexpr int kTripleBytes = 32;
constexpr int kSentinelTriples = 512;    // zero triples after the last (the virtual word's slots of one walk step)

}  // namespace gdist
