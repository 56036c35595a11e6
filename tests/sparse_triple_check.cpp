// sparse_triple_check.cpp — the triple records of the sparse tile kernel's
// 3 x 3 walk (csrc/sparse_triple.hpp) without a device: the packing the
// record build runs per triple and the code derivation the walk runs per
// slot, on arrays of exactly the sizes they read (n words and n set bytes) so
// that a read past a short list's entries is the sanitizers' to report.
//
// For every set 0 .. 127 in each of a triple's three positions: the row code,
// the column byte offset and the column shift taken out of d6 / d7 equal
// row_code / col_code, and a product's counter address row ^ offset with its
// shift is cnt_index's 16-bit slot. For n = 1, 2, 3 entries: the words and
// sets come back out of the record, and the missing entries are word 0 and
// set 0 with codes that address the counter of pair (0, 0).
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>

#include "sparse_triple.hpp"

using namespace gdist;

static int failures = 0, checks = 0;

#define EXPECT(cond, ...)                                \
    do {                                                 \
        checks++;                                        \
        if (!(cond)) {                                   \
            if (failures < 20) {                         \
                std::printf("FAIL %s: ", #cond);         \
                std::printf(__VA_ARGS__);                \
                std::printf("\n");                       \
            }                                            \
            failures++;                                  \
        }                                                \
    } while (0)

static unsigned long long word_of(const Triple& t, int k) {
    return (unsigned long long)t.d[2 * k] | ((unsigned long long)t.d[2 * k + 1] << 32);
}

int main() {
    std::mt19937_64 rng(20261021);
    // every set in every position, the other two positions random
    for (int k = 0; k < 3; k++)
        for (int s = 0; s < 128; s++) {
            std::unique_ptr<unsigned long long[]> w(new unsigned long long[3]);
            std::unique_ptr<uint8_t[]> set(new uint8_t[3]);
            for (int j = 0; j < 3; j++) {
                w[j] = rng();
                set[j] = j == k ? (uint8_t)s : (uint8_t)(rng() & 127);
            }
            const Triple t = triple_pack(w.get(), set.get(), 3);
            for (int j = 0; j < 3; j++) {
                const int sj = set[j];
                EXPECT(word_of(t, j) == w[j], "word %d of position %d set %d", j, k, s);
                EXPECT(triple_row(t.d[6], t.d[7], j) == row_code(sj), "row code of set %d at %d", sj, j);
                EXPECT(triple_coff(t.d[6], t.d[7], j) == col_code(sj) >> 16, "column offset of set %d at %d", sj, j);
                EXPECT(triple_shift(t.d[6], t.d[7], j) == (col_code(sj) & 31u), "column shift of set %d at %d", sj, j);
            }
            // the counter of (row = the set at k, column = every set b)
            for (int b = 0; b < 128; b++) {
                uint8_t cs[1] = {(uint8_t)b};
                unsigned long long cw[1] = {rng()};
                const Triple c = triple_pack(cw, cs, 1);
                const uint32_t addr = triple_row(t.d[6], t.d[7], k) ^ triple_coff(c.d[6], c.d[7], 0);
                const uint32_t sh = triple_shift(c.d[6], c.d[7], 0);
                const int slot = cnt_index(s, b);
                EXPECT(addr == (uint32_t)(slot >> 1) * 4 && sh == (uint32_t)(slot & 1) * 16, "counter of (%d, %d)", s, b);
                int ra, rb;
                cnt_pair(slot, ra, rb);
                EXPECT(ra == s && rb == b, "cnt_pair of (%d, %d)", s, b);
            }
        }
    // short lists: exactly n words and n set bytes on the heap
    for (int n = 1; n <= 3; n++)
        for (int rep = 0; rep < 200; rep++) {
            std::unique_ptr<unsigned long long[]> w(new unsigned long long[n]);
            std::unique_ptr<uint8_t[]> set(new uint8_t[n]);
            for (int j = 0; j < n; j++) {
                w[j] = rng() | 1ull;
                set[j] = (uint8_t)(rng() & 127);
            }
            const Triple t = triple_pack(w.get(), set.get(), n);
            for (int j = 0; j < 3; j++) {
                const int sj = j < n ? set[j] : 0;
                EXPECT(word_of(t, j) == (j < n ? w[j] : 0ull), "n %d: word %d", n, j);
                EXPECT(triple_row(t.d[6], t.d[7], j) == row_code(sj), "n %d: row code %d", n, j);
                EXPECT(triple_coff(t.d[6], t.d[7], j) == col_code(sj) >> 16, "n %d: column offset %d", n, j);
                EXPECT(triple_shift(t.d[6], t.d[7], j) == (col_code(sj) & 31u), "n %d: column shift %d", n, j);
            }
        }
    static_assert(sizeof(Triple) == kTripleBytes, "a triple record is 32 bytes");
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
