// bitset.hip — the dense tier of a step: tiles of |A∩B| over the dictionary-
// rank bitsets.
//
// Replaces the SequenceKmers.distance(other) loop over many pairs
// (FastaDistanceProcessor.java:177-186, GenomeProcessor.java:140,
// WidthProcessor.java:159-165): |A∩B| = Σ_w popcount(a_w & b_w) over
// per-set bitsets indexed by the rank of each kmer in a global dictionary
// (built by bitset_build.hip / bitset_fill.hip; kmers held by few sets are
// left to the other tiers: rare.hip, sparse.hip, variant.hip, whose counts
// are added to the same I).
//
// Two tile kernels. bitset_mfma_kernel (the default from kMfmaMinWords dense
// words): the count as a bit-matrix product on the matrix cores, FP4 operands
// where a bit is the nibble 0.0 / 1.0, a 256 x 256 tile per 512-thread
// workgroup, the bitsets themselves staged global -> LDS by DMA and expanded
// to nibbles in registers (or read from the operand fp4_expand_kernel expands
// once: option bitset_mfma_raw 0), exact in f32 below kMfmaMaxSplitWords words
// a K split. bitset_tile_kernel2 (few dense words, or option bitset_mfma 0):
// AND + popcount on the VALU, a 128 x 128 tile per 256-thread workgroup, 8 x 8
// accumulators a thread, with trimmed instantiations for diagonal tiles and a
// partial last row tile. K splits of either are summed with exact int32
// atomics. dense_tiles_launch picks the kernel and the K split for a region's
// plan; where the launch stands among the step's other families is
// bitset_matrix's (matrix_step.hip). bitset_row is the one-row query.
#include <algorithm>

#include "gdist_internal.hpp"
#include "bitset_tiles.hpp"

namespace gdist {
namespace {

constexpr int NT = 256;

// v_bcnt_u32_b32 d, x, acc = popcount(x) + acc. Written as asm because hipcc
// otherwise reassociates the sums into extra v_add3_u32 (10 VALU ops per
// 4 dwords instead of 8).
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

// ---- dense tiles: LDS-DMA double buffering, split-major XCD-aware order ----
// 256 threads own a 128×128 tile, 8×8 counts per thread;
//  * chunks of KC2 = 8 words are moved HBM/L2 -> LDS by global_load_lds_dwordx4
//    (no register staging, so ≤ 128 VGPRs and 4 waves per SIMD), double
//    buffered: chunk k+1 is in flight while chunk k is computed;
//  * the LDS image swizzle (slot q of row g at q ^ ((g >> 2) & 3)) is applied on
//    the DMA source address (the destination of one DMA instruction is linear);
//  * blocks are ordered split-major and remapped so one XCD runs consecutive
//    units: concurrently resident blocks work on the same K-range of every set,
//    which stays in the L2 / Infinity Cache while all tiles consume it.
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

constexpr int KC2 = 8;                        // words per chunk
constexpr int ROW2 = KC2 * 8;                 // 64 B per set row
constexpr int OPB2 = BT * ROW2;               // 8 KiB per operand per stage
constexpr int STAGE2 = 2 * OPB2;              // A + B

__device__ __forceinline__ int lds_off2(int g, int q) { return g * ROW2 + ((q ^ ((g >> 2) & 3)) << 4); }

// one operand's chunk: 8 DMA instructions of 1 KiB (16 rows), 2 per wave
__device__ __forceinline__ void dma_chunk(const unsigned long long* __restrict__ bits, int64_t W, int64_t set0,
                                          int64_t lo, int64_t lim, int64_t kc, unsigned char* lds_op, int wave,
                                          int lane) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int rbase = (wave * 2 + i) * 16;
        const int g = rbase + (lane >> 2);
        const int p = lane & 3;
        const int q = p ^ ((g >> 2) & 3);
        int64_t set = set0 + g;
        set = set < lim ? set : lim - 1;              // clamp: rows outside [lo, lim) are masked at the end
        set = set >= lo ? set : lo;
        const unsigned long long* src = bits + set * W + kc * KC2 + q * 2;
        __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)(lds_op + rbase * ROW2), 16, 0, 0);
    }
}

// One staged chunk (KC2 words of 128 row sets and 128 column sets) into the
// thread's 8x8 accumulators, two column fragments at once, dword-outer, so
// consecutive v_and/v_bcnt pairs belong to 16 different accumulators and no
// instruction waits on its predecessor. DIAG: the tile sits on the diagonal of an
// upper-triangle region, where accumulator (r, c) holds pairs with j > i only
// when c >= r (rows ty + 16r, columns tx + 16c): the c < r ones (28 of 64) are
// never computed. RR: only accumulator rows r < RR hold rows of the block (a
// partial row tile at a block's end); the others are never computed.
template <bool DIAG, int RR = 8>
__device__ __forceinline__ void chunk_pairs(const unsigned char* A, const unsigned char* B, int ty, int tx,
                                            uint32_t (&acc)[8][8]) {
#pragma unroll 1
    for (int q = 0; q < KC2 / 2; q++) {
        uint4 a[8];
#pragma unroll
        for (int r = 0; r < RR; r++) a[r] = *reinterpret_cast<const uint4*>(A + lds_off2(ty + 16 * r, q));
#pragma unroll
        for (int c = 0; c < 8; c += 2) {
            const uint4 b0 = *reinterpret_cast<const uint4*>(B + lds_off2(tx + 16 * c, q));
            const uint4 b1 = *reinterpret_cast<const uint4*>(B + lds_off2(tx + 16 * (c + 1), q));
            const uint32_t bw0[4] = {b0.x, b0.y, b0.z, b0.w};
            const uint32_t bw1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int d = 0; d < 4; d++) {
#pragma unroll
                for (int r = 0; r < RR; r++) {
                    const uint32_t ad = d == 0 ? a[r].x : d == 1 ? a[r].y : d == 2 ? a[r].z : a[r].w;
                    if (!DIAG || c >= r) acc[r][c] = bcnt_acc(ad & bw0[d], acc[r][c]);
                    if (!DIAG || c + 1 >= r) acc[r][c + 1] = bcnt_acc(ad & bw1[d], acc[r][c + 1]);
                }
            }
        }
    }
}

// DIAG: every tile of the launch sits on the diagonal of an upper-triangle
// region (bitset_matrix launches those tiles separately). RR < 8: every tile
// of the launch is the partial last row tile of the block, with at most 16 RR
// rows (rows ty + 16r with r >= RR are past r1 for every thread).
template <bool DIAG, int RR = 8>
__global__ __launch_bounds__(NT, 4) void bitset_tile_kernel2(
    const unsigned long long* __restrict__ bits, int64_t W, const int2* __restrict__ tiles, int ntiles, int splits,
    int64_t nchunks, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int64_t corg, int upper,
    int32_t* __restrict__ I, int64_t ldI) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE2];

    // XCD-aware bijective remap, then split-major unit order
    const int64_t G = gridDim.x, blk = blockIdx.x;
    const int64_t xcd = blk & 7, kq = blk >> 3, qg = G >> 3, rem = G & 7;
    const int64_t u = xcd * qg + (xcd < rem ? xcd : rem) + kq;
    const int split = (int)(u / ntiles);
    const int tile = (int)(u - (int64_t)split * ntiles);
    const int2 t = tiles[tile];
    if (split >= splits || t.x < 0 || t.y < 0) return;
    const int64_t row0 = r0 + (int64_t)t.x * BT;
    const int64_t col0 = corg + (int64_t)t.y * BT;     // column tiles start at corg <= c0 (see bitset_matrix)
    const int64_t kc_per = ceil_div(nchunks, splits);
    const int64_t kc0 = (int64_t)split * kc_per;
    const int64_t kc1 = kc0 + kc_per < nchunks ? kc0 + kc_per : nchunks;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = tid & 15, ty = tid >> 4;

    uint32_t acc[8][8];
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
        for (int c = 0; c < 8; c++) acc[r][c] = 0;

    if (kc0 < kc1) {
        dma_chunk(bits, W, row0, r0, r1, kc0, lds, wave, lane);
        dma_chunk(bits, W, col0, c0, c1, kc0, lds + OPB2, wave, lane);
    }
    for (int64_t kc = kc0; kc < kc1; kc++) {
        const int st = (int)((kc - kc0) & 1);
        unsigned char* A = lds + st * STAGE2;
        unsigned char* B = A + OPB2;
        if (kc + 1 < kc1) {
            unsigned char* An = lds + (st ^ 1) * STAGE2;
            dma_chunk(bits, W, row0, r0, r1, kc + 1, An, wave, lane);
            dma_chunk(bits, W, col0, c0, c1, kc + 1, An + OPB2, wave, lane);
            asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");   // chunk kc landed everywhere
        } else {
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        }
        chunk_pairs<DIAG, RR>(A, B, ty, tx, acc);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // stage free for the next DMA
    }

#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int64_t i = row0 + ty + 16 * r;
        if (i >= r1) continue;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int64_t j = col0 + tx + 16 * c;
            if (j < c0 || j >= c1 || (upper && j <= i)) continue;
            if (acc[r][c]) atomicAdd(I + (i - r0) * ldI + (j - c0), (int32_t)acc[r][c]);
        }
    }
}

// ---- dense tiles on the matrix cores (round 4) ------------------------------
// |A ∩ B| over the dense words is a bit-matrix product: I = Σ_k a_ik b_jk over
// the dictionary bits. The block-scaled MFMA v_mfma_scale_f32_32x32x64_f8f6f4
// takes FP4 (e2m1) operands, where the codes 0x0 and 0x2 are 0.0 and 1.0:
// with every bit stored as one nibble, one instruction is a 32 x 32 block of
// pairs over 64 bits (one word), products and f32 sums exact (a count <=
// 64 W < 2^24). The FP4 rate is 4x the BF16 MFMA rate, 5 P products/s
// dense; the AND + popcount tiles are capped at 0.63 P bit-pairs/s by the
// half-rate v_bcnt. Operand map (scripts/microbench/fp4_probe.hip, checked
// against the CPU): lane r + 32 h holds row r's bits [32 h, 32 h + 32) of the
// word as 16 bytes of nibbles, low nibble first; D: column lane & 31, row
// (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
// F = the dense bits expanded once per collection, [N][32 W] bytes (4x the
// bitsets). A workgroup of 8 waves owns a 256 x 256 tile of pairs and a range
// of words, each wave 64 rows x 128 columns (2 x 4 MFMA blocks, 128 f32
// accumulators a lane); stages of KM words of both operands (256 rows x
// 32 KM bytes each) are moved by global_load_lds, double buffered, with the
// 16-byte chunk c of row g stored at c ^ ((g >> 1) & 7) (conflict-free
// fragment reads); units split-major and XCD-remapped as the VALU tiles.
constexpr int MNT = 512;                      // threads
// f32 is exact for integers <= 2^24: one K split's count of shared bits is
// <= 64 x its words, so a split spans at most 2^18 words
constexpr int64_t kMfmaMaxSplitWords = int64_t(1) << 18;
// the fewest K splits (of nst stages of km words) that keep every split's
// count exact in f32
static inline int64_t mfma_min_splits(int64_t nst, int km) {
    const int64_t per_max = kMfmaMaxSplitWords / km;                 // stages a split may span
    return nst <= per_max ? 1 : (nst + per_max - 1) / per_max;
}
// KM words per stage (4: 2 x 32 KiB a stage, 128 KiB double-buffered; 2:
// 64 KiB, so a row-major rare workgroup fits beside it on a CU: option
// bitset_mfma_km)
template <int KM> constexpr int mrow() { return KM * 32; }          // bytes per row per stage
template <int KM> constexpr int mopb() { return MT * mrow<KM>(); }  // one operand's stage
typedef int v8i_t __attribute__((ext_vector_type(8)));
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef float v16f_t __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint32_t bits_to_nibbles(uint32_t byte) {   // 8 bits -> 8 nibbles 0x0 / 0x2
    uint32_t t = (byte & 0x0Fu) | ((byte & 0xF0u) << 12);
    t = (t | (t << 6)) & 0x03030303u;
    t = (t | (t << 3)) & 0x11111111u;
    return t << 1;
}

// F[i][32 w + q] for one (set, word) per thread: 32 bytes of nibbles
__global__ void fp4_expand_kernel(const unsigned long long* __restrict__ bits, int64_t n, uint4* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const unsigned long long w = bits[t];
        const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
        out[2 * t] = make_uint4(bits_to_nibbles(lo & 0xFF), bits_to_nibbles((lo >> 8) & 0xFF),
                                bits_to_nibbles((lo >> 16) & 0xFF), bits_to_nibbles(lo >> 24));
        out[2 * t + 1] = make_uint4(bits_to_nibbles(hi & 0xFF), bits_to_nibbles((hi >> 8) & 0xFF),
                                    bits_to_nibbles((hi >> 16) & 0xFF), bits_to_nibbles(hi >> 24));
    }
}

// chunk c (16 B) of row g: KM = 4 rows of 8 chunks, c ^ ((g >> 1) & 7); KM =
// 2 rows of 4 chunks, c ^ ((g >> 2) & 3) (conflict-free ds_read_b128 either way)
template <int KM> __device__ __forceinline__ int mslot(int g, int c) {
    return KM == 4 ? (c ^ ((g >> 1) & 7)) : (c ^ ((g >> 2) & 3));
}
template <int KM> __device__ __forceinline__ int mlds(int g, int c) { return g * mrow<KM>() + (mslot<KM>(g, c) << 4); }

// one operand's stage: 16-byte chunks, KM per thread (lane-linear LDS, the
// swizzle applied on the source address)
template <int KM, int NT = MNT>
__device__ __forceinline__ void mfma_stage(const unsigned char* __restrict__ F, int64_t rowbytes, int64_t set0,
                                           int64_t lo, int64_t lim, int64_t w0, unsigned char* lds_op, int tid) {
    constexpr int CPR = 2 * KM;                       // chunks per row
#pragma unroll
    for (int i = 0; i < KM * (MNT / NT); i++) {
        const int q = i * NT + tid;                   // 16-byte slot of the stage
        const int g = q / CPR, sl = q % CPR;
        const int c = mslot<KM>(g, sl);               // the chunk this slot holds (the swizzle is an involution)
        int64_t set = set0 + g;
        set = set < lim ? set : lim - 1;              // rows outside [lo, lim): clamped, masked at the end
        set = set >= lo ? set : lo;
        const unsigned char* src = F + set * rowbytes + w0 * 32 + c * 16;
        __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)(lds_op + (i * NT + (tid & ~63)) * 16), 16,
                                         0, 0);
    }
}

// piece i (0 .. KM - 1) of one operand's stage: the i-th iteration of
// mfma_stage, so that a stage's DMA can be spread between MFMAs
template <int KM>
__device__ __forceinline__ void mfma_piece(const unsigned char* __restrict__ F, int64_t rowbytes, int64_t set0,
                                           int64_t lo, int64_t lim, int64_t w0, unsigned char* lds_op, int tid,
                                           int i) {
    constexpr int CPR = 2 * KM;
    const int q = i * MNT + tid;
    const int g = q / CPR, sl = q % CPR;
    const int c = mslot<KM>(g, sl);
    int64_t set = set0 + g;
    set = set < lim ? set : lim - 1;
    set = set >= lo ? set : lo;
    const unsigned char* src = F + set * rowbytes + w0 * 32 + c * 16;
    __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)(lds_op + (i * MNT + (tid & ~63)) * 16), 16, 0,
                                     0);
}

// the wait at the top of a stage: every stage still in flight after it may stay
// (g = glds per stage per thread: 2 KM); a counted vmcnt keeps the later stages'
// DMAs going across the barrier (raw s_barrier, never __syncthreads, whose
// fence would drain them)
template <int G>
__device__ __forceinline__ void mfma_wait(int later) {
    switch (later) {
        case 0: asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(G) : "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(2 * G) : "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(3 * G) : "memory"); break;
    }
}

// Round 5 (RAW): the operand is the bitsets themselves, not the nibbles. A
// stage of the same 128 bytes per row holds 16 words instead of 4, so a tile
// moves a quarter of the bytes global -> LDS (C4: 80 -> 20 GB a 1,024-row
// step; the nibble operand was 4x the bitsets in HBM and in every L2), and
// each lane expands its fragment in registers: MFMA step m of a stage takes
// lane (r, h)'s dword 4 q + m of its half h of row r (chunk 4 h + q), and
// nibble j of fragment dword k holds bit 4 j + k of that dword as 0x0 / 0x2
// (x << 1, x, x >> 1, x >> 2 under 0x22222222: 7 VALU per dword). Any
// assignment of bits to K positions is exact as long as both operands use
// the same one.
__device__ __forceinline__ v4i_t raw_nibbles(uint32_t x) {
    const v4i_t f = {(int)((x << 1) & 0x22222222u), (int)(x & 0x22222222u), (int)((x >> 1) & 0x22222222u),
                     (int)((x >> 2) & 0x22222222u)};
    return f;
}

// NS stages in a ring (2: double buffering; 4 with KM = 2 in the same 128
// KiB: three stages in flight while one is computed; option bitset_mfma_km)
// STORE (round 5, option bitset_mfma_store): one K split, every pair of the
// tile STORED (the tile is its only writer; the other families add after it
// in stream order) instead of 64 K device atomics a tile
// SPREAD (round 6, raw KM = 4 double-buffered only; option bitset_mfma_sched,
// default 1): the next stage's DMA spread between the current stage's MFMAs
// (one piece after each MFMA step of its first two fragment reads) with ONE
// barrier a stage — the barrier at the top of stage ks says both that stage
// ks landed and that every wave is done with stage ks - 1's buffer, which the
// pieces of stage ks + 1 then overwrite. Before, every wave issued its 8
// pieces at the top of the stage, where the CU's 64 KiB of requests held
// the MFMA pipe (tiles alone: C4 slice 7.45 vs 7.98 ms, C3 0.72 vs 0.79;
// profiles/r06/s12)
// PLANE (round 6, with SPREAD; option bitset_mfma_plane): MFMA step m takes
// bit m of every nibble of the chunk's four dwords (x & 0x11111111 << m;
// plane 3, the sign bit, shifted into bit 2) instead of the four bits of
// dword m moved to bit 1: 5 VALU a dword instead of 7. The planes' nibbles
// are the e2m1 codes 0x1 / 0x2 / 0x4 = 0.5 / 1.0 / 2.0, each step under the
// e8m0 scale (both operands) that makes them 1.0 (128 / 127 / 126), so every
// product is still 0 or 1 (scripts/microbench/fp4_scale_probe.hip)
__device__ __forceinline__ int bit_plane(uint32_t x, int m) {
    return (int)(m < 3 ? (x & (0x11111111u << m)) : ((x >> 1) & 0x44444444u));
}
template <int KM, int NS, bool RAW = false, bool STORE = false, bool SPREAD = false, bool PLANE = false>
__global__ __launch_bounds__(MNT, 2) void bitset_mfma_kernel(
    const unsigned char* __restrict__ F, int64_t W, const int2* __restrict__ tiles, int ntiles, int splits,
    int64_t nstages, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int upper, int32_t* __restrict__ I,
    int64_t ldI) {
    static_assert(NS >= 2 && NS <= 4, "stage ring of 2..4");
    extern __shared__ __attribute__((aligned(16))) unsigned char mlds_buf[];     // NS stages x (A, B)
    constexpr int MOPB = mopb<KM>();
    const int64_t G = gridDim.x, blk = blockIdx.x;
    const int64_t xcd = blk & 7, kq = blk >> 3, qg = G >> 3, rem = G & 7;
    const int64_t u = xcd * qg + (xcd < rem ? xcd : rem) + kq;
    const int split = (int)(u / ntiles);
    const int tile = (int)(u - (int64_t)split * ntiles);
    if (split >= splits) return;
    const int2 t = tiles[tile];
    const int64_t row0 = r0 + (int64_t)t.x * MT, col0 = c0 + (int64_t)t.y * MT;
    const int64_t per = ceil_div(nstages, splits);
    const int64_t ks0 = (int64_t)split * per, ks1 = ks0 + per < nstages ? ks0 + per : nstages;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;          // 4 x 2 waves of 64 rows x 128 columns
    const int r = lane & 31, h = lane >> 5;
    const int64_t rowbytes = RAW ? W * 8 : W * 32;
    v16f_t acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[a][b][q] = 0.0f;
    if constexpr (SPREAD) {
        static_assert(RAW && KM == 4 && NS == 2 && !STORE, "the spread DMA: raw 16-word stages, double buffered");
        // piece pc of stage ks: operand A's slots 0 .. KM - 1, then B's
        // (into the buffer of stage ks, the bytes of stage kd: the last stage
        // re-reads its own bytes into the free buffer, so that the pieces
        // need no branch between the MFMAs)
        auto piece = [&](int64_t ks, int64_t kd, int pc) {
            unsigned char* An = mlds_buf + (int)((ks - ks0) & 1) * (2 * MOPB);
            if (pc < KM) mfma_piece<KM>(F, rowbytes, row0, r0, r1, kd * KM, An, tid, pc);
            else mfma_piece<KM>(F, rowbytes, col0, c0, c1, kd * KM, An + MOPB, tid, pc - KM);
        };
        if (ks0 < ks1)
            for (int pc = 0; pc < 2 * KM; pc++) piece(ks0, ks0, pc);
        for (int64_t ks = ks0; ks < ks1; ks++) {
            // stage ks landed everywhere, and stage ks - 1's buffer is free
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            const int64_t kd = ks + 1 < ks1 ? ks + 1 : ks;
            const unsigned char* A = mlds_buf + (int)((ks - ks0) & 1) * (2 * MOPB);
            const unsigned char* B = A + MOPB;
#pragma unroll
            for (int q = 0; q < KM; q++) {
                v4i_t af[2], bf[4];
#pragma unroll
                for (int a = 0; a < 2; a++)
                    af[a] = *reinterpret_cast<const v4i_t*>(A + mlds<KM>(wr * 64 + a * 32 + r, KM * h + q));
#pragma unroll
                for (int b = 0; b < 4; b++)
                    bf[b] = *reinterpret_cast<const v4i_t*>(B + mlds<KM>(wc * 128 + b * 32 + r, KM * h + q));
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    v4i_t an[2], bn[4];
                    if constexpr (PLANE) {
#pragma unroll
                        for (int a = 0; a < 2; a++)
                            an[a] = v4i_t{bit_plane((uint32_t)af[a][0], m), bit_plane((uint32_t)af[a][1], m),
                                          bit_plane((uint32_t)af[a][2], m), bit_plane((uint32_t)af[a][3], m)};
#pragma unroll
                        for (int b = 0; b < 4; b++)
                            bn[b] = v4i_t{bit_plane((uint32_t)bf[b][0], m), bit_plane((uint32_t)bf[b][1], m),
                                          bit_plane((uint32_t)bf[b][2], m), bit_plane((uint32_t)bf[b][3], m)};
                    } else {
#pragma unroll
                        for (int a = 0; a < 2; a++) an[a] = raw_nibbles((uint32_t)af[a][m]);
#pragma unroll
                        for (int b = 0; b < 4; b++) bn[b] = raw_nibbles((uint32_t)bf[b][m]);
                    }
                    // plane m's nibbles are 0.5 / 1.0 / 2.0 / 2.0: scales 2, 1, 1/2, 1/2 a side
                    constexpr int kPlaneScale[4] = {128, 127, 126, 126};
                    const int sc = PLANE ? kPlaneScale[m] : 0;
#pragma unroll
                    for (int a = 0; a < 2; a++)
#pragma unroll
                        for (int b = 0; b < 4; b++) {
                            const v8i_t av = {an[a][0], an[a][1], an[a][2], an[a][3], 0, 0, 0, 0};
                            const v8i_t bv = {bn[b][0], bn[b][1], bn[b][2], bn[b][3], 0, 0, 0, 0};
                            acc[a][b] =
                                __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[a][b], 4, 4, 0, sc, 0, sc);
                        }
                    if (q * 4 + m < 2 * KM) piece(ks + 1, kd, q * 4 + m);
                }
            }
        }
    } else {
    auto issue = [&](int64_t ks) {
        unsigned char* An = mlds_buf + (int)((ks - ks0) % NS) * (2 * MOPB);
        mfma_stage<KM>(F, rowbytes, row0, r0, r1, ks * KM, An, tid);
        mfma_stage<KM>(F, rowbytes, col0, c0, c1, ks * KM, An + MOPB, tid);
    };
    for (int64_t k = ks0; k < ks1 && k < ks0 + NS - 1; k++) issue(k);
    for (int64_t ks = ks0; ks < ks1; ks++) {
        const unsigned char* A = mlds_buf + (int)((ks - ks0) % NS) * (2 * MOPB);
        const unsigned char* B = A + MOPB;
        if (ks + NS - 1 < ks1) issue(ks + NS - 1);
        // stages issued after ks: min(NS - 1, ks1 - 1 - ks)
        const int64_t later = ks1 - 1 - ks < NS - 1 ? ks1 - 1 - ks : NS - 1;
        mfma_wait<2 * KM>((int)later);               // stage ks landed everywhere
        if constexpr (RAW) {
            // KM = 4: 128-byte rows (16 words a stage); KM = 2: 64-byte rows
            // (8 words), a 64 KiB double-buffered ring (option bitset_mfma_km 2)
            // lane half h takes chunks KM h .. KM h + KM - 1 of its row
#pragma unroll
            for (int q = 0; q < KM; q++) {
                v4i_t af[2], bf[4];
#pragma unroll
                for (int a = 0; a < 2; a++)
                    af[a] = *reinterpret_cast<const v4i_t*>(A + mlds<KM>(wr * 64 + a * 32 + r, KM * h + q));
#pragma unroll
                for (int b = 0; b < 4; b++)
                    bf[b] = *reinterpret_cast<const v4i_t*>(B + mlds<KM>(wc * 128 + b * 32 + r, KM * h + q));
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    v4i_t an[2], bn[4];
#pragma unroll
                    for (int a = 0; a < 2; a++) an[a] = raw_nibbles((uint32_t)af[a][m]);
#pragma unroll
                    for (int b = 0; b < 4; b++) bn[b] = raw_nibbles((uint32_t)bf[b][m]);
#pragma unroll
                    for (int a = 0; a < 2; a++)
#pragma unroll
                        for (int b = 0; b < 4; b++) {
                            const v8i_t av = {an[a][0], an[a][1], an[a][2], an[a][3], 0, 0, 0, 0};
                            const v8i_t bv = {bn[b][0], bn[b][1], bn[b][2], bn[b][3], 0, 0, 0, 0};
                            acc[a][b] =
                                __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[a][b], 4, 4, 0, 0, 0, 0);
                        }
                }
            }
        } else
#pragma unroll
        for (int kk = 0; kk < KM; kk++) {
            v4i_t af[2], bf[4];
#pragma unroll
            for (int a = 0; a < 2; a++)
                af[a] = *reinterpret_cast<const v4i_t*>(A + mlds<KM>(wr * 64 + a * 32 + r, 2 * kk + h));
#pragma unroll
            for (int b = 0; b < 4; b++)
                bf[b] = *reinterpret_cast<const v4i_t*>(B + mlds<KM>(wc * 128 + b * 32 + r, 2 * kk + h));
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const v8i_t av = {af[a][0], af[a][1], af[a][2], af[a][3], 0, 0, 0, 0};
                    const v8i_t bv = {bf[b][0], bf[b][1], bf[b][2], bf[b][3], 0, 0, 0, 0};
                    acc[a][b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[a][b], 4, 4, 0, 0, 0, 0);
                }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // stage free for the next DMA
    }
    }
    // D of block (a, b): row (q & 3) + 8 (q >> 2) + 4 h of the block, column r
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const int64_t i = row0 + wr * 64 + a * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                const int64_t j = col0 + wc * 128 + b * 32 + r;
                const int v = (int)acc[a][b][q];
                if (STORE) {
                    if (i < r1 && j < c1 && !(upper && j <= i)) I[(i - r0) * ldI + (j - c0)] = v;
                } else if (v && i < r1 && j < c1 && !(upper && j <= i)) {
                    atomicAdd(I + (i - r0) * ldI + (j - c0), v);
                }
            }
}

// one query row against a column list: one wave per column, streaming
__global__ __launch_bounds__(256) void bitset_row_kernel(const unsigned long long* __restrict__ bits, int64_t W,
                                                         int64_t q, const int64_t* __restrict__ cols,
                                                         int64_t ncols, int32_t* __restrict__ I) {
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= ncols) return;
    const unsigned long long* a = bits + q * W;
    const unsigned long long* b = bits + cols[c] * W;
    uint32_t acc = 0;
    for (int64_t w = lane; w < W; w += 64) acc += __popcll(a[w] & b[w]);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) I[c] = (cols[c] == q) ? -1 : (int32_t)acc;   // -1: self pair, fixed by the epilogue
}

}  // namespace

void bitset_row(gdist_ctx* ctx, const gdist_sets* s, int64_t q, const int64_t* d_cols, int64_t ncols,
                int32_t* d_I) {
    if (ncols <= 0) return;
    bitset_row_kernel<<<(unsigned)ceil_div(ncols, 4), 256, 0, ctx->stream>>>(s->bits.as<unsigned long long>(), s->W,
                                                                             q, d_cols, ncols, d_I);
    GD_HIP(hipGetLastError());
    if (s->n_rare > 0 || s->variant) {
        DevBuf cnt(s->nsets * 4 + 4, ctx->stream);
        GD_HIP(hipMemsetAsync(cnt.p, 0, s->nsets * 4, ctx->stream));
        if (s->n_rare > 0) rare_query_launch(ctx, s, q, cnt.as<int32_t>());
        variant_query(ctx, s, q, cnt.as<int32_t>());
        gather_add_launch(ctx, d_cols, ncols, cnt.as<int32_t>(), d_I);
        GD_HIP(hipGetLastError());
        GD_HIP(hipStreamSynchronize(ctx->stream));
    }
}

MfmaChoice mfma_choice(gdist_ctx* ctx, const gdist_sets* s, const MatrixPlan& p) {
    MfmaChoice m;
    const int64_t tW = s->sparse ? s->Wd : s->W;
    // option bitset_mfma_raw (default 1): stages of the bitsets themselves,
    // expanded in registers; 0: the FP4 nibble operand
    m.raw = ctx->option(OPT_BITSET_MFMA_RAW, 1) != 0;
    m.km2 = ctx->option(OPT_BITSET_MFMA_KM, 4) == 2;
    // words a stage: raw 16 (8 with bitset_mfma_km 2), nibbles 4 (2)
    m.km = m.raw ? (m.km2 ? 8 : 16) : m.km2 ? 2 : 4;
    // option bitset_mfma_store: the MFMA tiles store their counts (one K
    // split; the side families then start after them). Off by default: the
    // tiles alone gain (C3 0.71 vs 0.76 ms) but the step loses its overlap
    // (C3 1.81 vs 1.67 ms, C4 slice span 16.9 vs 14.8 ms; profiles/r05/s26)
    // (only the raw 16-word kernel has the storing form: mstore with another
    // stage layout would give up the overlap without the stores)
    m.store = p.nmt > 0 && !s->sparse && m.raw && !m.km2 && ctx->option(OPT_BITSET_MFMA_STORE, 0) != 0 &&
              mfma_min_splits(tW / m.km, m.km) == 1;
    // raw 16-word stages: the next stage's DMA spread between the MFMAs, one
    // barrier a stage (bitset_mfma_kernel SPREAD; 0: the round-5 schedule.
    // Waves 4-7 at priority 1 as well measured neutral: C4 slice span 14.25-
    // 14.40 vs 14.08-14.63 ms, profiles/r06/s12)
    m.spread = ctx->option(OPT_BITSET_MFMA_SCHED, 1) != 0;
    // bit-plane operands (PLANE; tiles alone C3 0.709-0.714 vs 0.715-0.736 ms,
    // C4 slice 7.38-7.50 vs 7.51-7.54, spans unchanged: profiles/r06/s17)
    m.plane = ctx->option(OPT_BITSET_MFMA_PLANE, 1) != 0;
    return m;
}

void dense_tiles_launch(gdist_ctx* ctx, const gdist_sets* s, const MatrixPlan& p, const MfmaChoice& m, const Region& g,
                        bool side, int32_t* d_I, int64_t ldI) {
    hipStream_t st = ctx->stream;
    const int64_t r0 = g.r0, r1 = g.r1, c0 = g.c0, c1 = g.c1;
    const bool upper = g.upper;
    // dense tile operands: every word, or only the dense words when the
    // complement-sparse words run in their own kernel (sparse.hip)
    const unsigned long long* tbits = s->sparse ? s->dbits.as<unsigned long long>() : s->bits.as<unsigned long long>();
    const int64_t tW = s->sparse ? s->Wd : s->W;
    // no dense words, or so few that the sparse flush counts them
    if (tW == 0 || (s->sparse && s->sp_fold_dense)) return;
    FamilyTimer ft(ctx, GDIST_KERNEL_DENSE, st);
    if (p.nmt > 0) {
        // FP4 MFMA tiles: one 128 KiB workgroup per CU; K split so that
        // the grid fills ~4 rounds of the chip, each split >= 8 stages
        const int km = m.km;
        const int64_t nst = tW / km;
        // (~2 rounds when side-stream families run beside the tiles: C3's
        // 820 tiles unsplit, step 1.61 vs 1.67 ms with 2 splits, the walk
        // keeping more of the CUs; profiles/r05/s26)
        const int64_t rounds = side ? 2 : 4;
        int msp = (int)std::max<int64_t>(
            1, std::min<int64_t>(std::max<int64_t>(1, nst / 8), ceil_div((int64_t)ctx->cus * rounds, p.nmt)));
        if (ctx->has_option(OPT_BITSET_MFMA_SPLITS))      // A/B: a given K split
            msp = (int)std::max<int64_t>(1, std::min<int64_t>(nst, ctx->option(OPT_BITSET_MFMA_SPLITS, 1)));
        if (m.store) msp = 1;                             // stores: one writer a pair
        // exactness: a split's f32 accumulator sums at most 64 x (its
        // words) bits; f32 holds every integer <= 2^24 exactly, so no
        // split may span more than kMfmaMaxSplitWords words (a pair of
        // ~10 Mbp genomes on both strands shares > 2^24 dense kmers)
        msp = (int)std::max<int64_t>(msp, mfma_min_splits(nst, km));
        GD_REQUIRE(ceil_div(nst, (int64_t)msp) * km <= kMfmaMaxSplitWords, "MFMA K split past the f32 exact bound");
        const int64_t mgrid = p.nmt * msp;
        GD_REQUIRE(mgrid < (int64_t(1) << 31), "MFMA tile grid too large");
        if (!m.raw && s->fp4_W != tW) {
            // the operand as FP4 nibbles, once per set of bitsets (every
            // rebuild of the bits drops it; a capture replays a call that
            // ran uncaptured first, so the operand exists by then)
            GD_REQUIRE(!ctx->capturing, "FP4 operand built inside a capture");
            gdist_sets* ms = const_cast<gdist_sets*>(s);
            ms->fp4.alloc((size_t)s->nsets * tW * 32 + 64, st);
            fp4_expand_kernel<<<grid_for(s->nsets * tW, 256, 256 * 256), 256, 0, st>>>(
                tbits, s->nsets * tW, ms->fp4.as<uint4>());
            GD_HIP(hipGetLastError());
            ms->fp4_W = tW;
        }
        // stage ring: KM words a stage x NS stages (option bitset_mfma_ns: 2..4
        // with KM = 2; KM = 4 only double-buffered, 128 KiB either way)
        const int ns = !m.km2 ? 2 : (int)std::max<int64_t>(2, std::min<int64_t>(4, ctx->option(OPT_BITSET_MFMA_NS, 2)));
        auto mlaunch = [&](auto kern, int lds_bytes) {
            GD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
            const unsigned char* op = m.raw ? reinterpret_cast<const unsigned char*>(tbits) : s->fp4.as<unsigned char>();
            kern<<<(unsigned)mgrid, MNT, lds_bytes, st>>>(op, tW, p.mtiles.as<int2>(), (int)p.nmt, msp, nst, r0,
                                                           r1, c0, c1, upper ? 1 : 0, d_I, ldI);
        };
        if (m.raw && !m.km2 && m.store) mlaunch(&bitset_mfma_kernel<4, 2, true, true>, 2 * 2 * mopb<4>());
        else if (m.raw && !m.km2 && m.spread && m.plane)
            mlaunch(&bitset_mfma_kernel<4, 2, true, false, true, true>, 2 * 2 * mopb<4>());
        else if (m.raw && !m.km2 && m.spread) mlaunch(&bitset_mfma_kernel<4, 2, true, false, true>, 2 * 2 * mopb<4>());
        else if (m.raw && !m.km2) mlaunch(&bitset_mfma_kernel<4, 2, true>, 2 * 2 * mopb<4>());
        else if (m.raw && ns == 4) mlaunch(&bitset_mfma_kernel<2, 4, true>, 4 * 2 * mopb<2>());
        else if (m.raw && ns == 3) mlaunch(&bitset_mfma_kernel<2, 3, true>, 3 * 2 * mopb<2>());
        else if (m.raw) mlaunch(&bitset_mfma_kernel<2, 2, true>, 2 * 2 * mopb<2>());
        else if (km == 4) mlaunch(&bitset_mfma_kernel<4, 2>, 2 * 2 * mopb<4>());
        else if (ns == 4) mlaunch(&bitset_mfma_kernel<2, 4>, 4 * 2 * mopb<2>());
        else if (ns == 3) mlaunch(&bitset_mfma_kernel<2, 3>, 3 * 2 * mopb<2>());
        else mlaunch(&bitset_mfma_kernel<2, 2>, 2 * 2 * mopb<2>());
    } else {
        const int64_t nch2 = tW / KC2;
        // workgroups per CU the K-split aims for (GDIST_BITSET_WG_PER_CU, A/B)
        const int64_t wg_per_cu = std::max<int64_t>(1, ctx->option(OPT_BITSET_WG_PER_CU, 16));
        // ... but each workgroup streams at least min_kc chunks: a split's
        // prologue and its 16K accumulator atomics amortise over its chunks
        // (launches of few tiles: diagonal, partial; GDIST_BITSET_MIN_CHUNKS, A/B)
        const int64_t min_kc = std::max<int64_t>(1, ctx->option(OPT_BITSET_MIN_CHUNKS, 16));
        const int64_t corg = p.corg;
        auto launch = [&](auto kern, const int2* dtiles, size_t nt) {
            if (nt == 0) return;
            const int64_t target2 = (int64_t)ctx->cus * wg_per_cu;
            const int sp2 = (int)std::max<int64_t>(
                1, std::min<int64_t>(std::max<int64_t>(1, nch2 / min_kc), ceil_div(target2, (int64_t)nt)));
            const int64_t grid2 = (int64_t)nt * sp2;
            GD_REQUIRE(grid2 < (int64_t(1) << 31), "bitset matrix grid too large");
            kern<<<(unsigned)grid2, NT, 0, st>>>(tbits, tW, dtiles, (int)nt, sp2, nch2,
                                                 r0, r1, c0, c1, corg, upper ? 1 : 0, d_I, ldI);
        };
        const int2* dg = p.tiles.as<int2>();
        const size_t* at = p.at;
        launch(bitset_tile_kernel2<false>, dg, at[1]);
        launch(bitset_tile_kernel2<true>, dg + at[1], at[2] - at[1]);
        auto partial = [&](auto off_k, auto diag_k) {
            launch(off_k, dg + at[2], at[3] - at[2]);
            launch(diag_k, dg + at[3], at[4] - at[3]);
        };
        switch (p.part ? p.rr : 8) {
            case 1: partial(bitset_tile_kernel2<false, 1>, bitset_tile_kernel2<true, 1>); break;
            case 2: partial(bitset_tile_kernel2<false, 2>, bitset_tile_kernel2<true, 2>); break;
            case 3: partial(bitset_tile_kernel2<false, 3>, bitset_tile_kernel2<true, 3>); break;
            case 4: partial(bitset_tile_kernel2<false, 4>, bitset_tile_kernel2<true, 4>); break;
            case 5: partial(bitset_tile_kernel2<false, 5>, bitset_tile_kernel2<true, 5>); break;
            case 6: partial(bitset_tile_kernel2<false, 6>, bitset_tile_kernel2<true, 6>); break;
            case 7: partial(bitset_tile_kernel2<false, 7>, bitset_tile_kernel2<true, 7>); break;
            default: break;   // no partial row tile
        }
    }
    ft.end();
}

}  // namespace gdist
