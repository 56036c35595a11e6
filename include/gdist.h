/*
 * gdist.h — C-ABI of the MI355X-native pairwise kmer-distance hot path of
 * SEEDtk genome.distance (libgdist.so).
 *
 * Plain C types only: pointers, sizes and status codes. No torch, no C++.
 * Every entry point returns GDIST_OK (0) or a negative GDIST_E* code; the
 * message of the last failure on the calling thread is gdist_last_error().
 *
 * What each entry point replaces in the reference (paths relative to the
 * reference root /root/reference; the kmer classes live in the un-vendored
 * org.theseed:sequence:1.0.0 module, pom.xml:46-49, so their behaviour is
 * taken from the in-repo call sites):
 *
 *   gdist_sets_pack        KmerType.createKmers(seq, K)          FastaDistanceProcessor.java:153,184
 *                          new GenomeKmers(genome)               GenomeProcessor.java:109,139
 *                          new ProteinKmers(seq)                 ProteinKmerReader.java:101
 *   gdist_sets_sizes       SequenceKmers.size()                  (used by distance())
 *   gdist_intersect_matrix SequenceKmers.distance(other) over the
 *                          N×N upper triangle                    FastaDistanceProcessor.java:177-186
 *                          M×N rectangle                         GenomeProcessor.java:140
 *                          group all-pairs                       WidthProcessor.java:159-165
 *   gdist_row_query        anyMatch(d <= maxDist)                DistanceRepsProcessor.java:190
 *                          reduce(NULL_RESULT, merge) argmin     DistanceRepsProcessor.java:238-239
 *                          sequential early exit                 FastaDistanceRepsProcessor.java:117-128
 *   gdist_sketch_build     SequenceKmers.hashSet(width)          SketchProcessor.java:88, WidthProcessor.java:178
 *   gdist_sketch_matrix    Sketch.distance(other) all-pairs      WidthProcessor.java:183-185, TuningProcessor.java:131-133
 *   gdist_sketch_pairs     Sketch.distance(other) over an (id1, id2)
 *                          list, beside the exact kmer column    MethodTableProcessor.java:258-276
 *                          the sketch-against-exact comparison
 *                          over chosen pairs                     WidthProcessor.java:183-192
 *   gdist_sketch_greedy_reps the distReps / fastaReps selection with
 *                          Sketch.distance as the distance       DistanceRepsProcessor.java:185-200,227-237
 *   gdist_width_sweep      the per-size loop of ProcessGroup: sketch
 *                          error at every sketch size of a list  WidthProcessor.java:153-208
 *   gdist_closest          getClosest(kmers, n, maxDist), exhaustively
 *                          (every column, no LSH buckets)        MashProcessor.java:150, FindProcessor.java:110
 *                          --maxDist of the genomes table        GenomeProcessor.java:58-60,89
 *   gdist_within           the documented -m filter of the table GenomeProcessor.java:35
 *                          (every pair with d <= maxDist)
 *   gdist_pairs            getDistance over an (id1, id2) list   MethodTableProcessor.java:258-276
 *                          the lists of the pairs commands       BasicPairsProcessor.java:71-89, PairCreateProcessor.java:29-32
 *   gdist_cross_closest    getClosest(kmers, n, maxDist) per new genome
 *                          against the loaded genome database    FindProcessor.java:94-110, MashProcessor.java:150
 *   gdist_cross_matrix     the same queries x database rectangle
 *                          as counts and distances               GenomeProcessor.java:140
 *   gdist_cross_pairs      getDistance over an (id1, id2) list of
 *                          new genomes x database genomes        MethodTableProcessor.java:258-276
 *   gdist_cross_within     the -m filter of comparison genomes
 *                          against the pre-loaded base genomes   GenomeProcessor.java:35,140
 *   gdist_cross_group_stats in / out-group summary of new genomes
 *                          against the database                  DistanceCheckProcessor.java:200-223
 *   gdist_cross_histogram  the bucket report of new genomes
 *                          against the database                  TaxCheckProcessor.java:133-135
 *   gdist_group_stats      recordDistance over a distance table  GroupTypeSpec.java:77-95
 *                          in / out-group min, mean, sd, max     DistanceCheckProcessor.java:200-223
 *   gdist_histogram        new Distributor(0.0, 1.0, 50)         TaxCheckProcessor.java:93
 *                          fed every (method; group) series      TaxCheckProcessor.java:133-135
 *                          the count of pairs with d < 1.0       WidthProcessor.java:162
 *                          the close pairs below the target      TuningProcessor.java:131-133
 *   gdist_sets_allgather   (new) RCCL all-gather of packed sets for row-sharded N×N
 *
 * Kmer code spec (shared by the device packer, the CPU oracle in oracle/ and
 * the Python restatement; see DESIGN.md "Packing spec"). A kmer is k
 * consecutive characters of the sequence after case folding; its code is an
 * order-preserving (code order == Java String order) injective uint64:
 *   DNA, AMBIG_SKIP (default): 2-bit A0 C1 G2 T3, first char most significant,
 *        k <= 32; kmers holding any other char are skipped.
 *   DNA, AMBIG_KEEP: 3-bit A0 C1 G2 N3 R4 T5 Y6, k <= 21; any other char -> EINVAL.
 *   PROT, k <= 8: the k ASCII bytes big-endian (any byte value).
 *   PROT, 8 < k <= 12: 5-bit '*'0 'A'..'Z' 1..26; any other char -> EINVAL.
 *   PROT, AMBIG_SKIP: kmers holding a char outside ACDEFGHIKLMNPQRSTVWY skipped.
 * Byte 0x00 is a sequence separator in every mode: no kmer spans it (used to
 * pack the contigs of one genome, or the proteins of one group, as one set).
 * DNA strand modes: FWD (forward only), BOTH (forward kmers ∪ reverse-
 * complement kmers, the default), CANON (per-position min(fwd, rc)).
 * Distance: d = (I > 0) ? 1.0 - (double)I / (double)(|A|+|B|-I) : 1.0
 * (GDIST_EMPTY_NAN turns the I == 0 && |A|+|B| == 0 case into NaN), fp64,
 * no contraction: bit-identical to the Java expression.
 */
#ifndef GDIST_H
#define GDIST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDIST_ABI_VERSION 1

/* status codes */
#define GDIST_OK        0
#define GDIST_EINVAL   -1   /* bad argument / unencodable input        -> IllegalArgumentException */
#define GDIST_ENOMEM   -2   /* host or device allocation failed         -> OutOfMemoryError */
#define GDIST_EDEVICE  -3   /* HIP runtime / kernel failure             -> IllegalStateException */
#define GDIST_ECOMM    -4   /* RCCL failure                             -> IllegalStateException */

/* set kinds (KmerType) */
#define GDIST_DNA     0
#define GDIST_PROT    1
#define GDIST_SKETCH  2

/* pack flags */
#define GDIST_STRAND_BOTH   0x0u   /* default for DNA */
#define GDIST_STRAND_FWD    0x1u
#define GDIST_STRAND_CANON  0x2u
#define GDIST_STRAND_MASK   0x3u
#define GDIST_AMBIG_DEFAULT 0x0u   /* DNA: skip, PROT: keep */
#define GDIST_AMBIG_SKIP    0x4u
#define GDIST_AMBIG_KEEP    0x8u
#define GDIST_AMBIG_MASK    0xCu
#define GDIST_NO_CASE_FOLD  0x10u  /* PROT only; DNA always folds to upper case */

/* distance / matrix flags */
#define GDIST_UPPER_TRIANGLE 0x100u /* only pairs with global col > global row */
#define GDIST_OUT_DEVICE     0x200u /* I_out / D_out are device pointers (gdist_dev_alloc); the call
                                       returns once its work is queued on the context's stream:
                                       gdist_ctx_synchronize, gdist_memcpy_d2h or the next call that
                                       reads results waits for it */
#define GDIST_EMPTY_NAN      0x400u /* |A|+|B| == 0 -> NaN instead of 1.0 */
#define GDIST_SKETCH_JACCARD 0x800u /* sketch distance: plain Jaccard of the two signatures
                                       (default: Mash bottom-s of the union) */

/* intersection methods */
#define GDIST_METHOD_AUTO    0   /* bitsets if built; when the sorted join's estimate for the
                                    region exceeds ~20 ms, build the two-tier dictionary and
                                    keep it when its cost estimate beats the sorted join */
#define GDIST_METHOD_SORTED  1   /* sorted uint64 sets: LDS hash-join tiles */
#define GDIST_METHOD_BITSET  2   /* dictionary-rank bitsets: AND + popcount tiles */

/* bitset build flags */
#define GDIST_BITSET_KEEP_SINGLETONS 0x1u /* keep kmers present in only one set
                                             (default prunes them: they never intersect) */

/* row-query modes */
#define GDIST_QUERY_ALL     0
#define GDIST_QUERY_ANY_LE  1
#define GDIST_QUERY_ARGMIN  2

typedef struct gdist_ctx  gdist_ctx;
typedef struct gdist_sets gdist_sets;
typedef struct gdist_lsh  gdist_lsh;

/* ---- library / context ---------------------------------------------- */
const char* gdist_version(void);
/* sha256 prefix (16 hex) of the sources the library was built from
 * (csrc/ *.hip in name order, csrc/gdist_internal.hpp, include/gdist.h):
 * a stale build is detectable against the tree it runs from. */
const char* gdist_source_hash(void);
int  gdist_abi_version(void);
const char* gdist_last_error(void);                 /* thread-local */
int  gdist_device_count(int* n);
int  gdist_ctx_create(int device, gdist_ctx** out);
int  gdist_ctx_destroy(gdist_ctx* ctx);
int  gdist_ctx_synchronize(gdist_ctx* ctx);
/* HIP-event time of the last intersect/sketch matrix call's main kernel(s)
 * and of the whole call, in ms (recorded on the stream they run on); NaN when
 * the call recorded none (a graph-replayed step into device outputs records
 * no events unless option "step_timing" = 1; a call without a kernel of its
 * own has no kernel time). */
int  gdist_ctx_last_timing(gdist_ctx* ctx, double* kernel_ms, double* call_ms, int64_t* launches);
/* Kernel times (ms, HIP events on the stream they ran on) of the last
 * min(max, 256) matrix calls, oldest first, *count of them; waits for them. */
int  gdist_ctx_recent_timings(gdist_ctx* ctx, int max, double* kernel_ms, int* count);
/* HIP-event time (ms) of one kernel family's launches alone, on the stream
 * they ran on, in the last matrix call made with option "time_kernels" = 1
 * (such calls are not graph-replayed); -1 when that family was not timed.
 * Waits for it. Families: the sparse tile launch (with the rare rows it
 * carries), the rare-tier kernel (list- or row-major), the dense tile
 * launches, the sorted join. */
#define GDIST_KERNEL_SPARSE 0
#define GDIST_KERNEL_RARE   1
#define GDIST_KERNEL_DENSE  2
#define GDIST_KERNEL_SORTED 3
#define GDIST_KERNEL_VARIANT 4
int  gdist_ctx_kernel_ms(gdist_ctx* ctx, int family, double* ms);
/* Tuning options of a context: the A/B switches of DESIGN.md §5 by name
 * ("rare_t", "bitset_diag", "sparse", "sparse_zmax", "sketch_k", ...;
 * gdist_ctx_option_name enumerates them, EINVAL past the last). Every option
 * defaults to the measured best; GDIST_OPTION_DEFAULT restores it. No option
 * changes a result: each picks among exact kernels, tilings, thresholds or
 * setup paths, and the parity tests run every non-default value against the
 * oracle; an unknown name is EINVAL. The
 * library never reads the environment, so every host (JNI, ctypes) sharing a
 * context gets the same kernels (concurrent getDistance callers,
 * MethodTableProcessor.java:275). Options read at build time (rare_t,
 * rare_dedup, locus_order, sparse, sparse_zmax, guides) apply to collections
 * packed or built after the call. */
#define GDIST_OPTION_DEFAULT INT64_MIN
int  gdist_ctx_set_option(gdist_ctx* ctx, const char* name, int64_t value);
int  gdist_ctx_get_option(gdist_ctx* ctx, const char* name, int64_t* value, int* is_set);
int  gdist_ctx_option_name(int index, const char** name);
int  gdist_dev_alloc(gdist_ctx* ctx, int64_t bytes, void** dptr);
int  gdist_dev_free(gdist_ctx* ctx, void* dptr);
int  gdist_memcpy_d2h(gdist_ctx* ctx, void* dst, const void* src, int64_t bytes);
int  gdist_memcpy_h2d(gdist_ctx* ctx, void* dst, const void* src, int64_t bytes);
/* Page-locked host memory for sequence bytes (a FASTA reader fills it in
 * place): gdist_sets_pack uploads such a buffer with one DMA per pack chunk
 * at the link's rate instead of the runtime's staged pageable copies. */
int  gdist_host_alloc(int64_t bytes, void** hptr);
/* Return the library's cached device blocks of `device` (freed buffers it
 * keeps for reuse) to the driver, e.g. before another process takes the
 * GPU. Blocks in use are untouched. */
int  gdist_release_cache(int device);
int  gdist_host_free(void* hptr);

/* ---- kmer sets ------------------------------------------------------- */
/* Build kmer sets of nseqs sequences on the device. seqs is the byte
 * concatenation, sequence s = seqs[seq_off[s] .. seq_off[s+1]). The call
 * is synchronous; inside it a short-lived host thread of the library
 * uploads the bytes of pack chunk c + 1 while chunk c is packed (option
 * "pack_overlap"), so seqs is read until the call returns. */
/* seqs in a gdist_host_alloc buffer: one DMA per chunk (detected). */
int  gdist_sets_pack(gdist_ctx* ctx, int kind, int k, unsigned flags,
                     const char* seqs, const int64_t* seq_off, int64_t nseqs,
                     gdist_sets** out);
/* Same, but the sequences are already in device memory (no H2D). */
int  gdist_sets_pack_device(gdist_ctx* ctx, int kind, int k, unsigned flags,
                            const char* d_seqs, const int64_t* d_seq_off, int64_t nseqs,
                            int64_t total_bytes, gdist_sets** out);
/* Pack nseqs more sequences with the collection's kmer spec (kind, k, flags)
 * and append them as sets nsets .. nsets + nseqs - 1 (*first = the old nsets).
 * Replaces `new GenomeKmers(genome)` for a genome seen for the first time by
 * a cache that packs each genome once (MethodTableProcessor.java:261-275 via
 * jni/GpuKmerMethod.java). Every derived representation (bitsets, tiers,
 * plans, the sorted join's index) is dropped and rebuilt on the next call;
 * the codes grow in place, doubling when full.
 * A failed append (an unencodable sequence, bad offsets: EINVAL) returns
 * before anything of the collection is touched: its codes, every derived
 * representation and nsets are as before the call. An append of zero
 * sequences changes nothing and keeps built bitsets (*first = nsets). A
 * collection from gdist_sets_upload carries no pack flags and appends with
 * the default ones (flags 0); a gdist_sets_concat result appends with its
 * first input's. */
int  gdist_sets_append(gdist_ctx* ctx, gdist_sets* sets, const char* seqs, const int64_t* seq_off,
                       int64_t nseqs, int64_t* first);
/* Adopt caller-packed sets: CSR of sorted, unique codes (host arrays, copied). */
int  gdist_sets_upload(gdist_ctx* ctx, int kind, int k, int64_t nsets,
                       const int64_t* offsets, const uint64_t* codes, gdist_sets** out);
int  gdist_sets_free(gdist_sets* sets);
int  gdist_sets_info(const gdist_sets* sets, int* kind, int* k, int64_t* nsets, int64_t* total_codes);
int  gdist_sets_sizes(const gdist_sets* sets, int64_t* sizes);           /* nsets values */
int  gdist_sets_download(const gdist_sets* sets, int64_t* offsets, uint64_t* codes);
/* Build the dictionary-rank bitset representation (kept with the sets).
 * Two exact tiers: kmers held by >= T sets are bit columns of the dense
 * bitsets (AND + popcount tiles); kmers held by 2..T-1 sets are posting lists
 * whose m(m-1)/2 pairs are counted directly. _ex sets T (-1 = automatic,
 * 0..2 = dense only); KEEP_SINGLETONS forces a dense-only dictionary of
 * every distinct kmer. */
int  gdist_sets_build_bitsets(gdist_sets* sets, unsigned flags);
int  gdist_sets_build_bitsets_ex(gdist_sets* sets, unsigned flags, int64_t rare_threshold);
/* A collection the code all-gather returned (gdist_sets_allgather_ex) is the
 * same on every rank; its bitset build is then collective and split by rank
 * (option "split_build", default on): rank r counts 1/R of the code ranges
 * of the dictionary summary and fills the tiers of sets [r m, (r + 1) m),
 * m = ceil(N / R); the summary, bitset rows, rare records and variant entries
 * are all-gathered, and every rank holds the whole representation (the same
 * on every rank as a one-rank build). Every rank must make the build call
 * (build_bitsets, prepare, or a BITSET/AUTO matrix call that builds; AUTO
 * builds on every rank when any rank's region asks for it). The setup step of
 * FastaDistanceProcessor.java:150-155 (the reference builds every batch's
 * kmer sets on one host). */
/* Release the codes of a collection whose bitsets are built (the C4 code
 * all-gather's 160 GB per rank): the collection keeps its bitset tiers and
 * sizes and answers METHOD_BITSET / AUTO calls; the sorted join, sketches, a
 * rebuild and appends need codes and refuse it (EINVAL). */
int  gdist_sets_release_codes(gdist_sets* sets);
/* The last bitset build: wall time (ms), the time of its split stages (the
 * summary's code ranges and the fill's sets, all shares) and of the largest
 * share, and the shares (1: not split). One rank of a split build ran one
 * share; option "split_build" = k on one rank runs k shares in turn, so that
 * build_ms - split_ms + share_max_ms is one rank's build of 1/k of the sets. */
int  gdist_sets_build_timing(const gdist_sets* sets, double* build_ms, double* split_ms, double* share_max_ms,
                             int* shares);
/* Rare tier: threshold T, distinct posting lists and their member records.
 * Kmers with identical posting lists (e.g. every kmer covering one shared
 * variant) are one list weighted by their number (option "rare_dedup" = 0: one
 * list per kmer); gdist_sets_rare_kmers gives the kmers before merging. */
int  gdist_sets_rare_info(const gdist_sets* sets, int64_t* threshold, int64_t* lists, int64_t* records);
int  gdist_sets_rare_kmers(const gdist_sets* sets, int64_t* kmers);
/* Rare-tier statistics behind the cost model: pair increments (sum of
 * m(m-1)/2 over the posting lists) and the longest list. */
int  gdist_sets_rare_stats(const gdist_sets* sets, int64_t* pair_incs, int64_t* max_list);
int  gdist_sets_bitset_info(const gdist_sets* sets, int64_t* dict_size, int64_t* words_per_set);
/* Complement-sparse words of the dense tier: the dense
 * dictionary is ranked in locus order (the kmer's window in the collection's
 * first sequences), and each bitset word that few sets lack anything in is
 * counted from the sets' complement words instead of the AND+popcount tiles.
 * Reports the sparse words, the dense words left to the tiles (padded) and
 * the complement entries (0s when the split was not worth building).
 * Options "sparse" = 0 / "locus_order" = 0 switch it off (A/B). */
int  gdist_sets_sparse_info(const gdist_sets* sets, int64_t* sparse_words, int64_t* dense_words, int64_t* entries);
/* The variant tier: kmers held by T .. Dmin - 1 sets (Dmin:
 * option "variant_dmin", default N / 10) grouped by the substitution that
 * made them into 64-kmer words, each a list of (set, 64-bit mask) entries;
 * a pair adds popc(mask_i & mask_j) per shared word. Built by the bitset
 * build when those kmers dominate the dictionary (option "variant": 1
 * forces, 0 never). Reports the kmers, words, entries and the walk's
 * products (sum over words of z(z-1)/2); zeros without the tier. */
int  gdist_sets_variant_info(const gdist_sets* sets, int64_t* kmers, int64_t* words, int64_t* entries,
                             double* products);
/* The variant tier's layout: kmers a word (47 or 64, option variant_bits;
 * 16 for the grouped rare tier, option rare_group), the bytes of a list
 * member the walk reads (4: set | mask << 16 of the short-list walk, 16-kmer
 * words of <= 65,536 sets; 8: set << 47 | mask, 47-kmer words of < 2^17
 * sets; 12: the 4-byte set and 8-byte mask arrays), and the largest sum of a
 * set's entry popcounts (16-bit counters below 2^16; 4-byte layout only).
 * Zeros without a variant tier. Diagnostics (bench roofline). */
int  gdist_sets_variant_layout(const gdist_sets* sets, int* word_kmers, int* member_bytes, int64_t* row_weight_max);
/* The sparse words by side: counted from the sets' complement words (sets
 * lacking a commonly held kmer) or from their words (sets holding a rarely
 * held one: positive-sparse). */
int  gdist_sets_sparse_sides(const gdist_sets* sets, int64_t* complement_words, int64_t* positive_words);
/* The sparse tile kernel's products over the whole collection: the sum over
 * the sparse words of z (z - 1) / 2 (z = the word's entries), each pair of a
 * word's entries once (0 without the split). Diagnostics: the bench line's
 * VALU per 64 products. */
int  gdist_sets_sparse_pairs(const gdist_sets* sets, double* pairs);
/* The triple records of the sparse words (the 3 x 3 walk of
 * option "sparse_mt" 3): every (set block, sparse word) list of n entries as
 * ceil(n / 3) records. out[0] = the records, out[1..4] = the lists that are
 * empty and those with n mod 3 = 1, 2 and 0 (n > 0), counted at build time.
 * Zeros without the split, or where the records were left out (more than
 * 2^27 of them). Diagnostics and tests. */
int  gdist_sets_sparse_triples(const gdist_sets* sets, int64_t* out);
/* The group tier of the sparse words: groups of sets (e.g.
 * the clades of a structured collection) whose members all carry the same
 * pattern in a word; those words keep per member only the residual entries
 * and the group part of a pair is evaluated from per-group tables (T, V)
 * with the pair's constant part. Reports the groups used
 * and the sparse words factorised by one (0s without the tier; option
 * "sparse_groups" = 0 switches it off). */
int  gdist_sets_group_info(const gdist_sets* sets, int64_t* groups, int64_t* grouped_words);
/* Copy the bitsets (nsets x words_per_set uint64, row-major) to the host. */
int  gdist_sets_bitset_download(const gdist_sets* sets, uint64_t* bits);
/* Concatenate two collections (e.g. base genomes + comparison genomes): a's
 * sets, then b's, both kmer sets of one kind, k, strand and ambiguity flags
 * (GDIST_NO_CASE_FOLD may differ) or both sketches of one width and kmer
 * spec; anything else is EINVAL and leaves both inputs as they were. The
 * result is a deep copy, independent of its inputs: either may be appended
 * to or freed afterwards, and appending to the result touches neither. It
 * holds codes (signatures) only, no derived representation, and carries a's
 * pack flags, which a later gdist_sets_append to it uses. */
int  gdist_sets_concat(const gdist_sets* a, const gdist_sets* b, gdist_sets** out);

/* ---- distances ------------------------------------------------------- */
/* Prepare the representation `method` needs for a region of `pairs` pairs
 * (pairs < 0: the whole N(N-1)/2 triangle) and report the method a later
 * gdist_intersect_matrix(method) call will run (*chosen: SORTED or BITSET).
 * With METHOD_AUTO this is where the two-tier dictionary is built and costed;
 * *cost_bitset_s / *cost_sorted_s (may be NULL) return the model's estimates
 * (-1 when no bitsets are held). The setup step of FastaDistanceProcessor.java:150-155
 * (a batch's kmer sets are built and cached before its pair loop). */
int  gdist_sets_prepare(gdist_ctx* ctx, gdist_sets* sets, int method, double pairs, int* chosen,
                        double* cost_bitset_s, double* cost_sorted_s);
/* Pairs (i, j), r0 <= i < r1, c0 <= j < c1 (global set indices of `sets`).
 * I_out[(i-r0)*ld + (j-c0)] = |A_i ∩ A_j|, D_out[...] = distance; either
 * output may be NULL. With GDIST_UPPER_TRIANGLE, entries with j <= i are
 * left untouched.
 * Ordering of device outputs (GDIST_OUT_DEVICE): a call's I_out and D_out are
 * complete in the order of the context's stream, whatever streams the library
 * launched on (repeated fused sparse steps run their tile kernels on two
 * further streams so that consecutive calls overlap; each call's reduce, the
 * only writer of its outputs, stays on the context's stream). Every later
 * call on the context (a download, another query, a free, a rebuild) is
 * ordered behind them, gdist_ctx_synchronize waits for them, and consecutive
 * calls may share output buffers: they are written in call order. */
int  gdist_intersect_matrix(gdist_ctx* ctx, const gdist_sets* sets,
                            int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                            int method, unsigned flags,
                            int32_t* I_out, double* D_out, int64_t ld);
/* How the context's repeated gdist_intersect_matrix calls into device outputs
 * went out so far: out[0] fused sparse steps issued pipelined (tile launch on
 * a tile stream, reduce on the context's stream), out[1] those of them that
 * were fully ordered behind the context's stream first (a plan's first step
 * of a run, another collection, or any other API call in between), out[2]
 * steps replayed as one hipGraph on the context's stream (every step under
 * option "serial_step" = 1), out[3] bytes of second buffer copies (chunk
 * partials, rare slab) the pipelined plans hold. */
int  gdist_ctx_step_info(gdist_ctx* ctx, int64_t out[4]);
/* Greedy representatives over the whole collection, on the device.
 * Pass 1 (DistanceRepsProcessor.java:185-200, FastaDistanceRepsProcessor.java:
 * 117-144): sets in index order; set k becomes a representative unless an
 * earlier representative lies within max_dist (d <= max_dist); is_rep[k] =
 * 1 / 0, *nreps = their number. Keys are assumed unique (the reference's
 * repMap.put would replace a representative with the same id).
 * Pass 2, when rep_of or rep_dist is non-NULL (DistanceRepsProcessor.java:
 * 227-237): every set's closest representative, ties to the lowest
 * tie_rank (NULL: index), d < 1.0 only (NULL_RESULT identity); a
 * representative maps to itself at 0.0; -1 / 1.0 when none. */
int  gdist_greedy_reps(gdist_ctx* ctx, const gdist_sets* sets, int method, double max_dist,
                       const int64_t* tie_rank, int32_t* is_rep, int64_t* rep_of, double* rep_dist,
                       int64_t* nreps);
/* One query set q against ncols sets (indices cols[]):
 *  ALL:    D_out[c] for every c
 *  ANY_LE: *hit = 1 if any distance <= t (D_out may be NULL)
 *  ARGMIN: *best_idx = position in cols[] of the smallest distance (ties ->
 *          lowest position), *best_d = that distance; -1 / 1.0 when no
 *          distance is below 1.0 (the reference's NULL_RESULT identity wins
 *          ties at 1.0, DistanceRepsProcessor.java:108-122). */
int  gdist_row_query(gdist_ctx* ctx, const gdist_sets* sets, int64_t q,
                     const int64_t* cols, int64_t ncols, int mode, double t,
                     double* D_out, int32_t* hit, int64_t* best_idx, double* best_d);

/* ---- MinHash sketches ------------------------------------------------ */
/* Bottom-`width` signature per set: the width smallest distinct
 * murmur3_x86_32(seed 0) hashes (signed int order) of the kmer strings. */
int  gdist_sketch_build(gdist_ctx* ctx, const gdist_sets* sets, int width, gdist_sets** out);
int  gdist_sketch_upload(gdist_ctx* ctx, int width, int64_t nsets, const int64_t* offsets,
                         const int32_t* sigs, gdist_sets** out);
int  gdist_sketch_download(const gdist_sets* sk, int64_t* offsets, int32_t* sigs);
int  gdist_sketch_matrix(gdist_ctx* ctx, const gdist_sets* sk,
                         int64_t r0, int64_t r1, int64_t c0, int64_t c1, unsigned flags,
                         int32_t* common_out, double* D_out, int64_t ld);
/* Sketch.distance over a pair list (MethodTableProcessor.java:258-276; the
 * chosen pairs of WidthProcessor.java:183-192): for p in [0, npairs)
 * common_out[p] and D_out[p] are the common count and the sketch distance of
 * signature rows[p] of `a` and signature cols[p] of `b`, host arrays, either
 * may be NULL. `a` and `b` are two GDIST_SKETCH collections of `ctx` with one
 * width and one kmer spec (what gdist_sets_concat accepts); the same handle
 * may be passed for both (the one-collection pair list). Both are only read:
 * nothing is built or kept on either.
 *
 * The list may come in any order, may repeat a pair and, with one handle, may
 * hold i == j: output slot p depends on (rows[p], cols[p], flags) only, not on
 * the order, the rest of the list or the run. Both outputs are bit for bit
 * what gdist_cross_matrix(ctx, a, b, ...) writes for cell (rows[p], cols[p])
 * with the same flags; with one handle that is gdist_sketch_matrix's cell, for
 * i == j the diagonal one (common = the signature's length, d = 0.0, or the
 * empty value of an empty signature). flags: GDIST_EMPTY_NAN and
 * GDIST_SKETCH_JACCARD, as in gdist_sketch_matrix.
 *
 * The list is uploaded once, sorted by row on the device and cut into work
 * units there (a row and at most 64 of its pairs; a signature is at most
 * `width` hashes, so a pair is never split); a workgroup stages a unit's row
 * signature on chip once and a wave merges each of its pairs; the outputs come
 * back in one download and nothing at or past npairs is touched.
 * gdist_ctx_pairs_info then reports this call: groups = the distinct rows of
 * the list, units = the sum over them of ceil(pairs of the row / 64).
 * npairs == 0: GDIST_OK, nothing is touched (rows and cols may be NULL).
 * EINVAL, decided before any work (the outputs stay untouched): a null handle,
 * a handle of another context, a collection of kmer sets on either side
 * (gdist_pairs takes those), widths or kmer specs gdist_sets_concat would
 * refuse, npairs < 0 or >= 2^31, null rows or cols or both outputs null with
 * npairs > 0, any other flag, a rows[p] outside [0, nsets of a), a cols[p]
 * outside [0, nsets of b). */
int  gdist_sketch_pairs(gdist_ctx* ctx, const gdist_sets* a, const gdist_sets* b, int64_t npairs,
                        const int64_t* rows /* into a */, const int64_t* cols /* into b */, unsigned flags,
                        int32_t* common_out, double* D_out);
/* Greedy representatives of a sketch collection: gdist_greedy_reps's contract
 * (pass 1 DistanceRepsProcessor.java:185-200, pass 2 :227-237) with d the
 * sketch distance, bit for bit gdist_sketch_matrix's cell under the same
 * flags (GDIST_EMPTY_NAN and GDIST_SKETCH_JACCARD, no other).
 * Pass 1: signatures in index order; signature k becomes a representative
 * unless an earlier representative r has d(k, r) <= max_dist, a plain fp64
 * comparison: NaN (an empty pair under GDIST_EMPTY_NAN) never covers, d == 1.0
 * covers when max_dist >= 1.0. is_rep[k] = 1 / 0 for every k, *nreps = their
 * number (nreps may be NULL).
 * Pass 2, when rep_of or rep_dist is non-NULL: every signature's closest
 * representative, the least (d, tie_rank[representative]) over the
 * representatives with d < 1.0 (tie_rank NULL: the set index; NaN is never
 * closest); a representative maps to itself at 0.0; -1 / 1.0 when none.
 *
 * Only distances to representatives, and those inside a row block, are
 * computed: per row block the ring kernel runs over the list of the
 * representatives chosen so far (a column list, not a range), a second kernel
 * says which rows one of them covers, and the host resolves the order inside
 * the block from the block's own tile. The row block is gdist_greedy_reps's
 * (option "reps_block" overrides it); the ring follows the options
 * "sketch_cap", "sketch_ring", "sketch_wait" and "sketch_perm" as
 * gdist_sketch_matrix's ring does. The collection is only read. On several
 * ranks a gathered or replicated collection is answered whole on every rank.
 * nsets == 0: GDIST_OK, *nreps = 0, nothing else is touched.
 * EINVAL, decided before any work (the outputs stay untouched): a null handle,
 * a handle of another context, a collection of kmer sets (gdist_greedy_reps
 * takes those), a null is_rep, any other flag. */
int  gdist_sketch_greedy_reps(gdist_ctx* ctx, const gdist_sets* sk, double max_dist, unsigned flags,
                              const int64_t* tie_rank, int32_t* is_rep, int64_t* rep_of, double* rep_dist,
                              int64_t* nreps);
/* The context's last gdist_sketch_greedy_reps call: out[0] the row blocks of
 * pass 1, out[1] the (row, representative) cells its column-list launches
 * covered in pass 1 (the sum over the blocks of rows x representatives chosen
 * before the block), out[2] the same for pass 2 (nsets x representatives, 0
 * when neither rep_of nor rep_dist was asked for), out[3] the column-list
 * launches. Zeros before any such call. */
int  gdist_ctx_reps_info(gdist_ctx* ctx, int64_t out[4]);

/* ---- LSH bucket query (MashProcessor / FindProcessor) ------------------ */
/* Index of a sketch collection: new LSHMemSeqHash(width, stages, buckets)
 * + add() per subject (MashProcessor.java:110,130; BuildProcessor.java:131,148).
 * Stage t files a sketch in bucket (min over its signature of a salted
 * splitmix64 mix) mod buckets; seed picks the salts. The sketches must
 * outlive the index. (Restated: the LSH classes are un-vendored.) */
int  gdist_lsh_build(gdist_ctx* ctx, const gdist_sets* sketches, int stages, int buckets, uint64_t seed,
                     gdist_lsh** out);
int  gdist_lsh_free(gdist_lsh* lsh);
/* getClosest(kmers, n, maxDist) for every query sketch (MashProcessor.java:150,
 * FindProcessor.java:110): among the indexed sets sharing a bucket with the
 * query in any stage, those at sketch distance <= max_dist, nearest first
 * (ties by index), at most n: idx_out[q*n + r], d_out[q*n + r], count_out[q]. */
int  gdist_lsh_closest(gdist_ctx* ctx, const gdist_lsh* lsh, const gdist_sets* queries, int n, double max_dist,
                       int64_t* idx_out, double* d_out, int32_t* count_out);

/* ---- exact nearest neighbours ----------------------------------------- */
/* getClosest(kmers, n, maxDist) (MashProcessor.java:150, FindProcessor.java:110)
 * over every column instead of the LSH buckets: for every query set q in
 * [r0, r1) the columns j in [c0, c1) with d(q, j) <= max_dist (j = q excluded
 * unless GDIST_CLOSEST_KEEP_SELF), ordered by (d ascending as fp64, j
 * ascending), the first n of them. Host outputs laid out as gdist_lsh_closest:
 * idx_out[(q-r0)*n + r] the global set index of the r-th neighbour,
 * d_out[(q-r0)*n + r] its distance, count_out[q-r0] the neighbours found;
 * slots at or past the count are -1 / 1.0. d is bit-identical to the D of
 * gdist_intersect_matrix (kmer sets: method AUTO / SORTED / BITSET) or
 * gdist_sketch_matrix (GDIST_SKETCH collections: method ignored,
 * GDIST_SKETCH_JACCARD honoured) with the same flags; NaN (GDIST_EMPTY_NAN)
 * never qualifies, d == 1.0 does when max_dist >= 1.0 (a plain <=, not the
 * ARGMIN identity rule). Queries against other subjects (M×N): one collection
 * through gdist_sets_concat. The N×N never leaves the device: row blocks x
 * column chunks (options "closest_rows" / "closest_cols", defaults by memory)
 * are selected from as the matrix kernels produce them, and for kmer sets D
 * is never written. n == 0 or an empty range: GDIST_OK, counts 0. EINVAL:
 * n < 0 or n > GDIST_CLOSEST_MAX_N, NaN max_dist, GDIST_UPPER_TRIANGLE or
 * GDIST_OUT_DEVICE (not supported), SORTED on a bitsets-only collection. */
#define GDIST_CLOSEST_KEEP_SELF 0x1000u   /* a query in [c0, c1) may be its own neighbour */
#define GDIST_CLOSEST_MAX_N     512
int  gdist_closest(gdist_ctx* ctx, const gdist_sets* sets,
                   int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                   int method, unsigned flags, int n, double max_dist,
                   int64_t* idx_out, double* d_out, int32_t* count_out);
/* HIP-event time (ms, summed over the steps, on the context's stream) of the
 * last gdist_closest call made with option "time_kernels" = 1: the matrix
 * kernels (intersect or sketch) and the select kernel apart; -1 when the
 * call was not timed. */
int  gdist_ctx_closest_timing(gdist_ctx* ctx, double* matrix_ms, double* select_ms);

/* ---- in-group / out-group distance summary ----------------------------- */
/* The distCheck report (DistanceCheckProcessor.java:149-223) over the pairs
 * of a rectangle without the distance table leaving the device: for each of
 * ntypes groupings of the sets (labels[t * nsets + i] the group of set i
 * under grouping t, < 0: the set has none) the pairs (i, j), i in [r0, r1),
 * j in [c0, c1), are split as GroupTypeSpec.java:77-95 splits them. With
 * GDIST_UPPER_TRIANGLE only j > i counts; without it a diagonal pair inside
 * the rectangle counts like any other. A label < 0 on either set adds 1 to
 * bad[t] and nothing else (GroupTypeSpec.java:80-81); otherwise the pair
 * goes to out[2 t] (equal labels: in-group) or out[2 t + 1] (out-group).
 * d is the bit pattern gdist_intersect_matrix (kmer sets; method AUTO /
 * SORTED / BITSET resolved as gdist_closest resolves it) or
 * gdist_sketch_matrix (GDIST_SKETCH collections: method ignored) writes with
 * the same flags (GDIST_EMPTY_NAN, GDIST_SKETCH_JACCARD). Within a side
 * d == 1.0 adds to ones (GroupTypeSpec.java:84-87), NaN to nans, any other d
 * to n, min, max, sum and sumsq. Java's addValue(NaN) would poison the
 * statistics; this call counts NaNs apart instead.
 *
 * Every d < 1.0 the library produces is an integer multiple of 2^-53, so
 * sum and sumsq are exact integers of m = d * 2^53 and the result does not
 * depend on block sizes, method, run or rank: gdist_group_stats_merge adds
 * the results of disjoint rectangles (the ranks of a row-sharded run) to the
 * bytes one call over their union returns. mean and sdev (bias-corrected,
 * SummaryStatistics.getStandardDeviation) come from the exact sums, within
 * 1 / 2 ulp of the exact values; the reference's incremental update in file
 * order may differ from them in the last digits.
 *
 * The walk is gdist_closest's (options "closest_rows" / "closest_cols"). An
 * empty range: GDIST_OK, every side in its n == 0 form, bad 0. EINVAL (the
 * outputs stay untouched): a bad range, ntypes outside 1..GDIST_GROUP_MAX_TYPES,
 * a null pointer, GDIST_OUT_DEVICE, SORTED on a bitsets-only collection. */
#define GDIST_GROUP_MAX_TYPES 8
typedef struct {
    int64_t  n, ones, nans;     /* d < 1.0 values summarised; d == 1.0; NaN (GDIST_EMPTY_NAN only) */
    double   min, max;          /* over the n values; 1.0 / 1.0 when n == 0 */
    double   mean, sdev;        /* from the exact sums; 1.0 / 0.0 when n == 0; sdev 0.0 when n == 1 */
    uint64_t sum[2];            /* sum of m = d * 2^53, little-endian limbs */
    uint64_t sumsq[3];          /* sum of m * m */
} gdist_group_side;
int  gdist_group_stats(gdist_ctx* ctx, const gdist_sets* sets,
                       int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                       int method, unsigned flags, int ntypes,
                       const int32_t* labels /* [ntypes][nsets], host */,
                       gdist_group_side* out /* [ntypes][2]: in, out */, int64_t* bad /* [ntypes] */);
/* acc += part for every side and bad count (host only, exact): integer fields
 * limb-wise with carries, min / max over the sides holding values, mean and
 * sdev recomputed. EINVAL: a null pointer, ntypes outside 1..GDIST_GROUP_MAX_TYPES. */
int  gdist_group_stats_merge(gdist_group_side* acc, int64_t* bad_acc, const gdist_group_side* part,
                             const int64_t* bad_part, int ntypes);
/* HIP-event time (ms, summed over the steps) of the last gdist_group_stats
 * call made with option "time_kernels" = 1: the matrix kernels and the reduce
 * kernel apart; -1 when the call was not timed. */
int  gdist_ctx_group_stats_timing(gdist_ctx* ctx, double* matrix_ms, double* reduce_ms);

/* ---- sketch error at every sketch size --------------------------------- */
/* The per-size loop of WidthProcessor.ProcessGroup (WidthProcessor.java:
 * 153-208) as one walk of the pairs, with neither table leaving the device.
 * `sets` is the group's kmer collection and `sk` a GDIST_SKETCH collection
 * of the same context and the same number of sets, set i the bottom-W
 * signature of set i: what gdist_sketch_build(ctx, sets, W, ...) returns for
 * a W >= sizes[nsizes - 1]. The first s hashes of a bottom-W signature are
 * the bottom-s signature, so sk holds the sketches of every listed size.
 * Both collections are only read (a method may build its index on `sets`,
 * as in gdist_closest).
 *
 * For every pair i < j: r is the exact distance (the bit pattern
 * gdist_intersect_matrix writes; method AUTO / SORTED / BITSET resolved as
 * gdist_closest resolves it) and, per size s = sizes[k], s_k the sketch
 * distance gdist_sketch_matrix would write for the two size-s sketches under
 * the same flags (0, or GDIST_SKETCH_JACCARD). *pairs counts the pairs with
 * r < 1.0 (WidthProcessor.java:162). Row k describes size s over the pairs
 * with r != s_k (pairs with r == 1.0 included, WidthProcessor.java:186-192):
 * differing their number, max_err the largest e = |r - s_k| * 2.0 / (r + s_k)
 * (fp64, no contraction; 0.0 when none differ), sum the exact integer sum of
 * E = rint(e * 2^62) (ties to even; e <= 2, so E <= 2^63), total = sum *
 * 2^-62 (one rounding to nearest even, then an exact scale) and mean = total
 * / pairs. dwarves counts the sets whose signature in sk is shorter than s
 * (WidthProcessor.java:180). Every field is an integer result or comes from
 * one by a fixed expression, so the rows depend on neither the block sizes
 * (options "closest_rows" / "closest_cols": the walk is gdist_closest's),
 * the method nor the run. The reference adds the doubles e in i-major
 * order; `total` is the sum of the errors quantised to 2^-62 and may differ
 * from that sum in its last digits.
 *
 * nsets < 2 or nsizes == 0: GDIST_OK, *pairs = 0, every row's size and
 * dwarves set and its other fields zero. EINVAL, decided before any work
 * (the outputs stay untouched): a null handle, null pairs, null sizes or
 * rows_out with nsizes > 0, sets of another context, `sets` a sketch
 * collection or `sk` not one, differing set counts, nsizes outside
 * 0..GDIST_WIDTH_MAX_SIZES, sizes not strictly increasing or < 1, a last
 * size above the width of sk, any flag but GDIST_SKETCH_JACCARD
 * (GDIST_EMPTY_NAN too: a NaN has no place in an integer sum), an unknown
 * method, SORTED on a bitsets-only collection. */
#define GDIST_WIDTH_MAX_SIZES 512
typedef struct {
    int32_t  size, pad;              /* sizes[k]; 0 */
    int64_t  dwarves, differing;     /* signatures shorter than size; pairs with r != s_k */
    double   max_err, total, mean;   /* mean: total / pairs; 0.0 when pairs == 0 */
    uint64_t sum[2];                 /* sum of rint(e * 2^62), little-endian limbs */
} gdist_width_row;
int  gdist_width_sweep(gdist_ctx* ctx, const gdist_sets* sets, const gdist_sets* sk,
                       int nsizes, const int32_t* sizes /* host */, int method, unsigned flags,
                       gdist_width_row* rows_out /* [nsizes] */, int64_t* pairs);

/* ---- every pair within a distance -------------------------------------- */
/* The documented maxDist filter of the genomes table (GenomeProcessor.java:35,
 * "if a comparison results in a distance greater than this value, it will not
 * be output") as a CSR list, without the distance table leaving the device:
 * every pair (i, j), i in [r0, r1), j in [c0, c1), with d(i, j) <= max_dist.
 * The comparison is a plain fp64 <=: NaN (GDIST_EMPTY_NAN) never qualifies,
 * d == 1.0 does when max_dist >= 1.0, a negative max_dist gives nothing and
 * +inf everything but NaN. j == i is left out unless GDIST_CLOSEST_KEEP_SELF;
 * with GDIST_UPPER_TRIANGLE only j > i counts (supported here, unlike
 * gdist_closest: the fastaDist table is the upper triangle). d is the bit
 * pattern gdist_intersect_matrix (kmer sets: method AUTO / SORTED / BITSET
 * resolved as gdist_closest resolves it) or gdist_sketch_matrix (GDIST_SKETCH
 * collections: method ignored, GDIST_SKETCH_JACCARD honoured) writes with the
 * same flags.
 *
 * Order: row ascending, column ascending within a row; it depends on nothing
 * else (not the method, not "closest_rows", not the run). rowptr_out[a] is
 * the number of qualifying pairs in rows r0 .. r0 + a - 1, always complete
 * whatever capacity is, and *total = rowptr_out[r1 - r0]. col_out (global set
 * indices) and d_out receive the first min(*total, capacity) entries of that
 * order: a row may be cut in the middle, and nothing at or past capacity is
 * touched. capacity == 0 is the counting call: col_out and d_out may be NULL
 * and no survivor is written on the device either. A caller counts and calls
 * again, or guesses a capacity and calls again when *total > capacity.
 *
 * An empty row or column range: GDIST_OK, rowptr all zero, total 0. Disjoint
 * row ranges concatenate (shift the later rowptr by the earlier total), so
 * the ranks of a row-sharded run need no merge call. The walk is by row
 * blocks only (option "closest_rows", default by memory; "closest_cols" is
 * not read): per block the matrix kernels leave I or D on the device, a count
 * kernel, a scan and a write kernel compact it, and for kmer sets D is never
 * written. EINVAL, decided before any work (every output stays untouched): a
 * bad range, NaN max_dist, capacity < 0, null rowptr_out or total, null
 * col_out or d_out with capacity > 0, GDIST_OUT_DEVICE, an unknown method,
 * SORTED on a bitsets-only collection, 2^32 - 1 sets or more. After any other
 * failure the contents of col_out and d_out are unspecified. */
int  gdist_within(gdist_ctx* ctx, const gdist_sets* sets,
                  int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                  int method, unsigned flags, double max_dist, int64_t capacity,
                  int64_t* rowptr_out /* r1 - r0 + 1 */, int64_t* col_out, double* d_out,
                  int64_t* total);
/* HIP-event time (ms, summed over the steps) of the last gdist_within call
 * made with option "time_kernels" = 1: the matrix kernels and the count, scan
 * and write kernels apart; -1 when the call was not timed. */
int  gdist_ctx_within_timing(gdist_ctx* ctx, double* matrix_ms, double* select_ms);

/* ---- distances of a pair list ------------------------------------------ */
/* getDistance over a pair list (MethodTableProcessor.java:258-276): for p in [0, npairs)
 * I_out[p] = |A_rows[p] ∩ A_cols[p]|, D_out[p] = the distance, host arrays, either may be NULL.
 *
 * The list may come in any order, may repeat a pair and may hold i == j:
 * output slot p depends on (rows[p], cols[p]) only, not on the order, the rest
 * of the list, the method or the run. D_out[p] is bit for bit the D that
 * gdist_intersect_matrix writes for that cell with the same flags
 * (GDIST_EMPTY_NAN is honoured) and I_out[p] its I; for i == j that is |A_i|
 * (not the popcount of the pruned bitsets) and d = 0.0, or the empty-set value.
 * method AUTO / SORTED / BITSET is resolved as gdist_closest resolves it, for
 * npairs pairs; a collection whose codes were released answers BITSET and AUTO.
 *
 * The list is uploaded once, sorted by row on the device and cut into work
 * units there (a row, at most 64 of its pairs, a range of the sorted join's
 * segment index: a few pairs of huge sets are cut into many units whose
 * integer counts are added, which is exact); the outputs come back in one
 * download. npairs == 0: GDIST_OK, nothing is touched. EINVAL, decided before
 * any work (the outputs stay untouched): npairs < 0 or >= 2^31, null rows or
 * cols or both outputs null with npairs > 0, an index outside [0, nsets), a
 * GDIST_SKETCH collection, GDIST_UPPER_TRIANGLE or GDIST_OUT_DEVICE, an
 * unknown method, SORTED on a bitsets-only collection. */
int  gdist_pairs(gdist_ctx* ctx, const gdist_sets* sets, int64_t npairs,
                 const int64_t* rows, const int64_t* cols, int method, unsigned flags,
                 int32_t* I_out, double* D_out);
/* last gdist_pairs, gdist_cross_pairs or gdist_sketch_pairs call: kernel time (ms; -1 unless option "time_kernels" = 1), the
 * distinct-row groups of the list and the work units launched for them */
int  gdist_ctx_pairs_info(gdist_ctx* ctx, double* kernel_ms, int64_t* groups, int64_t* units);

/* ---- new query sets against a resident collection ---------------------- */
/* The reference loads its genome database once and answers one
 * getClosest(kmers, n, maxDist) per incoming genome (FindProcessor.java:94-110,
 * MashProcessor.java:150). `subjects` is that database: a collection of kmer
 * sets (or of sketches, below) that stays as it is. `queries` is another collection of the same context and
 * kmer spec (what gdist_sets_concat would accept; GDIST_NO_CASE_FOLD may
 * differ). Rows are query sets [q0, q1), columns subject sets [c0, c1).
 *
 * gdist_cross_matrix: I_out[(i-q0)*ld + (j-c0)] = |Q_i ∩ S_j| and D_out
 * likewise the distance (host arrays, either may be NULL), the header's Java
 * expression with |A| from the queries' sizes and |B| from the subjects';
 * GDIST_EMPTY_NAN is honoured. Bit for bit what
 * gdist_intersect_matrix(GDIST_METHOD_SORTED) writes for rows
 * [ns+q0, ns+q1) x cols [c0, c1) of gdist_sets_concat(subjects, queries),
 * ns = the subjects' sets. Cells outside the rectangle, the ld padding
 * included, are not touched. The rectangle is walked in row blocks x column
 * chunks sized like gdist_closest's (device scratch is bounded).
 *
 * gdist_cross_closest: for every query row the subjects j in [c0, c1) with
 * d <= max_dist, ordered by (d as fp64, j), the first n. Output layout, fill
 * values (-1 / 1.0) and the NaN / d == 1.0 rules are gdist_closest's. No
 * column is left out as "self": the collections are different, and the same
 * handle passed for both behaves as GDIST_CLOSEST_KEEP_SELF. The counts stay
 * on the device and D is never written; the walk takes the options
 * "closest_rows" / "closest_cols".
 *
 * Both run the sorted join over work units (query row, <= 64 consecutive
 * subject columns, a range of the subjects' segment index), so one query
 * against many subjects still fills the device (the pruned dictionary of the
 * subjects cannot answer for kmers that only a query and one subject share).
 *
 * Sketches. Every cross call also takes two GDIST_SKETCH collections of one
 * context, width and kmer spec (what gdist_sets_concat accepts): the
 * reference's MinHash database and the sketches of incoming genomes. One
 * sketch collection and one of kmer sets is EINVAL. For a sketch pair
 *  - flags may hold GDIST_SKETCH_JACCARD beside GDIST_EMPTY_NAN, with the
 *    meaning they have in gdist_sketch_matrix;
 *  - gdist_cross_matrix's I_out is the common count (gdist_sketch_matrix's
 *    common_out) and D_out the sketch distance;
 *  - each call returns, bit for bit, what its twin (gdist_sketch_matrix,
 *    gdist_closest, gdist_within, gdist_group_stats, gdist_histogram) returns
 *    on gdist_sets_concat(subjects, queries) for rows [ns+q0, ns+q1) x cols
 *    [c0, c1) with the same flags (plus GDIST_CLOSEST_KEEP_SELF for closest
 *    and within) and the labels slabels[t] followed by qlabels[t]; every other
 *    rule below carries over;
 *  - a wave merges a (query, subject) pair in 64 segments, a workgroup holds
 *    a run of subjects on chip for every query row of the step: one query
 *    against a million subjects fills the device, the subjects are read once
 *    a step and never copied. Nothing is built or kept on either collection
 *    (there is no segment index here); both need their signatures.
 * The exact list this gives is the yardstick of gdist_lsh_closest, which looks
 * at the LSH buckets only.
 *
 * The subjects are read only: bitsets, tiers, launch plans, captured graphs,
 * codes and the number of sets are as before the call. The one thing a cross
 * call adds, when absent, is the subjects' segment index of the sorted join,
 * exactly as a GDIST_METHOD_SORTED call on them does; like after such a call,
 * a later GDIST_METHOD_AUTO on subjects without bitsets stays on the sorted
 * join instead of trying the dictionary build. Nothing is kept on the queries.
 *
 * An empty row or column range: GDIST_OK; the matrix outputs are untouched,
 * the closest counts are 0 with slots -1 / 1.0 (n == 0 likewise). EINVAL,
 * decided before any work with every output untouched: a null handle,
 * collections of another context or of different contexts, one GDIST_SKETCH
 * collection with one of kmer sets, kmer specs (or sketch widths)
 * gdist_sets_concat would refuse, a collection without
 * codes (released, or from gdist_sets_allgather_bitsets), a range outside its
 * collection, ld < c1 - c0, both matrix outputs NULL on a non-empty
 * rectangle, any flag but GDIST_EMPTY_NAN (sketches: and
 * GDIST_SKETCH_JACCARD), n < 0 or n > GDIST_CLOSEST_MAX_N,
 * NaN max_dist, NULL closest outputs with a non-empty row range, subjects of
 * 2^32 - 1 sets or more. */
int  gdist_cross_matrix(gdist_ctx* ctx, const gdist_sets* queries, const gdist_sets* subjects,
                        int64_t q0, int64_t q1, int64_t c0, int64_t c1, unsigned flags,
                        int32_t* I_out, double* D_out, int64_t ld);
int  gdist_cross_closest(gdist_ctx* ctx, const gdist_sets* queries, const gdist_sets* subjects,
                         int64_t q0, int64_t q1, int64_t c0, int64_t c1, unsigned flags,
                         int n, double max_dist,
                         int64_t* idx_out, double* d_out, int32_t* count_out);

/* gdist_cross_pairs: getDistance over a pair list (MethodTableProcessor.java:258-276;
 * the lists BasicPairsProcessor.java:71-89 and PairCreateProcessor.java:29-32
 * write) whose rows index `queries` and whose columns index `subjects`: a
 * handful of cells of the rectangle, without the rectangle. For p in
 * [0, npairs) I_out[p] and D_out[p] (host arrays, either may be NULL) are bit
 * for bit what gdist_cross_matrix(ctx, queries, subjects, ...) writes for cell
 * (rows[p], cols[p]) with the same flags, which is what
 * gdist_pairs(GDIST_METHOD_SORTED) gives on gdist_sets_concat(subjects, queries)
 * for the pair (ns + rows[p], cols[p]), ns = the subjects' sets.
 *
 * Slot p depends on (rows[p], cols[p], flags) only: not on the order of the
 * list, its repeats, the rest of the list or the run. No pair is "self": with
 * the same handle passed for both collections i == j gives I = |A_i| and
 * d = 0.0 (or the empty-set value of an empty set) by the join itself.
 * GDIST_EMPTY_NAN is the only flag for kmer sets. There is no `method`, as in
 * the other cross calls: the subjects' pruned dictionary cannot answer for
 * kmers that only one query and one subject share.
 *
 * The list is uploaded once and sorted by query row on the device; a row's
 * pairs are cut into work units of at most 64 pairs and, past the call's code
 * budget (the query's size plus its listed subjects' sizes), a range of the
 * subjects' segment index. Where a query is cut by the subjects' splitters is
 * found per unit and cached nowhere; a unit's integer counts are added, which
 * is exact. The outputs come back in one download.
 *
 * The subjects are read only, under the rule above: the one thing the call may
 * add is their segment index. Nothing is kept on the queries.
 * gdist_ctx_pairs_info reports this call (groups = the distinct rows of the
 * list, units = the work units launched, as for gdist_pairs; kernel ms under
 * option "time_kernels"); gdist_ctx_cross_info is left as it was.
 *
 * Two GDIST_SKETCH collections are answered by the code behind
 * gdist_sketch_pairs(ctx, queries, subjects, ...), bit for bit, and flags may
 * then hold GDIST_SKETCH_JACCARD beside GDIST_EMPTY_NAN.
 *
 * npairs == 0: GDIST_OK, nothing is touched. EINVAL, decided before any work
 * with every output untouched: what gdist_cross_matrix refuses of the handles
 * (null, another context or different contexts, one GDIST_SKETCH collection
 * with one of kmer sets, kmer specs gdist_sets_concat would refuse, a
 * collection without codes), npairs < 0 or >= 2^31, null rows or cols or both
 * outputs null with npairs > 0, any flag but the ones above, a rows[p] outside
 * [0, nsets of queries), a cols[p] outside [0, nsets of subjects). */
int  gdist_cross_pairs(gdist_ctx* ctx, const gdist_sets* queries, const gdist_sets* subjects,
                       int64_t npairs, const int64_t* rows /* into queries */,
                       const int64_t* cols /* into subjects */, unsigned flags,
                       int32_t* I_out, double* D_out);

/* gdist_cross_within, gdist_cross_group_stats, gdist_cross_histogram: the
 * three table-free queries of one collection (gdist_within,
 * gdist_group_stats, gdist_histogram) over the same rectangle of query rows
 * [q0, q1) x subject columns [c0, c1), by the same join and under the same
 * read-only rule for the subjects as the two calls above. Each takes its
 * twin's arguments with `sets` replaced by `queries, subjects` and without
 * `method`; column indices in the outputs (col_out) are subject indices. The
 * only flag is GDIST_EMPTY_NAN (a sketch pair: and GDIST_SKETCH_JACCARD): no column is "self" and there is no
 * GDIST_UPPER_TRIANGLE, so every cell of the rectangle counts, and the same
 * handle passed for both collections behaves as GDIST_CLOSEST_KEEP_SELF
 * without GDIST_UPPER_TRIANGLE. Labels come per side: qlabels[t * nq + i] the
 * group of query set i and slabels[t * ns + j] of subject set j under
 * grouping t (nq, ns = all sets of the collections, whatever the ranges).
 *
 * Each call returns, bit for bit (rowptr, col, the d patterns, every field of
 * gdist_group_side, counts, nans, bad), what its twin returns on
 * C = gdist_sets_concat(subjects, queries) with GDIST_METHOD_SORTED for rows
 * [ns+q0, ns+q1) x cols [c0, c1), the same flags (plus
 * GDIST_CLOSEST_KEEP_SELF for within) and, for grouping t, the labels
 * slabels[t] followed by qlabels[t]. Every other rule of the twins carries
 * over: capacity may cut a row, capacity == 0 is the counting call and nothing
 * at or past capacity is touched; disjoint row ranges of within concatenate;
 * the group sums are exact limbs and merge through gdist_group_stats_merge;
 * buckets are found by fp64 comparison only and the results of disjoint
 * rectangles add element-wise.
 *
 * Walks. Group stats and histogram fold every (row block x column chunk) step
 * into their accumulators (options "closest_rows" / "closest_cols"). Within
 * needs a row's full width before it can compact in (row, column) order: row
 * blocks sized as gdist_within sizes them ("closest_rows"; "closest_cols" is
 * not read) over all of [c0, c1). No result depends on either option.
 *
 * An empty row or column range: GDIST_OK in the twin's empty form (rowptr all
 * zero and total 0; every side in its n == 0 form and bad 0; every count
 * zero). EINVAL, decided before any work with every output untouched: what
 * gdist_cross_matrix refuses of the handles, ranges and flags, and each twin's
 * own conditions: NaN max_dist, capacity < 0, null rowptr_out or total, null
 * col_out or d_out with capacity > 0; ntypes outside 1..GDIST_GROUP_MAX_TYPES,
 * null labels, out or bad; nedges outside 1..GDIST_HIST_MAX_EDGES, a NaN edge,
 * edges not strictly ascending, ntypes outside 0..GDIST_GROUP_MAX_TYPES, null
 * edges, counts_out or nans_out, null qlabels, slabels or bad_out with
 * ntypes > 0. */
int  gdist_cross_within(gdist_ctx* ctx, const gdist_sets* queries, const gdist_sets* subjects,
                        int64_t q0, int64_t q1, int64_t c0, int64_t c1, unsigned flags,
                        double max_dist, int64_t capacity,
                        int64_t* rowptr_out /* q1 - q0 + 1 */, int64_t* col_out, double* d_out,
                        int64_t* total);
int  gdist_cross_group_stats(gdist_ctx* ctx, const gdist_sets* queries, const gdist_sets* subjects,
                             int64_t q0, int64_t q1, int64_t c0, int64_t c1, unsigned flags, int ntypes,
                             const int32_t* qlabels /* [ntypes][nq], host */,
                             const int32_t* slabels /* [ntypes][ns], host */,
                             gdist_group_side* out /* [ntypes][2]: in, out */, int64_t* bad /* [ntypes] */);
int  gdist_cross_histogram(gdist_ctx* ctx, const gdist_sets* queries, const gdist_sets* subjects,
                           int64_t q0, int64_t q1, int64_t c0, int64_t c1, unsigned flags,
                           int nedges, const double* edges /* host, strictly ascending */,
                           int ntypes, const int32_t* qlabels, const int32_t* slabels /* NULL when ntypes == 0 */,
                           int64_t* counts_out /* [S][nedges + 1] */, int64_t* nans_out /* [S] */,
                           int64_t* bad_out /* [ntypes]; may be NULL when ntypes == 0 */);
/* last cross call: HIP-event time (ms, summed over the steps; -1 unless option
 * "time_kernels" = 1) of the join kernel and of the kernels that follow it
 * (gdist_cross_closest: the select; gdist_cross_matrix: the distance
 * epilogue, 0 without D_out; gdist_cross_within: count, scan and write;
 * gdist_cross_group_stats: the reduce; gdist_cross_histogram: the histogram
 * kernel), and the work units launched. A sketch pair: join_ms is the merge
 * kernel, select_ms the same consumers (0 for gdist_cross_matrix: D comes from
 * the merge itself), units the (query, subject) pairs merged,
 * (q1 - q0) (c1 - c0) */
int  gdist_ctx_cross_info(gdist_ctx* ctx, double* join_ms, double* select_ms, int64_t* units);

/* ---- distribution of the distances ------------------------------------- */
/* How the distances of a rectangle are distributed over caller-supplied
 * bucket edges, without the distance table leaving the device: the bucket
 * report of the taxonomy check (TaxCheckProcessor.java:93 sets up 50 buckets
 * over [0, 1], TaxCheckProcessor.java:133-135 feeds every series into them),
 * and what a max_dist for gdist_within, gdist_closest or gdist_greedy_reps is
 * chosen from. A histogram also answers the hand-rolled counts of the
 * reference (pairs with d < 1.0, WidthProcessor.java:162; close pairs below a
 * target, TuningProcessor.java:131-133) and any multi-threshold count.
 *
 * Pairs are those of gdist_group_stats: (i, j), i in [r0, r1), j in [c0, c1);
 * with GDIST_UPPER_TRIANGLE only j > i counts, without it a diagonal pair
 * inside the rectangle counts like any other. d is the bit pattern
 * gdist_intersect_matrix (kmer sets; method AUTO / SORTED / BITSET resolved
 * as gdist_closest resolves it) or gdist_sketch_matrix (GDIST_SKETCH
 * collections: method ignored) writes with the same flags (GDIST_EMPTY_NAN,
 * GDIST_SKETCH_JACCARD).
 *
 * Series. ntypes == 0: one series (S = 1) of every pair; labels and bad_out
 * may be NULL. ntypes in 1..GDIST_GROUP_MAX_TYPES: S = 2 ntypes, series 2 t
 * the in-group and 2 t + 1 the out-group pairs of grouping t, split as
 * gdist_group_stats splits them (GroupTypeSpec.java:77-95): a label < 0 on
 * either set adds 1 to bad_out[t] and nothing else.
 *
 * Buckets. With edges e_0 < ... < e_{E-1} (host, strictly ascending; -inf and
 * +inf allowed) a non-NaN d goes to bucket b = the number of edges <= d
 * (numpy.searchsorted(edges, d, side="right")): bucket 0 is d < e_0, bucket b
 * is e_{b-1} <= d < e_b, bucket E is d >= e_{E-1}. The bucket is found by
 * fp64 comparisons against the edges alone, so edges one ulp apart and
 * denormal edges are exact. d == 1.0 is bucketed like any other value: an
 * edge at 1.0 separates the "ones". NaN goes to nans_out[s] and to no bucket,
 * so for every series sum_b counts + nans is its number of pairs (with
 * ntypes >= 1: n + ones + nans of the matching gdist_group_side).
 * counts_out[s * (E + 1) + b], nans_out[s]. The reference's buckets are the
 * edges i / 50, i = 0..50.
 *
 * Every output is an integer count decided by fp64 comparisons, so the result
 * does not depend on block sizes, method, pair order, run or rank, and the
 * results of disjoint rectangles with the same edges and labels add
 * element-wise (no merge call). The walk is gdist_group_stats's (options
 * "closest_rows" / "closest_cols"). An empty row or column range: GDIST_OK,
 * every output zero. EINVAL, decided before any work (the outputs stay
 * untouched): a bad range, nedges outside 1..GDIST_HIST_MAX_EDGES, a NaN
 * edge, edges not strictly ascending (-0.0 next to 0.0 is not), ntypes
 * outside 0..GDIST_GROUP_MAX_TYPES, null edges, counts_out or nans_out, null
 * labels or bad_out with ntypes > 0, GDIST_OUT_DEVICE, an unknown method,
 * SORTED on a bitsets-only collection. */
#define GDIST_HIST_MAX_EDGES 1023          /* at most 1024 buckets */
int  gdist_histogram(gdist_ctx* ctx, const gdist_sets* sets,
                     int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                     int method, unsigned flags,
                     int nedges, const double* edges /* host, strictly ascending */,
                     int ntypes, const int32_t* labels /* [ntypes][nsets], host; NULL when ntypes == 0 */,
                     int64_t* counts_out /* [S][nedges + 1] */, int64_t* nans_out /* [S] */,
                     int64_t* bad_out /* [ntypes]; may be NULL when ntypes == 0 */);
/* HIP-event time (ms, summed over the steps) of the last gdist_histogram call
 * made with option "time_kernels" = 1: the matrix kernels and the histogram
 * kernel apart; -1 when the call was not timed. */
int  gdist_ctx_histogram_timing(gdist_ctx* ctx, double* matrix_ms, double* reduce_ms);

/* ---- multi-GPU (RCCL over xGMI) -------------------------------------- */
#define GDIST_UNIQUE_ID_BYTES 128
int  gdist_comm_unique_id(char id[GDIST_UNIQUE_ID_BYTES]);
int  gdist_comm_init(gdist_ctx* ctx, const char id[GDIST_UNIQUE_ID_BYTES], int nranks, int rank);
/* Host-staged communicator: every collective of the library becomes one
 * all-gather of host buffers through `fn`, which must place the `bytes` of
 * every rank, in rank order, into recv (nranks * bytes) and return 0. For
 * ranks that share one GPU (rehearsing the multi-rank path; RCCL refuses two
 * ranks on one device) or hosts without RCCL peer access; RCCL
 * (gdist_comm_init) is the transport of a multi-GPU node. */
typedef int (*gdist_allgather_fn)(const void* send, void* recv, int64_t bytes, void* user);
int  gdist_comm_init_host(gdist_ctx* ctx, int nranks, int rank, gdist_allgather_fn fn, void* user);
int  gdist_comm_destroy(gdist_ctx* ctx);
/* Every rank passes its local shard; every rank receives the concatenation
 * in rank order (one all-gather of offsets and one, in place, of codes). */
int  gdist_sets_allgather(gdist_ctx* ctx, const gdist_sets* local, gdist_sets** out);
/* The same; with GDIST_ALLGATHER_CONSUME the library releases `local`'s
 * device data once its codes are in the gather buffer (local keeps its sizes
 * and can still be freed; it can no longer be used for distances). Peak
 * device bytes per rank: (ranks + 1) x the largest shard's codes. The local
 * data is released BEFORE the collective runs: if the all-gather itself
 * fails (GDIST_ECOMM, or the host transport's callback), `local` stays
 * unusable and no result is returned; the caller re-packs its shard. */
#define GDIST_ALLGATHER_CONSUME 0x1u
int  gdist_sets_allgather_ex(gdist_ctx* ctx, gdist_sets* local, unsigned flags, gdist_sets** out);
/* Which exchange a row-sharded N×N over this communicator should use
 * (collective: every rank calls it with its local shard and gets the same
 * answer). *chosen = GDIST_METHOD_BITSET: the dictionary exchange
 * (gdist_sets_allgather_bitsets); GDIST_METHOD_SORTED: the code all-gather
 * (gdist_sets_allgather_ex) for the sorted join. METHOD_AUTO takes the
 * dictionary exchange when its per-rank estimate fits the budget (option
 * "exchange_budget", default 0.8 x the device memory), else the codes; the
 * estimates (bytes per rank; the codes' assume the shard is consumed) are
 * returned. ENOMEM when neither fits.
 * (C4 = 100,000 x 100 kbp on 8 GPUs takes the codes.) */
int  gdist_sets_exchange_plan(gdist_ctx* ctx, const gdist_sets* local, int method, int* chosen,
                              double* bytes_bitsets, double* bytes_codes);
/* Dictionary-rank bitsets of the concatenation (in rank order) of every
 * rank's local sets: one all-gather of the local dictionary summaries
 * (distinct codes + counts), one of the local bitsets. The result holds the
 * bitsets and sizes of all sets but no codes: use it with
 * GDIST_METHOD_BITSET (or AUTO). Memory per rank ~ N * W words instead of
 * every rank's codes. */
int  gdist_sets_allgather_bitsets(gdist_ctx* ctx, const gdist_sets* local, unsigned flags, gdist_sets** out);
/* Scalar max-reduction and barrier over the communicator (timing only). */
int  gdist_comm_allreduce_max(gdist_ctx* ctx, double* value);

/* The cost model's estimate (seconds) of one intersect-matrix call on the
 * block rows [r0, r1) x columns [c0, c1) (upper: pairs j > i only): with
 * bitsets built, dense tiles + the rare kernel the call would pick
 * (*rare_kernel = 0 list-major, 1 row-major, -1 no rare tier); otherwise the
 * sorted join (*rare_kernel = -1). For row partitions that balance modelled
 * time rather than area (gdist.shard.balanced_bounds). */
int  gdist_sets_block_cost(const gdist_sets* sets, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int upper,
                           double* seconds, int* rare_kernel);

/* Row partition with equal upper-triangle area:
 * r_g = N (1 - sqrt(1 - g/G)), rounded to multiples of `align`. */
int  gdist_triangle_partition(int64_t n, int nparts, int64_t align, int64_t* bounds /* nparts+1 */);

#ifdef __cplusplus
}
#endif
#endif /* GDIST_H */
