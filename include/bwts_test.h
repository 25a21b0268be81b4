/*
 * bwts_test.h -- harness and unit-test entry points of libbwts_hip.so.
 *
 * Not part of the drop-in surface (include/bwts.h is): these exist for tests/, bench.py and tools/ --
 * synthetic inputs generated in device memory, raw device buffers without a tensor library, and hooks that
 * run single stages of the engine.  The reference (NealB/Bijective-BWT) has no counterpart.
 */
#ifndef BWTS_TEST_H
#define BWTS_TEST_H

#include "bwts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Harness utilities (bench / tests): synthetic inputs of SURVEY.md 8(d) written
 * straight into device memory (kind 0 uniform256, 1 zipf, 2 dna, 3 text: zipf stream with back-references), device
 * buffers without a tensor library, and a 64-bit FNV-style checksum. */
int bwts_generate_device(bwts_ctx *ctx, int kind, uint64_t seed, uint64_t n, void *d_out);
int bwts_device_alloc(bwts_ctx *ctx, uint64_t bytes, void **d_ptr);
int bwts_device_free(bwts_ctx *ctx, void *d_ptr);
int bwts_copy_to_device(bwts_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes);
int bwts_copy_to_host(bwts_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes);
int bwts_device_equal(bwts_ctx *ctx, const void *d_a, const void *d_b, uint64_t bytes, int *equal);

/* Unit-test hooks for single kernels (stable LSD radix sort of (u64 key, u32
 * value) pairs on the low key_bits bits; suffix array via the non-cyclic sort). */
int bwts_debug_sort_pairs(bwts_ctx *ctx, uint64_t *h_keys, uint32_t *h_vals, uint64_t m, int key_bits);
int bwts_debug_suffix_array(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint32_t *h_sa);
/* The ranking of one tile of the packed round-0 radix passes alone, in one workgroup of 8 waves: 8192 digits and 8192 validity bytes
 * (0: the item does not exist) in host memory, item j (0 .. 15) of lane l of wave w at [(w * 16 + j) * 64 + l].  A wave ranks its
 * items in the order of j on one set of counters, the first atomic_items (even, 0 .. 16) of them with one returning LDS add each,
 * the others by ballots.  ranks: every valid item's number of earlier (item, lane) pairs of its wave with its digit, ~0 for an
 * invalid item.  shipped: the atomic_items of the first, middle, classic last and lean last pass as built.  BWTS_E_ARG for a NULL
 * pointer or an atomic_items outside that set. */
int bwts_debug_rank_steps(bwts_ctx *ctx, const uint8_t *digits, const uint8_t *valid, int atomic_items, uint32_t *ranks, uint32_t shipped[4]);
int bwts_debug_lyndon(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint64_t *h_starts, uint64_t cap, uint64_t *count);
/* Pure arithmetic, no context and no device: the chunk tables of the forward's later rounds for a tied list of a0 elements, and the
 * re-cut of the a_chunks <= a0 elements left at a compaction.  out = {nominal chunk size of a0, table capacity = a0 / 2048 + 128,
 * nominal size of a_chunks, chunks of the re-cut}; returns 1 when the re-cut fits the tables, which it always does (the capacity
 * holds every run the driver can make: csrc/chunk_rounds.h, chunk_table_capacity), else 0.
 * _target: the same with cuts that aim at `target` chunks (16 .. 16384; the engine's own 16384 unless the test switch
 * BWTS_CHUNK_TARGET is set); -1 on a target outside that range.  bwts_debug_chunk_plan is the call with 16384. */
int bwts_debug_chunk_plan(uint64_t a0, uint64_t a_chunks, uint64_t out[4]);
int bwts_debug_chunk_plan_target(uint64_t a0, uint64_t a_chunks, uint32_t target, uint64_t out[4]);
/* Pure arithmetic, no context and no device: the round-0 key layout a sort picks for a text of n >= 1 bytes with this byte histogram
 * (csrc/key_plan.h, the single statement of the rules).  reserve_pad: 0 the cyclic sort, 1 the suffix form (code 0 is "past the end").
 * key_symbols, varlen, key_bits: the knobs BWTS_KEY_SYMBOLS, BWTS_VARLEN and BWTS_KEY_BITS as numbers, BWTS_KEY_KNOB_ABSENT for one
 * that is not set (key_symbols and key_bits: atoi of the text; varlen: 0 never, 1 always, any other value: set and neither).  kb_emp
 * and partners_of (65 doubles, < 0 where the sample has no say; may be NULL): what the key sample of a cyclic sort of n >= 2^22
 * found, kb_emp = 0 for no sample.  Without a sample the answer is the engine's for n < 2^22 (and for every suffix sort); from 2^22 on
 * the engine may widen the key by its sample.
 * out: 0 sigma; 1 bits per fixed-width code; 2 pad_add; 3 msym; 4 key_bits; 5 varlen; 6 hstep; 7 patch_span; 8 few_ties; 9 lmax, the
 * longest word of the alphabetic code (0: none was built; 99: built and refused); 10 the model's own key width (iid_key_bits; 0
 * without a code); 11, 12 radix passes of the fixed-width and of the variable-length alternative (12 is 0 where there is none);
 * 13 the mean code length in bits per symbol, a double's bit pattern; 14 an alphabetic code was built and accepted; 15 the
 * variable-length alternative's key width after sample and knob.  codes: byte -> fixed-width code.  vtab: (length << 32) | code of
 * each byte value's word, all 0 when word 14 is 0.
 * Returns 0; -1 on a NULL pointer (partners_of excepted), n = 0, or a histogram that does not sum to n. */
#define BWTS_KEY_PLAN_WORDS 16
#define BWTS_KEY_KNOB_ABSENT (-2147483647 - 1)
int bwts_debug_key_plan(const uint64_t hist[256], uint64_t n, int reserve_pad, int key_symbols, int varlen, int key_bits, int kb_emp,
                        const double *partners_of, uint64_t out[BWTS_KEY_PLAN_WORDS], uint8_t codes[256], uint64_t vtab[256]);
/* Pure arithmetic, no context and no device: how the move-to-front stage (bwts_mtf.h) cuts one input of n >= 1 bytes.  out = {T, the
 * tile size in bytes; G, the tiles one wave composes in the scan's first level; tiles = ceil(n / T); groups = ceil(tiles / G)}.
 * Returns 0, -1 on a bad argument. */
int bwts_debug_mtf_plan(uint64_t n, uint64_t out[4]);
/* Device time in ms of every timed launch of the most recent call on the context, in launch order, into ms[0 .. cap): with
 * bwts_set_timing level 2 every launch is timed, so this is the per-kernel split that bwts_timings sums by class.  Returns the
 * number written (0 with timing off), < 0 on a bad argument. */
int bwts_debug_last_spans(bwts_ctx *ctx, double *ms, uint64_t cap);
/* Pure arithmetic, no context and no device: the arena of the inverse for n <= 2^32 elements.  out[0] = bytes one attempt with
 * splitter spacing 2^g (g < 0: the spacing the engine picks for n) and mark 0 index log, 1 sentinel, 2 byte map, 3 moments (the
 * default) reserves; out[1] = bytes the host path allocates before the transform runs.  Returns the g used, -1 on a bad argument. */
int bwts_debug_inverse_arena(uint64_t n, int g, int mark, uint64_t out[2]);
/* Likewise for the narrow forward (1 <= n <= 2^32): out[0] = bytes of the arena a call declares and the host path allocates ahead.
 * Returns 0, -1 on a bad argument. */
int bwts_debug_forward_arena(uint64_t n, uint64_t out[1]);
/* Likewise for one run of the forward beyond 2^32 (1 <= n <= 2^36; the forced runs of the tests take it below 2^32 too): out[0] =
 * bytes of the arena a run in mode 0 direct (no rank array), 1 ranks, 2 suffix (the route to the Lyndon factors) declares, with
 * segments of 2^seg_log2 positions (11..31) and buckets of bucket_cap elements (256..0xff000000); 0 for either means the engine's own
 * choice for n.  Returns 0, -1 on a bad argument. */
int bwts_debug_wide_forward_arena(uint64_t n, int mode, int seg_log2, uint64_t bucket_cap, uint64_t out[1]);
/* What the most recent inverse call on the context did, one record of 16 words per attempt of its fallback chain, oldest first
 * (no device work: the engine keeps the records on the host as it goes).  Word 0 g: log2 of the splitter spacing; 1 mark: 0 index
 * log, 1 sentinel, 2 byte map, 3 moments; 2 outcome: 0 done, 1 retry with every element a splitter (node pool overflow, or the unit
 * nodes refused), 2 ambiguous sentinel (n = 2^32), 3 the moments do not name the unreached elements (next: the index log; wide form:
 * the marks), 255 the attempt ended with an error code; 3 s: splitters; 4 virtual nodes handed out by the walk (s_all - s; counted
 * past the pool's end when it overflows); 5 node_cap; 6 nu: elements no walk reached; 7 nu2: nodes no level-2 walk reached;
 * 8 room for unreached elements at the first collection; 9 a second collection ran; 10 moments: classes listed for the search, as
 * read back after the first collection; 11 moments: the fallback flag, likewise; 12 the unit-node route ranked the cycles without a
 * splitter; 13 kc: cycles of the node list; 14 kt: cycles without a splitter; 15 form: 0 narrow, 1 wide, 2 wide compact, 3 narrow,
 * segmented (the shared pass of bwts_inverse_segments over a run of segments: after such a call the records are those of the last
 * pass that ran).  A stage
 * that did not run leaves its words 0; the wide form has no level 2 (word 7 stays 0).
 * out receives whole records while they fit into cap_words; *attempts = attempts the call made (records exist for the first 8; 0
 * after the constant-input shortcut beyond 2^31, and before any call).  Returns the number of records written, < 0 on a bad argument. */
int bwts_debug_inverse_report(bwts_ctx *ctx, uint64_t *out, uint64_t cap_words, uint64_t *attempts);
/* Pure arithmetic, no context and no device (so no test switch applies): what bwts_inverse_segments would do with `count` segments of
 * these lengths.  out: 0 plan: 0 = A, segments below `big` are walked one lane each in one pass; 1 = B, every maximal run of consecutive
 * segments below `big` goes through one shared pass of the splitter walk; 1 big: segments of this length or more take a single-input
 * call each (2^64 - 1: none); 2 runs: shared passes (plan A: 1 when a segment is walked, else 0); 3, 4 segments and bytes on the plan's
 * own route (lane walk or shared pass); 5, 6 segments and bytes that go single; 7 arena bytes the call reserves for its own route.
 * Returns the plan, -1 on a bad argument (no lengths, a zero length, a sum beyond 2^32). */
int bwts_debug_segments_plan(const uint64_t *lengths, uint64_t count, uint64_t out[8]);
/* What the most recent segmented inverse (host or device entry) on the context did (host memory, no device work).  Words as for
 * bwts_debug_segments_plan with the test switches applied, except: 0 plan: also 2 = B was chosen, its arena was refused
 * (BWTS_E_NOMEM) and plan A ran instead; 7 the largest attempt count of the call's passes and single calls.  A call with one segment
 * is a single call (words 5 and 6).  All 0 before any call. */
int bwts_debug_segments_report(bwts_ctx *ctx, uint64_t out[8]);
/* What the doubling sorts of the most recent forward call on the context did (also bwts_debug_suffix_array and bwts_debug_lyndon;
 * no device work: the engine keeps the records on the host as it goes, from values its stages read back anyway).  One record of
 * BWTS_FWD_SORT_WORDS words per sort, in the order they ran: a forward that found its factors by the general Lyndon path has the
 * suffix sort first, then the cyclic sort.  Nothing is recorded by the paths beyond 2^32 positions, the one-symbol shortcut, or a
 * segmented call's shared pass before its last sort.
 * Header, words 0..47: 0 cyclic (1) or suffix form (0); 1 n; 2 factors k (0: suffix form); 3 sigma; 4 bits per symbol; 5 msym;
 * 6 key_bits; 7 varlen; 8 hstep; 9 keys: 0 one u64 each, 1 split without the high byte, 2 split with it; 10 flags_outside_rank;
 * 11 tied after round 0; 12 rank_early; 13 form of the later rounds: 0 none, 1 sparse, 2 chunks, 3 tiles, 4 direct (every tied group
 * ordered by comparing its members' rotations: one round, no rank of any other position); 14 why chunks did not apply (form 3 only): 1 list shorter than CH_MIN_LIST, 2 BWTS_DENSE=tiles, 3 no room for the store, 4 no room for the order block,
 * 5 no room for the big list; 15 need_sa (forms 2 and 3; else 0); 16 how the rounds ended: 0 there were none, 1 list empty, 2 no group split; 17, 18, 19
 * elements the stable finish laid out from chunks, from the big list, from the tile list; 20 rounds, round 0 included; 21 sparse:
 * log2 of the key directory's size, 0 without one; 22 tiles: the one-off order sort ran; 23 tied when the rounds ended.
 * Chunks, words 24..35: 24 S, the nominal chunk size at the start; 25 maxchunks; 26 a_small, elements of groups of at most 256;
 * 27 the big list's first size; 28, 29, 30 m_exit, m_stay and groups staying of the first split; 31 wide_possible; 32 factor
 * starts in LDS (1) or the general instantiation (0); 33 compactions done; 34 always 0 (it counted refused compactions while the tables could be too small for a re-cut); 35 a round was
 * enqueued behind the last one.  All of 24..35 stay 0 when the chunk form did not run to its end (form 3 after a hand-over included).
 * 36 the direct form: 0 not tried, 1 all groups settled (form 4), 2 fell back to the sparse rounds on a group above its cap, 3 fell
 * back on two rotations equal beyond its depth.  37 (BWTS_FWD_LEAN_WORD) the lean last pass of round 0, which leaves the group flags
 * and the tied positions instead of the sorted keys and the suffix array: 0 not tried, 1 held, 2 gave up on a run of equal low key
 * words too long across a tile seam, 3 gave up on the tied count (above n / 32), 4 the direct form gave up behind it; after 2, 3 and 4
 * the classic last pass ran from the same input and words 0..36 and the rounds are what they are without the lean pass.
 * 38 chunks: the nominal chunk size after the last compaction, 0 without one (it is below word 24 when the list had shrunk enough;
 * 0 as words 24..35 when the chunk form did not run to its end).  Words 39..47 stay 0.
 * Rounds, BWTS_FWD_ROUND_WORDS words each, the first BWTS_MAX_ROUND_STATS rounds after round 0 (those past that are counted in word 20
 * and leave no record): 0 form, as header word 13; 1 h; 2 list going in; 3 list coming out; 4 a group split in this round (1) or none did (0; direct: always 1); then sparse: 5 probe: 0 list of at most 4096, 1 ran, 2 skipped after skip_next; 6 m_big; 7 whole; 8 skip_next;
 * chunks: 5, 6 elements in chunks before and after; 7, 8, 9 big list before, stays, leaves; 10 chunks in the tables; 11 the nominal
 * chunk size, both as the round ran (what leaves is appended behind, cut by that size);
 * tiles: 5 m_big.
 * out receives whole records while they fit into cap_words; *sorts = sorts the call made.  Returns the records written, < 0 on a
 * bad argument. */
#define BWTS_FWD_HEADER_WORDS 48
#define BWTS_FWD_LEAN_WORD 37
#define BWTS_FWD_ROUND_WORDS 12
#define BWTS_FWD_SORT_WORDS (BWTS_FWD_HEADER_WORDS + BWTS_MAX_ROUND_STATS * BWTS_FWD_ROUND_WORDS)
int bwts_debug_forward_report(bwts_ctx *ctx, uint64_t *out, uint64_t cap_words, uint64_t *sorts);

/* Pure arithmetic, no context and no device: how the entropy coder (bwts_ec.h) cuts one input of 1 <= n <= 2^36 bytes.  out = {T, the
 * tile size in bytes; K, the tiles that share one frequency table; tiles = ceil(n / T); blocks = ceil(tiles / K); the bound of the
 * stream in bytes}.  Returns 0, -1 on a bad argument. */
int bwts_debug_ec_plan(uint64_t n, uint64_t out[5]);
/* Pure arithmetic, no context and no device: how the checksum (bwts_pack.h) cuts one input of 1 <= n <= 2^36 bytes.  out = {T, the tile
 * size in bytes; G, the tile values one wave folds at the second level; tiles = ceil(n / T); groups = ceil(tiles / G)}.  Returns 0, -1
 * on a bad argument. */
int bwts_debug_crc_plan(uint64_t n, uint64_t out[4]);
/* Pure arithmetic, no context and no device: how the zero-run stage (bwts_zrl.h) cuts one input of 1 <= n <= 2^36 bytes.  out = {T, the
 * tile size in bytes the kernels use; tiles = ceil(n / T)}.  Returns 0, -1 on a bad argument. */
int bwts_debug_zrl_plan(uint64_t n, uint64_t out[2]);
/* Pure arithmetic, no context and no device: how the byte-plane split (bwts_planes.h) cuts one input of 1 <= n <= 2^36 bytes at a width
 * of 2, 4 or 8.  out = {T, the tile size in bytes (4096 elements); tiles = ceil(n / T); q, the whole elements; the bytes of the tail}.
 * Returns 0, -1 on a bad argument. */
int bwts_debug_planes_plan(uint64_t n, uint32_t width, uint64_t out[4]);
/* Pure arithmetic, no context and no device: what a range read of a frame (bwts_pack.h: bwts_unpack_ranges) would decode and move for `count` ranges
 * (offset, bytes pairs, as bwts_range) of the frame of in_bytes bytes whose first 32 + entry x nblk bytes are at `frame` (nothing
 * behind them is read) into an output of out_cap bytes.  Returns the call's code for frame and ranges (0, or the negative code of
 * the first check that refuses), -1 also for NULL pointers.  On 0, out = {0 covered blocks, 1 runs, 2 C: the covered bytes, 3 the
 * covered streams' bytes, 4 the covered coded_bytes (version 1: C), 5 the output's bytes, 6 T: the tile of copy_pieces_kernel in
 * bytes, 7 the words the lists take: 2 runs + 3 runs + 3 count}, and, where cap_words holds them, lists = the runs as (first block,
 * blocks), then one stream piece per run as (offset in the frame, offset in the gathered streams, bytes), then one output piece per
 * range as (offset in the covered-block buffer, offset in the output, bytes). */
int bwts_debug_unpack_ranges_plan(const uint8_t *frame, uint64_t in_bytes, const uint64_t *ranges, uint64_t count, uint64_t out_cap,
                                  uint64_t out[8], uint64_t *lists, uint64_t cap_words);
/* What the most recent bwts_unpack_ranges / _device on the context did (host memory, no device work; all 0 before any call and
 * after one that was refused by the frame checks).  out = {0 covered blocks, 1 runs, 2 C, 3 stream bytes read, 4 the stream gather
 * ran, 5 output pieces, 6 stages run, a bit each: 1 gather, 2 decode, 4 zero-run decode, 8 inverse move-to-front, 16 inverse
 * transform, 32 join, 64 checksums, 128 cut-out, 256 delta decode, 512 the regrouping of a covered set that holds both chain and
 * direct members (bwts_members.h, version 3; where every covered member is direct, none of 4, 8, 16 and 512); 7 the single-input
 * stages were used (one covered block)}. */
int bwts_debug_unpack_ranges_report(bwts_ctx *ctx, uint64_t out[8]);
/* copy_pieces_kernel alone: `count` pieces as (offset in d_src, offset in d_dst, bytes) triples.  BWTS_E_ARG, before anything is
 * launched, for NULL pointers, count == 0, a piece of no bytes, a piece that leaves either buffer, or two pieces that share a
 * destination byte. */
int bwts_debug_copy_pieces(bwts_ctx *ctx, const void *d_src, uint64_t src_bytes, const uint64_t *pieces, uint64_t count, void *d_dst,
                           uint64_t dst_bytes);

#ifdef __cplusplus
}
#endif
#endif
