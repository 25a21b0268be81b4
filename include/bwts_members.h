/*
 * bwts_members.h -- the member frame: arrays of any lengths and element widths packed in one call, into one frame, and read back
 * whole, by byte ranges or member by member.  A checkpoint, a snapshot or a column store is such a set: bf16 beside float32 beside
 * int64 beside raw bytes.  The frames of bwts_pack.h cut one input into equal blocks at one width; here every member is a block of
 * its own, split (bwts_planes.h) at its own width, and all members go through every stage together, in one launch per stage.
 *
 * Not part of the drop-in surface of the two reference programs (include/bwts.h is, and stays as it is).
 *
 * The frame (all integers little-endian).  count members of len_k >= 1 bytes and width w_k in {1, 2, 4, 8}; n is the sum of the
 * len_k, 1 <= n <= 2^32, 1 <= count <= 2^20 (the largest directory a "BWTZ" frame can have: 2^32 / 4096).
 *   1. Header, 32 bytes:
 *        offset  0  u32 magic 0x4D545742 ("BWTM")
 *        offset  4  u32 version = 1, or 2 where a member names a filter, or 3 where one names a method (below)
 *        offset  8  u64 n
 *        offset 16  u64 count; version 3: u32 count and, at offset 20, u32 ext, the 8-byte words of the extension table (below);
 *                   versions 1 and 2 have the upper half zero, and count <= 2^20 always fits
 *        offset 24  u32 CRC-32 of the directory bytes (version 3: the entries and the extension table)
 *        offset 28  u32 CRC-32 of header bytes 0 .. 27
 *   2. Directory, count x 32 bytes:
 *        offset  0  u64 stream_bytes
 *        offset  8  u32 CRC-32 of the member's original bytes (before the split)
 *        offset 12  u32 w; version 2: bits 0-7 w, bits 8-15 the member's filter f (bwts_delta.h: 0 none, 1 delta), bits 16-31 zero;
 *                   version 3: bits 16-23 the member's method (0 or 1, below), bits 24-31 zero
 *        offset 16  u64 coded_bytes (the zero-run stage's out_bytes for the member: 1 <= coded_bytes <= len)
 *        offset 24  u64 len (the slot that versions 2 and 3 of the "BWTZ" frame keep zero)
 *   3. Streams: for every member in order the version-1 stream of bwts_ec.h of ZRL(MTF(BWTS(SPLIT_w(member)))); w = 1 means no
 *      split; every member is split on its own, with the tail rule of bwts_planes.h; each stream a multiple of 16 bytes, together
 *      exactly what bwts_ec_encode_segments_device writes for the coded_bytes lengths.  Version 2: a member with f = 1 goes through
 *      the delta filter of bwts_delta.h at its width first, ZRL(MTF(BWTS(SPLIT_w(DELTA_w(member))))); the CRC-32 stays that of the
 *      original bytes.
 * The frame is canonical: only a version-2 frame may name a filter, and a version-2 frame in which no entry names one does not
 * exist.  A pack without a filter writes the version-1 frame, byte for byte.
 *
 * Version 3: a method per member.  BWTS_METHOD_CHAIN = 0 is the chain above.  BWTS_METHOD_ORDER0 = 1 codes the member's planes
 * directly: (DELTA_w if asked,) SPLIT_w, coder -- no transform, no move-to-front, no zero-run stage.  That is the right method for
 * weights, noise and hashes, whose bytes are close to independent (the transform and move-to-front make the coder's input less
 * skewed than the plain planes, at forty times the cost), and the wrong one for text, integer walks and smooth fields: it is asked
 * for per member, like the width and the filter, and is never a default.
 *   The cut of a method-1 member of len bytes and width w into coder segments, with q = floor(len / w):
 *     w > 1 and q >= 8192: w segments, planes 0 .. w-2 of q bytes each, and plane w-1 followed by the tail, q + (len - q w) bytes
 *       (the planes as bwts_planes.h lays them out);
 *     otherwise (w = 1 and len < w among it): one segment of len bytes.
 *   The member's stream is its segments' version-1 streams of bwts_ec.h, one behind the other: every plane of a long member has
 *   tables of its own, which is where the gain lies (a coder block across a plane boundary mixes an exponent plane with a mantissa
 *   plane).  A stream of its own costs 800 bytes before its first symbol, which planes of 8192 bytes repay.
 *   Entries: coded_bytes = len; stream_bytes = the sum of the member's segment streams.
 *   Extension table, behind the count entries: for every method-1 member that has w > 1 segments, in member order, w x u64, the
 *   segments' stream sizes; the whole table zero-padded to a multiple of 16 bytes; ext counts its 8-byte words, the pad word among
 *   them.  Fixed bytes: 32 + 32 count + 8 ext; the streams begin behind them.
 *   Canonical again: the version is 3 where any member names method 1, else 2 where any names a filter, else 1; a pack that names
 *   no method writes the frame it always wrote, byte for byte, and a version-3 frame in which no entry names a method does not exist.
 *   "BWTZ" frames have no method.
 * Bound: 32 + 32 count + the sum of bwts_ec_bound(len_k); with methods, bwts_pack_members_bound_m: 32 + 32 count + 8 ext + the sum of
 * bwts_ec_bound over all coder segments (a chain member's one of len_k bytes, a direct member's by the cut).  Header and directory are written last: a pack that fails with
 * BWTS_E_SPACE has written nothing at all.
 * Members of width 1 and one length B >= 4096 make the streams of the version-2 "BWTZ" frame of the same bytes at block_bytes = B,
 * byte for byte; only the header and the entries' width and length words differ.
 *
 * A frame is not trusted.  It is refused with BWTS_E_FORMAT unless noted, in this order:
 *    1. in_bytes < 64 or not a multiple of 16;
 *    2. wrong magic or version;
 *    3. a wrong header CRC;
 *    4. n = 0 (n > 2^32: BWTS_E_RANGE);
 *    5. count = 0 or count > n (count > 2^20: BWTS_E_RANGE);
 *    6. a directory (version 3: with its extension table) longer than the frame;
 *    7. a wrong directory CRC;
 *    8. per entry, in order: w not in {1, 2, 4, 8} (version 1: the whole word is w; version 2: a filter above 1 or a nonzero bit
 *       16-31 is refused here too); len = 0, or a running sum of the lengths above n; coded_bytes outside [1, len]; stream_bytes not a
 *       multiple of 16, or outside what the coder can make of coded_bytes;
 *       version 3, in the same place: a method above 1 or a nonzero bit 24-31 with the bad width; behind coded_bytes, for a member of
 *       method 1, coded_bytes != len; for a member with several segments, instead of the bounds on stream_bytes: its table words
 *       reaching beyond ext, a table word that is not a multiple of 16 or lies outside what the coder can make of its segment's
 *       length, or a sum of the words that is not stream_bytes (a member of one segment is held to the bounds on stream_bytes itself);
 *    9. version 2 and no entry names a filter; version 3 and no entry names a method, an ext that is not exactly what the entries
 *       demand, or a pad word that is not zero;
 *   10. a sum of the lengths that is not n;
 *   11. 32 + 32 count + 8 ext + the sum of stream_bytes != in_bytes;
 *   12. n > out_cap: BWTS_E_SPACE.
 * After the checks unpack runs version 3's order: decode against coded_bytes (a stream whose header names another length is
 * BWTS_E_FORMAT), zero-run decode, inverse move-to-front, inverse transform, the join of every member at its own width, and the
 * CRC-32 of every member against the directory: BWTS_E_CHECKSUM.  A frame whose width word was rewritten to another valid width
 * decodes in bounds and fails with BWTS_E_CHECKSUM.  Version 2: behind the join of all members, one delta decode over the filtered
 * ones (one launch per sweep), then the CRCs; a rewritten filter bit that leaves the frame canonical decodes in bounds and fails
 * with BWTS_E_CHECKSUM.  Unpack still holds one block of n bytes beside d_out: with a stage more, the first stage writes the
 * other buffer, and the last one lands in d_out.
 * Version 3: one coder decode over all coder segments; the chain members' coded bytes are gathered and go through zero-run decode,
 * inverse move-to-front and the inverse transform under a segment table of their own; the split bytes are gathered back into member
 * order; join, delta decode and the CRCs run over all members.  Where every member is direct, no stage between coder and join is
 * entered, nothing is gathered and the transform's arena is not taken; where none is, the calls are those of version 2.  A
 * rewritten method bit that leaves the frame canonical decodes in bounds and fails with BWTS_E_FORMAT (the streams do not fit the
 * other cut) or BWTS_E_CHECKSUM; so do two table words exchanged.
 *
 * bwts_unpack, bwts_unpack_device, bwts_unpack_size, bwts_unpack_ranges and bwts_unpack_ranges_device (bwts_pack.h) take member
 * frames as they take "BWTZ" frames: unpack gives the concatenation of the members, and a range's offset is counted in that
 * concatenation; the members it touches are decoded, whole (filter included), and nothing else.  Every promise of the "Ranges" comment of bwts_pack.h
 * holds with "member" for "block".
 *
 * The calls.  The members lie back to back in d_in (in), in order; widths == NULL means width 1 for every member.  Semantics are those
 * of bwts_pack.h: synchronous, on the context's stream; BWTS_E_ARG on NULL pointers, count == 0, a zero length or a width that is
 * not 1, 2, 4 or 8; BWTS_E_RANGE for count > 2^20 or a sum of the lengths above 2^32, decided before the data is touched; the
 * device forms refuse buffers that overlap and a coded side that is not 16-byte aligned.  Pack never fails with BWTS_E_SPACE for
 * out_cap >= bwts_pack_members_bound.  One member goes through the single-input stages, several through the segment forms: the
 * bytes are the same by the segment forms' contract.
 * bwts_pack_members_f* are the same calls with a filter per member (bwts_delta.h; filters == NULL: none; a filter other than 0 or 1
 * is BWTS_E_ARG with the bad widths); the bound is bwts_pack_members_bound, the filter never changes a length.
 * bwts_pack_members_m* are the same calls with a method per member besides (methods == NULL: all 0; a method other than 0 or 1 is
 * BWTS_E_ARG with the bad widths and filters); the bound is bwts_pack_members_bound_m, which without a method is
 * bwts_pack_members_bound.  Every reader above, bwts_unpack_members* and bwts_frame_members* take version 3 as they take the others;
 * a touched direct member is decoded whole, with all its streams, its join and its filter.  bwts_frame_members_m gives the methods too
 * (all 0 below version 3).
 * bwts_frame_members is host arithmetic: it judges header and directory of a frame that is all of in_bytes (checks 1 to 11) and
 * gives the members' lengths and widths (of a version-2 entry the low byte); with both arrays NULL the count alone, else BWTS_E_SPACE
 * where cap < count.  bwts_frame_members_f gives the filters too (all 0 for a version-1 frame).  A "BWTZ" frame is BWTS_E_FORMAT here.
 * bwts_unpack_members* is the range reader with whole members as ranges: indices may come in any order and may repeat, a member is
 * decoded once, and the results lie back to back in the order asked.  indices == NULL is BWTS_E_ARG with the other NULL
 * pointers; after the frame checks: BWTS_E_ARG for icount == 0, BWTS_E_RANGE for icount > 2^20 or an index >= count, BWTS_E_SPACE
 * for a sum above out_cap; nothing is written to d_out (out) by a call that fails.  A "BWTZ" frame is BWTS_E_FORMAT here.
 * Cost: that of a version-3 pack or unpack of n bytes in `count` blocks; the split and the join are one launch each whatever the
 * mix of widths, and are left out where every width is 1; the delta stage is one launch per sweep whatever the mix of filters, and is
 * left out where there is none.  bwts_timings::device_bytes after a version-2 call is what the version-1 frame of the same lengths leaves.
 * A direct member costs a checksum, a split and the coder; in a mixed frame two gathers (a copy each) besides, and the transform's
 * arena is sized for the chain members alone.
 *
 * The estimate.  bwts_members_estimate* give, for every member, what the order-0 coder would make of its byte planes as they are
 * (est_none) and of the planes of its delta-filtered elements (est_delta), in bytes, from one read of the input.  Exact integer
 * arithmetic, the same on the device, on the host and in tests/estimate_model.py:
 *   a member of len bytes and width w has q = floor(len / w) elements; its tail of len - q w bytes is copied under either filter and
 *   is not counted.  The member is cut into units of 2^18 elements (what one 256 KiB coder block of a plane spans).  For every unit,
 *   every plane p < w and both filters, c[0..255] is the histogram of byte p of the unit's elements: filter 0 takes the element
 *   itself, filter 1 zigzag(element - predecessor) at width w as bwts_delta.h defines it, with 0 in front of the member's first
 *   element and the last element of the unit before in front of a unit's first.  With N the sum of c,
 *       bits = N lg(N) - sum over s of c[s] lg(c[s]), 0 where that would be negative;  a unit's plane costs ceil(bits / (8 * 2^16)) bytes,
 *   and the estimate is the sum over the member's units and planes; q = 0 gives 0 and 0.
 *   lg(x), 1 <= x < 2^32, is a fixed-point log2 with 16 fraction bits: k = the place of x's highest bit, y = x * 2^(31 - k), and
 *   sixteen times: y = floor(y * y / 2^31); the next fraction bit is 1, and y = floor(y / 2), where y >= 2^32, else 0.  lg(x) = k * 2^16 + the
 *   fraction bits, first one highest.  No floating point is used anywhere.
 * The estimate is a statement about planes, not a promise of a frame size; a member that the coder would code as one stream is
 * estimated by the same definition.  Refusals are those of bwts_pack_members (est_none or est_delta NULL: BWTS_E_ARG); working
 * memory is 16 bytes per unit.  bwts_last_timings: n and total_ms are filled, the kernel is accounted under BWTS_K_OTHER, as one
 * launch more in a pack that leaves a filter open.
 *
 * AUTO.  bwts_pack_members_a* take BWTS_FILTER_AUTO and BWTS_METHOD_AUTO (255) beside the values above, per member, and resolve them
 * by the rules of this writer; the frame is, byte for byte, what bwts_pack_members_m* writes for the resolved arrays (its canonical
 * version 1, 2 or 3 among it), which filters_out and methods_out give where they are not NULL, and which every reader takes as it
 * takes any other: the choice stands in the directory.  bwts_pack_members_m* refuse 255 as they always did.
 *   A filter AUTO becomes delta iff est_delta + (est_none >> 6) < est_none, else none: a filter must save more than 1/64 of the
 *   estimate, since one that buys nothing costs a decode sweep.  The filter is chosen by the estimate whatever the member's method.
 *   A method AUTO: the member is encoded both ways at its resolved filter; a way's cost is its stream_bytes + 8 x its extension-table
 *   words (none for the chain); the smaller cost wins, and a tie goes to the chain (method 0).
 *   The estimator runs only where some filter is AUTO, and over those members alone.  Checksum, filter and split run once; the
 *   chain stages run once, over the members that name the chain or AUTO; the coder runs over both sets of candidates into a block the
 *   context keeps for such calls, sized by the candidates' bounds, and the winners' streams are copied to their places.  A call whose
 *   arrays name no AUTO launches exactly what bwts_pack_members_m* launches; so does one with filters AUTO alone, behind the estimator.
 *   Bound: bwts_pack_members_bound_a: an AUTO member counts with the larger of its two bounds, and the extension table with every AUTO
 *   member's words; without AUTO it is bwts_pack_members_bound_m.  No BWTS_E_SPACE for out_cap >= that bound; header and directory are
 *   written last, behind the streams, and a call that fails with BWTS_E_SPACE has written nothing.
 *
 * Pointers.  Tensors do not lie back to back: the _p calls take every member where it is.  d_srcs, d_dsts and d_members are host
 * arrays of `count` device pointers; no alignment is asked of a member, and none need be a whole allocation.
 *   bwts_gather_device copies member k, lengths[k] >= 1 bytes at d_srcs[k], to d_out, the members back to back in order;
 *   bwts_scatter_device copies them from d_in, back to back, to d_dsts[k].  One launch of the copy kernel between scattered buffers
 *   (csrc/pieces.hip): it reads nothing but a source member's own bytes, writes nothing but a destination's, and makes no access wider
 *   than a byte at an address that is not a multiple of its width.  Refusals: BWTS_E_ARG for NULL pointers, count == 0 or a zero
 *   length, BWTS_E_RANGE for count > 2^20 or a sum above 2^32; then BWTS_E_ARG for a NULL entry, for a member that shares a byte with
 *   the contiguous side, and on scatter for two destinations that share a byte.  Sources of a gather may overlap or repeat.
 *   bwts_pack_members_p_device is bwts_pack_members_a_device over such a table (AUTO values, NULL widths, filters and methods, the
 *   bound and filters_out / methods_out with that call's meaning): the frame is, byte for byte, what that call writes for the same
 *   members back to back, so no reader and no version changes.  The set is gathered into a block of n bytes that the context keeps
 *   for this purpose (counted in bwts_timings::device_bytes, given up by bwts_ctx_release_memory); a set that lies back to back already,
 *   d_members[k + 1] == d_members[k] + lengths[k] for all k, is passed on as it is and launches what the contiguous call launches.
 *   Refusals, in this order: those of bwts_pack_members_a_device; a NULL table or entry, BWTS_E_ARG; a member that shares a byte with
 *   [d_out, d_out + out_cap), BWTS_E_ARG.  Members may overlap one another or repeat.
 *   bwts_unpack_members_p_device is bwts_unpack_members_device with a destination per index: member indices[j] goes to d_dsts[j], of
 *   which dst_bytes[j] bytes may be written and only the member's len are.  indices == NULL means every member in order, and icount
 *   must then be the frame's count (BWTS_E_ARG).  Indices may come in any order and may repeat; a member is decoded once and written to
 *   every destination that names it.  Refusals, in this order: NULL ctx or d_in, in_bytes == 0, d_in not 16-byte aligned, BWTS_E_ARG;
 *   the frame checks and the index checks of bwts_unpack_members_device, with their codes; a NULL table or entry, BWTS_E_ARG;
 *   dst_bytes[j] below the member's length, BWTS_E_SPACE; two destinations that share a byte (of their members' len bytes), or one
 *   that overlaps the frame, BWTS_E_ARG.  The decode ends in a block the context keeps, every member's CRC-32 is compared there, and
 *   only then is anything scattered: a call that fails, BWTS_E_CHECKSUM and the coder's BWTS_E_FORMAT among it, has written nothing
 *   to any destination.
 *   The range readers have no pointer form.
 */
#ifndef BWTS_MEMBERS_H
#define BWTS_MEMBERS_H

#include "bwts_pack.h"

#ifdef __cplusplus
extern "C" {
#endif

/* every segment split, or joined, at a width of its own: 1 (copied), 2, 4 or 8; one launch.  Otherwise the segment calls of
 * bwts_planes.h, plus BWTS_E_ARG for widths == NULL or a width outside {1, 2, 4, 8} */
int bwts_planes_split_segments_w_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, uint64_t count, void *d_out);
int bwts_planes_join_segments_w_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, uint64_t count, void *d_out);

#define BWTS_METHOD_CHAIN  0
#define BWTS_METHOD_ORDER0 1

uint64_t bwts_pack_members_bound(const uint64_t *lengths, uint64_t count);      /* 0 on bad arguments */
uint64_t bwts_pack_members_bound_m(const uint64_t *lengths, const uint32_t *widths, const uint32_t *methods, uint64_t count);    /* likewise */
int bwts_pack_members_m_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters,
                               const uint32_t *methods, uint64_t count, void *d_out, uint64_t out_cap, uint64_t *out_bytes);
int bwts_pack_members_m(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters,
                        const uint32_t *methods, uint64_t count, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes);
int bwts_frame_members_m(const uint8_t *frame, uint64_t in_bytes, uint64_t *lengths_out, uint32_t *widths_out, uint32_t *filters_out,
                         uint32_t *methods_out, uint64_t cap, uint64_t *count);
int bwts_pack_members_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, uint64_t count, void *d_out,
                             uint64_t out_cap, uint64_t *out_bytes);
int bwts_pack_members(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, const uint32_t *widths, uint64_t count, uint8_t *out,
                      uint64_t out_cap, uint64_t *out_bytes);
int bwts_frame_members(const uint8_t *frame, uint64_t in_bytes, uint64_t *lengths_out, uint32_t *widths_out, uint64_t cap, uint64_t *count);
int bwts_pack_members_f_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters, uint64_t count,
                               void *d_out, uint64_t out_cap, uint64_t *out_bytes);
int bwts_pack_members_f(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters, uint64_t count,
                        uint8_t *out, uint64_t out_cap, uint64_t *out_bytes);
int bwts_frame_members_f(const uint8_t *frame, uint64_t in_bytes, uint64_t *lengths_out, uint32_t *widths_out, uint32_t *filters_out, uint64_t cap,
                         uint64_t *count);
int bwts_unpack_members_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, const uint64_t *indices, uint64_t icount, void *d_out,
                               uint64_t out_cap, uint64_t *out_bytes);
int bwts_unpack_members(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const uint64_t *indices, uint64_t icount, uint8_t *out,
                        uint64_t out_cap, uint64_t *out_bytes);

/* the estimate: est_none and est_delta are host arrays of count */
int bwts_members_estimate_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, uint64_t count,
                                 uint64_t *est_none, uint64_t *est_delta);
int bwts_members_estimate(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, const uint32_t *widths, uint64_t count,
                          uint64_t *est_none, uint64_t *est_delta);

/* a filter or a method that the pack chooses (bwts_pack_members_a* alone take them) */
#define BWTS_FILTER_AUTO 255u
#define BWTS_METHOD_AUTO 255u

uint64_t bwts_pack_members_bound_a(const uint64_t *lengths, const uint32_t *widths, const uint32_t *methods, uint64_t count);    /* 0 on bad arguments */
/* filters_out, methods_out: host arrays of count for the resolved values, or NULL */
int bwts_pack_members_a_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters,
                               const uint32_t *methods, uint64_t count, void *d_out, uint64_t out_cap, uint64_t *out_bytes,
                               uint32_t *filters_out, uint32_t *methods_out);
int bwts_pack_members_a(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters,
                        const uint32_t *methods, uint64_t count, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes,
                        uint32_t *filters_out, uint32_t *methods_out);

/* members where they lie ("Pointers"): d_srcs, d_dsts, d_members are host arrays of device pointers */
int bwts_gather_device(bwts_ctx *ctx, const void *const *d_srcs, const uint64_t *lengths, uint64_t count, void *d_out);
int bwts_scatter_device(bwts_ctx *ctx, const void *d_in, void *const *d_dsts, const uint64_t *lengths, uint64_t count);
int bwts_pack_members_p_device(bwts_ctx *ctx, const void *const *d_members, const uint64_t *lengths, const uint32_t *widths,
                               const uint32_t *filters, const uint32_t *methods, uint64_t count, void *d_out, uint64_t out_cap,
                               uint64_t *out_bytes, uint32_t *filters_out, uint32_t *methods_out);
int bwts_unpack_members_p_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, const uint64_t *indices, uint64_t icount,
                                 void *const *d_dsts, const uint64_t *dst_bytes);

#ifdef __cplusplus
}
#endif
#endif
