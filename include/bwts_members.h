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
 *        offset  4  u32 version = 1, or 2 where a member names a filter (below)
 *        offset  8  u64 n
 *        offset 16  u64 count
 *        offset 24  u32 CRC-32 of the directory bytes
 *        offset 28  u32 CRC-32 of header bytes 0 .. 27
 *   2. Directory, count x 32 bytes:
 *        offset  0  u64 stream_bytes
 *        offset  8  u32 CRC-32 of the member's original bytes (before the split)
 *        offset 12  u32 w; version 2: bits 0-7 w, bits 8-15 the member's filter f (bwts_delta.h: 0 none, 1 delta), bits 16-31 zero
 *        offset 16  u64 coded_bytes (the zero-run stage's out_bytes for the member: 1 <= coded_bytes <= len)
 *        offset 24  u64 len (the slot that versions 2 and 3 of the "BWTZ" frame keep zero)
 *   3. Streams: for every member in order the version-1 stream of bwts_ec.h of ZRL(MTF(BWTS(SPLIT_w(member)))); w = 1 means no
 *      split; every member is split on its own, with the tail rule of bwts_planes.h; each stream a multiple of 16 bytes, together
 *      exactly what bwts_ec_encode_segments_device writes for the coded_bytes lengths.  Version 2: a member with f = 1 goes through
 *      the delta filter of bwts_delta.h at its width first, ZRL(MTF(BWTS(SPLIT_w(DELTA_w(member))))); the CRC-32 stays that of the
 *      original bytes.
 * The frame is canonical: only a version-2 frame may name a filter, and a version-2 frame in which no entry names one does not
 * exist.  A pack without a filter writes the version-1 frame, byte for byte.
 * Bound: 32 + 32 count + the sum of bwts_ec_bound(len_k).  Header and directory are written last: a pack that fails with
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
 *    6. a directory longer than the frame;
 *    7. a wrong directory CRC;
 *    8. per entry, in order: w not in {1, 2, 4, 8} (version 1: the whole word is w; version 2: a filter above 1 or a nonzero bit
 *       16-31 is refused here too); len = 0, or a running sum of the lengths above n; coded_bytes outside [1, len]; stream_bytes not a
 *       multiple of 16, or outside what the coder can make of coded_bytes;
 *    9. version 2 and no entry names a filter;
 *   10. a sum of the lengths that is not n;
 *   11. 32 + 32 count + the sum of stream_bytes != in_bytes;
 *   12. n > out_cap: BWTS_E_SPACE.
 * After the checks unpack runs version 3's order: decode against coded_bytes (a stream whose header names another length is
 * BWTS_E_FORMAT), zero-run decode, inverse move-to-front, inverse transform, the join of every member at its own width, and the
 * CRC-32 of every member against the directory: BWTS_E_CHECKSUM.  A frame whose width word was rewritten to another valid width
 * decodes in bounds and fails with BWTS_E_CHECKSUM.  Version 2: behind the join of all members, one delta decode over the filtered
 * ones (one launch per sweep), then the CRCs; a rewritten filter bit that leaves the frame canonical decodes in bounds and fails
 * with BWTS_E_CHECKSUM.  Unpack still holds one block of n bytes beside d_out: with a stage more, the first stage writes the
 * other buffer, and the last one lands in d_out.
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

uint64_t bwts_pack_members_bound(const uint64_t *lengths, uint64_t count);      /* 0 on bad arguments */
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

#ifdef __cplusplus
}
#endif
#endif
