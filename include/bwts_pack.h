/*
 * bwts_pack.h -- the three device stages as a compressor: pack runs transform (bwts.h), move-to-front (bwts_mtf.h) and entropy coder
 * (bwts_ec.h) over the blocks of an input and writes one self-describing frame with a CRC-32 per block; unpack checks the frame,
 * runs the chain backwards and checks every block's bytes.  The checksum kernel is a call of its own too.
 *
 * Not part of the drop-in surface of the two reference programs (include/bwts.h is, and stays as it is).
 *
 * CRC-32 is the one of zlib, gzip and PNG: reflected polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF.
 *
 * The frame, version 1 (all integers little-endian).  An input of n bytes, 1 <= n <= 2^32, is cut into nblk = ceil(n / B) blocks of
 * B bytes; the last may be shorter.
 *   1. Header, 32 bytes:
 *        offset  0  u32 magic 0x5A545742 ("BWTZ")
 *        offset  4  u32 version = 1
 *        offset  8  u64 n
 *        offset 16  u64 B
 *        offset 24  u32 CRC-32 of the directory bytes
 *        offset 28  u32 CRC-32 of header bytes 0 .. 27
 *   2. Directory, nblk x 16 bytes: u64 stream_bytes, u32 CRC-32 of the block's original (untransformed) bytes, u32 zero.
 *   3. Streams: the version-1 stream of bwts_ec.h of MTF(BWTS(block)) for every block, in order; each a multiple of 16 bytes, together
 *      exactly what bwts_ec_encode_segments_device writes for these lengths.
 * B is always the real block length: block_bytes == 0 on the way in means one block, B = n; otherwise block_bytes >= 4096, and a
 * value >= n is stored as n (a nonzero block_bytes below 4096 is BWTS_E_ARG).  So B = n or 4096 <= B < n.
 * Bound: 32 + 16 nblk + the sum of bwts_ec_bound over the blocks.
 *
 * The frame, version 2: zero-run coding (bwts_zrl.h) between the ranks and the coder.  Asked for with the _v calls; unpack takes both.
 *   1. Header: as above, with version = 2.
 *   2. Directory, nblk x 32 bytes: u64 stream_bytes, u32 CRC-32 of the block's original bytes, u32 zero, u64 coded_bytes (the zero-run
 *      stage's out_bytes for the block: 1 <= coded_bytes <= the block's length), u64 zero.
 *   3. Streams: the version-1 stream of bwts_ec.h of ZRL(MTF(BWTS(block))) for every block, in order; its header names coded_bytes;
 *      together exactly what bwts_ec_encode_segments_device writes for the coded_bytes lengths.
 * Bound: 32 + 32 nblk + the sum of bwts_ec_bound over the blocks' lengths (the zero-run stage never expands).
 *
 * The frame, version 3: version 2 with the byte-plane split (bwts_planes.h) in front of the transform, at a width w in {2, 4, 8}
 * that the caller names.  Asked for with the _planes calls (the _v calls keep to versions 1 and 2); unpack takes all three.
 *   1. Header: as above, with version = 3.
 *   2. Directory, nblk x 32 bytes: u64 stream_bytes, u32 CRC-32 of the block's original bytes (before the split), u32 w (the reserved
 *      word of versions 1 and 2; the same in every entry), u64 coded_bytes, u64 zero.
 *   3. Streams: the version-1 stream of bwts_ec.h of ZRL(MTF(BWTS(SPLIT_w(block)))) for every block, in order; every block is split
 *      on its own (a block whose length is no multiple of w keeps its tail, bwts_planes.h); otherwise as in version 2.
 * Bound: version 2's (the split never changes a length).
 * Unpack keeps version 2's order; the word at entry offset 12 is judged where versions 1 and 2 demand zero: a width that is not 2, 4
 * or 8, or that differs from the first entry's, is BWTS_E_FORMAT (so is a version-2 body under a version word of 3: its width is 0).
 * After the inverse transform every block is joined at w, and the CRC-32 of the result is held against the directory: a frame whose
 * width words name another of the three widths decodes in bounds and fails with BWTS_E_CHECKSUM.
 * The planes of a long smooth field are deeply repetitive, the transform's dear case: such a field packs at every size (2^30 bytes of
 * float32 run, in one block and in blocks of 1 MiB), but its pack takes several times as long as version 2's.
 *
 * A frame is not trusted.  Unpack refuses with BWTS_E_FORMAT, in this order: in_bytes < 48 or not a multiple of 16; wrong magic, or
 * a version that is not 1, 2 or 3; a wrong header CRC; n = 0 (n > 2^32 is BWTS_E_RANGE); B = 0, B > n, or B < 4096 with B != n; a directory longer than the
 * frame; a wrong directory CRC; an entry with a nonzero reserved word, or a stream_bytes that is not a multiple of 16 or outside
 * what the coder can make of the block's length; 32 + 16 nblk + the sum of stream_bytes != in_bytes.  Then a header n > out_cap is
 * BWTS_E_SPACE.  After the checks: decode (the coder's own BWTS_E_FORMAT passes through, and a stream whose header names another
 * length than its block's is BWTS_E_FORMAT), inverse move-to-front, inverse transform, and the CRC-32 of every block of the result
 * against the directory: a difference is BWTS_E_CHECKSUM.
 * Version 2 keeps that order with its own entries: the directory is judged to lie inside the frame with 32 bytes per block, before
 * its CRC is read; both reserved words must be zero, coded_bytes in range, and stream_bytes what the coder can make of coded_bytes.
 * After the checks: decode against coded_bytes (a stream whose header names another length is BWTS_E_FORMAT), zero-run decode of
 * every block against its length (its BWTS_E_FORMAT passes through), inverse move-to-front, inverse transform, the CRC check.
 *
 * Semantics are those of bwts_ec.h: the calls run on the context's stream and are synchronous; BWTS_E_ARG on NULL pointers, n == 0,
 * in_bytes == 0, count == 0 or a zero length; the device forms refuse buffers that overlap, and a coded side (d_out of a pack, d_in of
 * an unpack) that is not 16-byte aligned.  The checksum calls take single inputs up to 2^36 bytes and segment sums up to 2^32
 * (BWTS_E_RANGE above, decided before the data is touched) at any alignment of d_in and of the segment starts; pack takes up to
 * 2^32 bytes (BWTS_E_RANGE above).
 * Pack never fails with BWTS_E_SPACE for out_cap >= bwts_pack_bound; with less it returns BWTS_E_SPACE as soon as the frame is known
 * not to fit, and has then written nothing at all (header and directory are written last).  A device unpack that fails may have
 * written part of d_out; the host forms leave out as it was after any failure.
 * Cost: pack is one checksum pass and the three stages (version 2: four, version 3: five); between them the bytes stay in two n-byte
 * blocks that the context keeps (unpack: one; it decodes into d_out, version 2 into the block and from there into d_out, version 3
 * into d_out, from there into the block, and so on: the last stage always lands in d_out), counted in bwts_timings::device_bytes and given up by bwts_ctx_release_memory.  The checksum
 * takes four bytes per 64 KiB tile from the context's arena.  bwts_last_timings: n (the unpacked bytes) and total_ms are filled,
 * the kernels are accounted under BWTS_K_OTHER.
 */
#ifndef BWTS_PACK_H
#define BWTS_PACK_H

#include "bwts_planes.h"

#define BWTS_E_CHECKSUM -10   /* a block decoded in bounds but its bytes are not the ones that were packed */

#ifdef __cplusplus
extern "C" {
#endif

/* crc: one value; crcs: host array of count entries */
int bwts_crc32_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t *crc);
int bwts_crc32_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, uint32_t *crcs);

/* host arithmetic only: the largest frame of n bytes cut at block_bytes (0 on bad arguments), and what header and directory of a
 * frame say, of which in_bytes bytes are at hand (the frame may end before them: concatenated frames are stepped through by
 * frame_bytes; BWTS_E_FORMAT also for a frame that does not end within in_bytes) */
uint64_t bwts_pack_bound(uint64_t n, uint64_t block_bytes);
int bwts_unpack_size(const uint8_t *frame, uint64_t in_bytes, uint64_t *n, uint64_t *frame_bytes);

int bwts_pack_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint64_t block_bytes, void *d_out, uint64_t out_cap, uint64_t *out_bytes);
int bwts_unpack_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, void *d_out, uint64_t out_cap, uint64_t *n);
/* host buffers */
int bwts_pack(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint64_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes);
int bwts_unpack(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n);
/* the frame's version chosen by the caller: with version 1 these are the calls above, byte for byte; 2: zero-run coding in front of
 * the coder; any other version: BWTS_E_ARG (the bound: 0) */
uint64_t bwts_pack_bound_v(uint32_t version, uint64_t n, uint64_t block_bytes);
int bwts_pack_device_v(bwts_ctx *ctx, uint32_t version, const void *d_in, uint64_t n, uint64_t block_bytes, void *d_out, uint64_t out_cap,
                       uint64_t *out_bytes);
int bwts_pack_v(bwts_ctx *ctx, uint32_t version, const uint8_t *in, uint64_t n, uint64_t block_bytes, uint8_t *out, uint64_t out_cap,
                uint64_t *out_bytes);

/* frames of version 3: the byte-plane split at `width` (2, 4 or 8; anything else: BWTS_E_ARG, the bound: 0) in front of the
 * transform, zero-run coding in front of the coder; otherwise the calls above */
uint64_t bwts_pack_planes_bound(uint32_t width, uint64_t n, uint64_t block_bytes);
int bwts_pack_planes_device(bwts_ctx *ctx, uint32_t width, const void *d_in, uint64_t n, uint64_t block_bytes, void *d_out, uint64_t out_cap,
                            uint64_t *out_bytes);
int bwts_pack_planes(bwts_ctx *ctx, uint32_t width, const uint8_t *in, uint64_t n, uint64_t block_bytes, uint8_t *out, uint64_t out_cap,
                     uint64_t *out_bytes);

/*
 * Ranges: bytes [offset, offset + bytes) of the unpacked input, read by decoding only the blocks they touch.
 *
 * Results.  They lie back to back in d_out (out) in the order the ranges were given; *out_bytes is their sum.  Ranges may overlap,
 * repeat and come in any order; a block that several ranges touch is decoded once.
 * Versions.  All three frame versions are taken; a version-3 block is joined at its width before anything is cut out of it.  A frame
 * of one block (B = n) is covered whole by any range: the call then costs a full unpack minus the n-byte output.
 * Frame checks.  Header and the whole directory are judged exactly as bwts_unpack_device judges them, in the same order and with the
 * same codes (every block's entry, touched or not), and the frame must end at in_bytes.
 * Range checks.  Only after the frame checks are the ranges judged, in this order: BWTS_E_ARG for ranges == NULL, count == 0 or a
 * range with bytes == 0 (count > 2^20 is BWTS_E_RANGE, decided before the ranges are read); BWTS_E_RANGE for a range whose
 * offset + bytes overflows or exceeds n, or a sum of bytes above 2^32; BWTS_E_SPACE for a sum above out_cap.  All of these are
 * decided before the device touches a stream or d_out.
 * What is read.  Only the streams of covered blocks.  Every covered block's CRC-32 is held against the directory before the ranges
 * are cut out: a mismatch is BWTS_E_CHECKSUM; the coder's and the zero-run decoder's BWTS_E_FORMAT pass through, and a covered
 * stream whose header names another length than the directory's is BWTS_E_FORMAT.  Damage inside a block that no range touches
 * goes unnoticed: that is the point of the call, and a caller who wants the whole frame vouched for unpacks it.
 * Device form.  BWTS_E_ARG on NULL pointers, in_bytes == 0, a d_in that is not 16-byte aligned, or d_in and d_out that overlap; d_out
 * may have any alignment.  d_out is written by the last step alone, the cut-out behind the checksums: a call that fails has written
 * nothing to d_out.
 * Host form.  It leaves out as it was after any failure.  Only header, directory and the covered blocks' streams cross to the device.
 * Memory.  The bytes between the stages live in the two blocks that pack keeps with the context, sized for the covered bytes C (the
 * sum of the covered blocks' lengths; the gathered streams where those are longer), not for n.  bwts_last_timings: n holds C, total_ms
 * is filled, the kernels are accounted under BWTS_K_OTHER.
 */
typedef struct { uint64_t offset, bytes; } bwts_range;      /* bytes [offset, offset + bytes) of the unpacked input */

int bwts_unpack_ranges_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, const bwts_range *ranges, uint64_t count,
                              void *d_out, uint64_t out_cap, uint64_t *out_bytes);
int bwts_unpack_ranges(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const bwts_range *ranges, uint64_t count,
                       uint8_t *out, uint64_t out_cap, uint64_t *out_bytes);

#ifdef __cplusplus
}
#endif
#endif
