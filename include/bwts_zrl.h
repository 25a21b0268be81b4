/*
 * bwts_zrl.h -- zero-run coding of move-to-front ranks on the device: the stage between bwts_mtf.h and bwts_ec.h that every
 * block-sorting compressor runs, so that the coder sees a few digit bytes per run of zeros and not one byte per zero.
 *
 * Not part of the drop-in surface of the two reference programs (include/bwts.h is, and stays as it is).  Any byte string is a valid
 * input to the encoder; ranks are what it is built for.
 *
 * The coded form has no header: the caller keeps both lengths.  Input r[0 .. n), n >= 1; output z:
 *   - a maximal run of L >= 1 zeros becomes k = floor(log2(L + 1)) digit bytes d[0] .. d[k-1], each 0 or 1, with
 *     L = sum (d[i] + 1) 2^i: bijective base 2, least significant digit first (emit d = (L - 1) & 1, set L = (L - 1 - d) >> 1, repeat
 *     until L is 0);
 *   - a rank v in 1 .. 253 becomes the byte v + 1;
 *   - a rank v of 254 or 255 becomes the byte 255 followed by the byte v - 254.
 * With m the number of bytes this gives: if m < n the output is those m bytes (coded), otherwise it is the input itself, n bytes
 * (stored).  out_bytes = min(m, n): the stage never expands, and its bound is n.
 * The decoder takes (z, in_bytes, n) and trusts nothing in z:
 *   - in_bytes == n: a copy; in_bytes > n: BWTS_E_FORMAT; in_bytes < n: z is parsed.
 *   - A byte is a payload iff the byte in front of it is 255; a payload must be 0 or 1; a 255 as the last byte is BWTS_E_FORMAT.
 *   - A byte <= 1 that is no payload is a digit.  Its index i is the number of digits directly in front of it, no other byte between;
 *     it stands for (byte + 1) << i zeros; an index >= 36 is BWTS_E_FORMAT.
 *   - Every other byte and every 255 with its payload stands for one rank.  What all bytes stand for must be exactly n ranks, else
 *     BWTS_E_FORMAT.
 *   - Every output address comes from a checked or clamped value: no byte outside [0, n) of d_out is written, whatever z says.  All
 *     of the checks above are made before the first byte is written.
 * So a byte's meaning depends on at most the 37 bytes in front of it, and a run's length is the distance to the last rank that is
 * not 0: the two facts the kernels are built on.
 * Segment form: a run never crosses a segment start; the output of segment s is byte for byte the single call's for segment s alone,
 * coded or stored on its own account; the outputs are concatenated with no padding.  The encode returns out_lengths[s], the decode
 * takes both length arrays.
 *
 * Semantics are those of bwts_ec.h: the calls run on the context's stream and are synchronous; BWTS_E_ARG on NULL pointers, n == 0,
 * in_bytes == 0, count == 0, a zero length, or device buffers that overlap; single inputs up to 2^36 bytes and segment sums up to
 * 2^32 (BWTS_E_RANGE above, decided before the data is touched).  No alignment is demanded on either side; 16-byte aligned is
 * faster.  Encode never fails for out_cap >= n.  With less it returns BWTS_E_SPACE as soon as the real size is known to exceed
 * out_cap, and has then written nothing at all.  The host forms stage their buffers like bwts_ec_encode and leave out as it was
 * after any failure.
 * Cost: two passes over the input each way (encode: tile summaries, then the coded bytes through LDS; decode: tile weights, then
 * a clear of the output and a pass that places the ranks that are not 0), and a few scans over one value per 16 KiB tile.  Working
 * memory: 40 bytes per 16 KiB tile of the cut side plus a few KiB (n / 400 for an encode), from the context's arena: a call behind a
 * move-to-front call of the same bytes, more than one of its 4 KiB tiles long, allocates nothing.  bwts_last_timings: n (the uncoded
 * bytes) and total_ms are filled, the kernels are accounted under BWTS_K_OTHER.
 */
#ifndef BWTS_ZRL_H
#define BWTS_ZRL_H

#include "bwts_ec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* host arithmetic only: the bound of one input, n (0 for n == 0 or n > 2^36) */
uint64_t bwts_zrl_bound(uint64_t n);

int bwts_zrl_encode_device(bwts_ctx *ctx, const void *d_in, uint64_t n, void *d_out, uint64_t out_cap, uint64_t *out_bytes);
int bwts_zrl_decode_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, void *d_out, uint64_t n);
/* host buffers, single input */
int bwts_zrl_encode(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes);
int bwts_zrl_decode(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t n);
/* out_lengths, in_lengths: host arrays of count entries, written by the encode, read by the decode */
int bwts_zrl_encode_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, void *d_out, uint64_t out_cap,
                                    uint64_t *out_lengths);
int bwts_zrl_decode_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *in_lengths, const uint64_t *lengths, uint64_t count,
                                    void *d_out);

#ifdef __cplusplus
}
#endif
#endif
