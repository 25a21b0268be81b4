/*
 * bwts_mtf.h -- move-to-front (MTF), the recency ranking a block-sorting compressor applies to BWTS output, on the device.
 *
 * Not part of the drop-in surface of the two reference programs (include/bwts.h is, and stays as it is): NealB/Bijective-BWT stops
 * at the transform.  This is the stage right behind it, for callers that keep the bytes in device memory.
 *
 * Forward: start with the list L[k] = k, k = 0 .. 255.  For each input byte c in order, output the index k with L[k] == c, then move
 * c to the front (L[1..k] = L[0..k-1], L[0] = c).  Inverse: the same list; for each input byte k, output c = L[k], then move c to
 * the front.  Both are bijections on byte strings of any length: every byte string is a valid input to either.
 * Segment forms: the list is reset to the identity at the start of every segment; segment s of the output is byte for byte what
 * the single call gives for segment s alone.
 *
 * Semantics are those of the transform's entry points of the same shape (bwts.h): the calls run on the context's stream and are
 * synchronous; BWTS_E_ARG on NULL pointers, n == 0, count == 0 or a zero length; the device forms refuse a d_out that overlaps d_in,
 * the host forms stage their buffers like bwts_forward: out may equal in, and a failed call leaves out as it was.  Single inputs up to 2^36 bytes
 * (BWTS_E_RANGE above), segment sums up to 2^32 (BWTS_E_RANGE above, before the data is looked at).
 * Cost: working memory of n / 16 bytes plus a few MiB (256 bytes per 4 KiB tile; a segment's last tile may be shorter), taken from
 * the context's arena: a call behind a transform of the same bytes allocates nothing.  bwts_last_timings: n and total_ms are
 * filled, the kernels are accounted under BWTS_K_OTHER.
 */
#ifndef BWTS_MTF_H
#define BWTS_MTF_H

#include "bwts.h"

#ifdef __cplusplus
extern "C" {
#endif

int bwts_mtf_forward_device(bwts_ctx *ctx, const void *d_in, uint64_t n, void *d_out);
int bwts_mtf_inverse_device(bwts_ctx *ctx, const void *d_in, uint64_t n, void *d_out);
int bwts_mtf_forward(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out);
int bwts_mtf_inverse(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out);
int bwts_mtf_forward_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, void *d_out);
int bwts_mtf_inverse_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, void *d_out);
int bwts_mtf_forward_segments(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, uint64_t count, uint8_t *out);
int bwts_mtf_inverse_segments(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, uint64_t count, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif
