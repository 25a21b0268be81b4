/*
 * bwts_planes.h -- byte-plane split of typed arrays on the device: the stage in front of the transform for inputs that are arrays of
 * 2-, 4- or 8-byte numbers.  The transform then sees all first bytes, then all second bytes, and so on, and not the bytes of one
 * number beside each other: exponent bytes no longer share their contexts with mantissa noise.  It is what HDF5's shuffle filter and
 * Blosc do.  It pays on smooth 4- and 8-byte fields (a third off the packed size) and gains nothing on 2-byte noise:
 * the caller asks for it with a width, it is never a default.
 *
 * Not part of the drop-in surface of the two reference programs (include/bwts.h is, and stays as it is).  Any byte string is a valid
 * input at any width.
 *
 * Definition.  For a string in[0 .. L) and a width w in {2, 4, 8}, let q = floor(L / w):
 *   - out[k q + i] = in[i w + k]          for 0 <= k < w, 0 <= i < q   (plane k holds byte k of every element);
 *   - out[q w + j] = in[q w + j]          for the L - q w bytes of the tail;
 *   - L < w is the identity (q = 0: all of the string is tail).
 * Join is the inverse: out[i w + k] = in[k q + i], the tail copied.  The stage has no header and never changes a length.
 * Segment form: every segment is split, or joined, on its own, with its own q and its own tail; the outputs lie where the inputs lay.
 *
 * Semantics are those of bwts_zrl.h: the calls run on the context's stream and are synchronous; BWTS_E_ARG on NULL pointers, n == 0,
 * count == 0, a zero length, a width other than 2, 4 or 8, or buffers that overlap; single inputs up to 2^36 bytes and segment sums
 * up to 2^32 (BWTS_E_RANGE above, decided before the data is touched).  No alignment is demanded on either side, nor of a segment's
 * start.  The host forms stage their buffers like bwts_mtf_forward.
 * Cost: one read and one write of n bytes in one kernel; no working memory (the segment forms put one word per segment behind the
 * context's segment table).  bwts_last_timings: n and total_ms are filled, the kernel is accounted under BWTS_K_OTHER.
 */
#ifndef BWTS_PLANES_H
#define BWTS_PLANES_H

#include "bwts_zrl.h"

#ifdef __cplusplus
extern "C" {
#endif

int bwts_planes_split_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t width, void *d_out);
int bwts_planes_join_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t width, void *d_out);
int bwts_planes_split_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, uint32_t width, void *d_out);
int bwts_planes_join_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, uint32_t width, void *d_out);
/* host buffers, single input */
int bwts_planes_split(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint32_t width, uint8_t *out);
int bwts_planes_join(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint32_t width, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif
