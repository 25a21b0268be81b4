/*
 * bwts_delta.h -- delta filter of integer arrays on the device: a stage in front of the byte-plane split (bwts_planes.h) for inputs
 * whose differences are small while their values are not: counters, timestamps, sorted indices, CSR offsets, sample streams, random
 * walks.  Every element is replaced by the zigzag of its difference to the one before; the split then finds the upper planes nearly
 * all zero.  It is what HDF5 and Blosc pair with the shuffle.  It takes 15 to 20 % off an integer random walk or sorted ids and makes
 * bf16 noise 3 % larger: the caller asks for it, per array, like the width; it is never a default.
 *
 * Not part of the drop-in surface of the two reference programs (include/bwts.h is, and stays as it is).  Any byte string is a valid
 * input of either direction at any width.
 *
 * Definition.  For a string in[0 .. L) and a width w in {1, 2, 4, 8}, let q = floor(L / w), and let a_i, 0 <= i < q, be the
 * little-endian unsigned integer of the w bytes in[i w .. i w + w).  All arithmetic is mod 2^{8w}.  Encode:
 *   - d_0 = a_0, d_i = a_i - a_{i-1}                              (the difference to the element before; nothing before the first);
 *   - z_i = (d_i << 1) xor (d_i >> (8w - 1), arithmetically)      (zigzag: 0, -1, 1, -2, ... become 0, 1, 2, 3, ...; every element,
 *                                                                  the first one too);
 *   - out[i w .. i w + w) = z_i, little-endian;
 *   - out[q w + j] = in[q w + j]                                  for the L - q w bytes of the tail;
 *   - L < w is the identity (q = 0: all of the string is tail).
 * Decode is the inverse: d_i = (z_i >> 1) xor -(z_i and 1), a_i = d_0 + ... + d_i, the tail copied.  The stage has no header and never
 * changes a length.
 * Segment form: every segment has a width and a filter of its own.  BWTS_FILTER_DELTA: the segment is encoded, or decoded, on its
 * own, the sum starting anew with its first element.  BWTS_FILTER_NONE: the segment is copied, whatever its width.  The outputs lie
 * where the inputs lay.
 *
 * Semantics are those of bwts_planes.h: the calls run on the context's stream and are synchronous; BWTS_E_ARG on NULL pointers, n == 0,
 * count == 0, a zero length, a width other than 1, 2, 4 or 8, a filter other than the two named here, or buffers that overlap; single
 * inputs up to 2^36 bytes and segment sums up to 2^32 (BWTS_E_RANGE above, decided before the data is touched).  No alignment is
 * demanded on either side, nor of a segment's start.  The host forms stage their buffers like bwts_mtf_forward.
 * Cost: encode is one read and one write of n bytes in one kernel, with no working memory.  Decode reads n bytes twice and writes them
 * once: a sweep that sums every tile of 4096 elements, a scan of the tile sums, and a sweep that sums inside the tiles and writes; 8
 * bytes per tile of the context's arena.  No workgroup waits for another.  The segment forms are one launch per sweep whatever the
 * mix, and put two words per segment behind the context's segment table.  bwts_last_timings: n and total_ms are filled, the kernels
 * are accounted under BWTS_K_OTHER.
 */
#ifndef BWTS_DELTA_H
#define BWTS_DELTA_H

#include "bwts_planes.h"

#define BWTS_FILTER_NONE 0u
#define BWTS_FILTER_DELTA 1u

#ifdef __cplusplus
extern "C" {
#endif

int bwts_delta_encode_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t width, void *d_out);
int bwts_delta_decode_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t width, void *d_out);
int bwts_delta_encode_segments_f_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters,
                                        uint64_t count, void *d_out);
int bwts_delta_decode_segments_f_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters,
                                        uint64_t count, void *d_out);
/* host buffers, single input */
int bwts_delta_encode(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint32_t width, uint8_t *out);
int bwts_delta_decode(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint32_t width, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif
