/*
 * bwts_ec.h -- entropy coding of move-to-front ranks on the device: a static order-0 rANS coder and decoder, the stage behind
 * bwts_mtf.h and the first whose output is smaller than its input.
 *
 * Not part of the drop-in surface of the two reference programs (include/bwts.h is, and stays as it is).  Any byte string is a valid
 * input to the encoder; ranks are what it is built for.
 *
 * The stream, version 1 (all integers little-endian).  T = 16384 bytes per tile, K = 16 tiles per model block, 12-bit probabilities
 * (M = 4096), rANS states are u32 in [2^16, 2^32), renormalisation moves 16-bit words, ROW = 1024.  An input of n >= 1 bytes has
 * nt = ceil(n / T) tiles and nb = ceil(nt / K) blocks; block b covers bytes [b K T, min(n, (b + 1) K T)).
 *   1. Header, 16 bytes: u32 magic 0x43455742 ("BWEC"), u32 params = 14 | 4 << 8 | 12 << 16, u64 n.
 *   2. Tables, nb x 512 bytes: 256 x u16 frequencies f[s] per block, summing to 4096, from the block's byte counts h[s] (m = sum h):
 *      f[s] = 0 where h[s] = 0, else max(1, floor(4096 h[s] / m)); with d = 4096 - sum f: if d > 0, d is added, once, to the symbol with
 *      the largest f (lowest s on ties); if d < 0, -d times 1 is taken from the symbol that then has the largest f (lowest s on ties).
 *      c[s] is the exclusive prefix sum of f.
 *   3. Tile directory: nt x u32 payload sizes in bytes, zero-padded to a multiple of 16.
 *   4. Payloads in tile order: 64 x u32 final lane states, then the 16-bit words in the order the decoder reads them, then zero
 *      padding to a multiple of 16 (so less than 16 bytes: every payload size is >= 256 and a multiple of 16).
 * Inside a tile of len bytes, position p belongs to lane (p >> 4) & 63 and is that lane's step (p >> 10) 16 + (p & 15); steps run
 * 0 .. S - 1, S = 16 ceil(len / ROW); a lane is inactive in a step whose position is >= len.
 * Decoder: for j = 0 .. S - 1 every active lane does slot = x & 4095, s = the symbol with c[s] <= slot < c[s] + f[s],
 * x = f[s] (x >> 12) + slot - c[s], output s; then the active lanes with x < 2^16 take the next words of the payload in ascending lane
 * order, x = x << 16 | word.  At the end every lane's state must be 2^16 and the words taken must be all of the payload but its zero
 * padding.  Encoder: the mirror image, states from 2^16, j from S - 1 down to 0: an active lane with x >= f[s] 2^20 emits x & 0xffff
 * and shifts right by 16, then x = floor(x / f) 4096 + x mod f + c[s]; a step's words go, in ascending lane order, in front of all
 * words emitted before.
 * Segment form: the stream of segment s is byte for byte the single-input stream of segment s alone, with its own header; the
 * streams are concatenated, each a multiple of 16 bytes.
 * Bound: 16 + 512 nb + pad16(4 nt) + 272 nt + 2 n bytes (no step emits more than one word per symbol); segments: the sum.
 *
 * The format has no checksum.  The decoder refuses what it can see is malformed (BWTS_E_FORMAT) and forms every address from values
 * it has checked or clamped, so a hostile stream cannot make it read or write outside its buffers; but a changed payload bit that
 * still brings every lane back to 2^16 yields wrong bytes, in bounds, and BWTS_OK.  Callers that need integrity add their own check
 * (bwts_pack.h does: a CRC-32 per block, computed on the device).
 *
 * Semantics are those of bwts_mtf.h: the calls run on the context's stream and are synchronous; BWTS_E_ARG on NULL pointers, n == 0,
 * in_bytes == 0, count == 0, a zero length, or device buffers that overlap; single inputs up to 2^36 bytes and segment sums up to
 * 2^32 (BWTS_E_RANGE above, decided before the data is touched; also for a stream longer than the bound of 2^36 bytes, or whose
 * header names more).  The coded side of the device forms (d_out of an encode, d_in of a decode) must be 16-byte aligned
 * (BWTS_E_ARG otherwise); the byte side may have any alignment, 16-byte aligned is faster.
 * Encode never fails for out_cap >= the bound.  With less it returns BWTS_E_SPACE as soon as the real size is known to exceed
 * out_cap, and has then written nothing at all.  Decode returns BWTS_E_SPACE when the header's n exceeds out_cap.  A decode that
 * fails with BWTS_E_FORMAT may have written part of the output (the device forms; the host forms leave out as it was after any
 * failure).  The segment decode takes the caller's lengths; a header whose n differs is BWTS_E_FORMAT.
 * Cost: two passes over the input to encode (a counting pass, then every word straight to its place), one to decode; working memory
 * of about n / 64 bytes from the context's arena.  bwts_last_timings: n (the uncoded bytes) and total_ms are filled, the kernels
 * are accounted under BWTS_K_OTHER.
 */
#ifndef BWTS_EC_H
#define BWTS_EC_H

#include "bwts.h"

#define BWTS_E_FORMAT   -8   /* not a version-1 stream: header, table, directory or payload malformed */
#define BWTS_E_SPACE    -9   /* the result does not fit into out_cap */

#ifdef __cplusplus
extern "C" {
#endif

/* host arithmetic only: the bound of one input (0 for n == 0 or n > 2^36), of a list of segments, and the n a header names
 * (BWTS_E_FORMAT: in_bytes too small or not a multiple of 16, wrong magic or parameters, n == 0, or in_bytes outside what n allows) */
uint64_t bwts_ec_bound(uint64_t n);
int bwts_ec_bound_segments(const uint64_t *lengths, uint64_t count, uint64_t *bound);
int bwts_ec_decoded_size(const uint8_t header[16], uint64_t in_bytes, uint64_t *n);

int bwts_ec_encode_device(bwts_ctx *ctx, const void *d_in, uint64_t n, void *d_out, uint64_t out_cap, uint64_t *out_bytes);
int bwts_ec_decode_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, void *d_out, uint64_t out_cap, uint64_t *n);
/* host buffers, single input */
int bwts_ec_encode(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes);
int bwts_ec_decode(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n);
/* stream_bytes: host array of count entries, written by the encode, read by the decode */
int bwts_ec_encode_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, void *d_out, uint64_t out_cap,
                                   uint64_t *stream_bytes);
int bwts_ec_decode_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *stream_bytes, const uint64_t *lengths, uint64_t count,
                                   void *d_out);

#ifdef __cplusplus
}
#endif
#endif
