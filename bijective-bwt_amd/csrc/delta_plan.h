// delta_plan.h -- the arithmetic of the delta filter (include/bwts_delta.h) that host and device share: which widths and filters there
// are, how a segment is cut into tiles, the zigzag of one element, and the serial statements of both directions.  Plain C++ in the
// style of planes_plan.h, whose tile (E = 4096 elements) and copied tile (PLANES_COPY_T bytes) it keeps: the kernels of delta.hip, the
// host side of the calls, members_plan.h (the filter byte of a version-2 member frame) and a stand-alone host program
// (tests/delta_plan_check.cc, built with the sanitizers) all compile this file.
#pragma once
#include "planes_plan.h"

#define DELTA_FILTER_NONE 0u             // BWTS_FILTER_NONE: the segment is copied
#define DELTA_FILTER_DELTA 1u            // BWTS_FILTER_DELTA
#define DELTA_MAX_N PLANES_MAX_N

// the filter predicate, and the widths: width 1 (bytes) is differenced like the others
PLANES_HD bool delta_filter_ok(uint64_t f) { return f == DELTA_FILTER_NONE || f == DELTA_FILTER_DELTA; }
PLANES_HD bool delta_width_ok(uint64_t w) { return w == 1u || w == 2u || w == 4u || w == 8u; }
PLANES_HD uint32_t delta_log_w(uint32_t w) { return w == 1u ? 0u : (w == 2u ? 1u : (w == 4u ? 2u : 3u)); }
PLANES_HD uint64_t delta_mask(uint32_t w) { return w == 8u ? ~0ull : (1ull << (8u * w)) - 1u; }

// a string of L bytes at width w: q whole elements, then a tail of L - q w bytes that stays where it is
PLANES_HD uint64_t delta_q(uint64_t L, uint32_t w) { return L >> delta_log_w(w); }
PLANES_HD uint64_t delta_tail_at(uint64_t L, uint32_t w) { return delta_q(L, w) << delta_log_w(w); }
// Tiles of a filtered string: ceil(L / (E w)), cut from the string's own start, so that no tile lies across a segment start.  Tile j
// holds the elements [j E, min((j + 1) E, q)), none at all where q is a multiple of E and the tile is there for the tail alone; the
// last tile copies the tail.
PLANES_HD uint64_t delta_tile_bytes(uint32_t w) { return (uint64_t)PLANES_E * w; }
PLANES_HD uint64_t delta_tiles(uint64_t L, uint32_t w) { return (L + delta_tile_bytes(w) - 1u) / delta_tile_bytes(w); }
PLANES_HD uint32_t delta_tile_elems(uint64_t L, uint32_t w, uint64_t j)
{
    const uint64_t q = delta_q(L, w), e0 = j << PLANES_LOG_E;
    return e0 >= q ? 0u : (q - e0 < PLANES_E ? (uint32_t)(q - e0) : PLANES_E);
}

// ---- a width and a filter per segment (bwts_delta_*_segments_f_device, the version-2 member frame) ----
// A segment without a filter is copied, whatever its width, in tiles of PLANES_COPY_T bytes (planes_copy_bytes says how many bytes
// tile j has): the LDS footprint of a filtered tile at the largest width serves every tile of a mixed call.
PLANES_HD uint64_t delta_tiles_f(uint64_t L, uint32_t w, uint32_t f)
{
    return f == DELTA_FILTER_NONE ? (L + PLANES_COPY_T - 1u) / PLANES_COPY_T : delta_tiles(L, w);
}
// first[s]: the first tile of segment s over the call, count + 1 entries; the total is first[count]
PLANES_HD uint64_t delta_cut_f(const uint64_t *off, const uint32_t *widths, const uint32_t *filters, uint64_t count, uint64_t *first)
{
    uint64_t tiles = 0;
    for (uint64_t s = 0; s < count; s++) {
        first[s] = tiles;
        tiles += delta_tiles_f(off[s + 1] - off[s], widths[s], filters[s]);
    }
    first[count] = tiles;
    return tiles;
}
// the word a segment's width and filter travel in, to the kernels and in a version-2 entry: width in bits 0-7, filter in bits 8-15
PLANES_HD uint32_t delta_word(uint32_t w, uint32_t f) { return w | (f << 8); }

// one element: a difference d (mod 2^{8w}) to its zigzag and back
PLANES_HD uint64_t delta_zigzag(uint64_t d, uint32_t w)
{
    return ((d << 1) ^ (0ull - ((d >> (8u * w - 1u)) & 1u))) & delta_mask(w);
}
PLANES_HD uint64_t delta_unzigzag(uint64_t z, uint32_t w)
{
    return ((z >> 1) ^ (0ull - (z & 1u))) & delta_mask(w);
}

// a little-endian element of w bytes at any address, byte by byte
PLANES_HD uint64_t delta_load(const uint8_t *p, uint32_t w)
{
    uint64_t v = 0;
    for (uint32_t k = 0; k < w; k++) v |= (uint64_t)p[k] << (8u * k);
    return v;
}
PLANES_HD void delta_store(uint8_t *p, uint32_t w, uint64_t v)
{
    for (uint32_t k = 0; k < w; k++) p[k] = (uint8_t)(v >> (8u * k));
}

// the serial statements.  Encode: z_i = zigzag(a_i - a_{i-1}), a_{-1} = 0; decode: a_i = the running sum of the un-zigzagged z_j;
// the tail is copied.  in and out do not overlap.
PLANES_HD void delta_encode_serial(const uint8_t *in, uint64_t L, uint32_t w, uint8_t *out)
{
    const uint64_t q = delta_q(L, w), m = delta_mask(w);
    uint64_t prev = 0;
    for (uint64_t i = 0; i < q; i++) {
        const uint64_t a = delta_load(in + i * w, w);
        delta_store(out + i * w, w, delta_zigzag((a - prev) & m, w));
        prev = a;
    }
    for (uint64_t i = q * w; i < L; i++) out[i] = in[i];
}
PLANES_HD void delta_decode_serial(const uint8_t *in, uint64_t L, uint32_t w, uint8_t *out)
{
    const uint64_t q = delta_q(L, w), m = delta_mask(w);
    uint64_t run = 0;
    for (uint64_t i = 0; i < q; i++) {
        run = (run + delta_unzigzag(delta_load(in + i * w, w), w)) & m;
        delta_store(out + i * w, w, run);
    }
    for (uint64_t i = q * w; i < L; i++) out[i] = in[i];
}
