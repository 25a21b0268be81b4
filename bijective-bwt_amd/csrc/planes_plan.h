// planes_plan.h -- the arithmetic of the byte-plane split (include/bwts_planes.h) that host and device share: which widths there
// are, how a string is cut into tiles, where its planes and its tail lie, and the serial statements of split and join.  Plain C++
// with no dependency, like zrl_plan.h: the kernels of planes.hip, the host side of the calls, pack_plan.h (the width word of a
// version-3 frame) and a stand-alone host program (tests/planes_plan_check.cc, built with the sanitizers) all compile this file.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PLANES_HD __host__ __device__ static inline
#else
#define PLANES_HD static inline
#endif

#define PLANES_LOG_E 12u                 // tile: E = 4096 elements of w bytes, 16 to a thread; T = E w bytes of the interleaved side
#define PLANES_E (1u << PLANES_LOG_E)
#define PLANES_MAX_W 8u
#define PLANES_MAX_N (1ull << 36)

PLANES_HD bool planes_width_ok(uint64_t w) { return w == 2u || w == 4u || w == 8u; }
PLANES_HD uint32_t planes_log_w(uint32_t w) { return w == 2u ? 1u : (w == 4u ? 2u : 3u); }
PLANES_HD uint64_t planes_tile_bytes(uint32_t w) { return (uint64_t)PLANES_E * w; }

// a string of L bytes at width w: q whole elements, then a tail of L - q w bytes that stays where it is
PLANES_HD uint64_t planes_q(uint64_t L, uint32_t w) { return L >> planes_log_w(w); }
PLANES_HD uint64_t planes_tail_at(uint64_t L, uint32_t w) { return planes_q(L, w) << planes_log_w(w); }
// Tiles of the string: ceil(L / T), so that stage_cut.h cuts a call with the unit T.  Tile j holds the elements [j E, min((j + 1) E, q)),
// none at all where q is a multiple of E and the tile is there for the tail alone; the last tile copies the tail.
PLANES_HD uint64_t planes_tiles(uint64_t L, uint32_t w) { return (L + planes_tile_bytes(w) - 1u) / planes_tile_bytes(w); }
PLANES_HD uint32_t planes_tile_elems(uint64_t L, uint32_t w, uint64_t j)
{
    const uint64_t q = planes_q(L, w), e0 = j << PLANES_LOG_E;
    return e0 >= q ? 0u : (q - e0 < PLANES_E ? (uint32_t)(q - e0) : PLANES_E);
}

// ---- a width per segment (bwts_planes_*_segments_w_device, the member frame of include/bwts_members.h) ----
// Width 1 joins the three: such a segment is copied.  Its tile is PLANES_COPY_T bytes, the interleaved side of a tile at the largest
// width, so that one LDS footprint (that of w = 8) serves every tile of a mixed call: 16 bytes to a thread, eight times over.
#define PLANES_COPY_T (PLANES_E * PLANES_MAX_W)
PLANES_HD bool planes_width_w_ok(uint64_t w) { return w == 1u || planes_width_ok(w); }
PLANES_HD uint64_t planes_tile_bytes_w(uint32_t w) { return w == 1u ? (uint64_t)PLANES_COPY_T : planes_tile_bytes(w); }
PLANES_HD uint64_t planes_tiles_w(uint64_t L, uint32_t w) { return (L + planes_tile_bytes_w(w) - 1u) / planes_tile_bytes_w(w); }
// the bytes of tile j of a copied segment
PLANES_HD uint32_t planes_copy_bytes(uint64_t L, uint64_t j)
{
    const uint64_t at = j * PLANES_COPY_T;
    return at >= L ? 0u : (L - at < PLANES_COPY_T ? (uint32_t)(L - at) : PLANES_COPY_T);
}
// first[s]: the first tile of segment s over the call, count + 1 entries (stage_cut.h's cut, with a unit per segment); the total is
// first[count]
PLANES_HD uint64_t planes_cut_w(const uint64_t *off, const uint32_t *widths, uint64_t count, uint64_t *first)
{
    uint64_t tiles = 0;
    for (uint64_t s = 0; s < count; s++) {
        first[s] = tiles;
        tiles += planes_tiles_w(off[s + 1] - off[s], widths[s]);
    }
    first[count] = tiles;
    return tiles;
}

// where byte i of the interleaved string lies in the split string
PLANES_HD uint64_t planes_split_index(uint64_t L, uint32_t w, uint64_t i)
{
    const uint64_t q = planes_q(L, w);
    return i >= planes_tail_at(L, w) ? i : (i & (w - 1u)) * q + (i >> planes_log_w(w));
}

// the serial statements: out[k q + i] = in[i w + k], the tail copied; the join is the inverse
PLANES_HD void planes_split_serial(const uint8_t *in, uint64_t L, uint32_t w, uint8_t *out)
{
    for (uint64_t i = 0; i < L; i++) out[planes_split_index(L, w, i)] = in[i];
}
PLANES_HD void planes_join_serial(const uint8_t *in, uint64_t L, uint32_t w, uint8_t *out)
{
    for (uint64_t i = 0; i < L; i++) out[i] = in[planes_split_index(L, w, i)];
}
