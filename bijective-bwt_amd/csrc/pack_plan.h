// pack_plan.h -- the arithmetic of the packed frame (include/bwts_pack.h, versions 1 to 3) and of its checksum that host and device share:
// CRC-32 as polynomial arithmetic over GF(2), how an input is cut into blocks, the bound, and what makes a header and a directory
// valid.  Plain C++ with no dependency but ec_plan.h and planes_plan.h: crc.hip, pack.hip, the host side of the calls and a stand-alone host program
// (tests/pack_plan_check.cc, built with the sanitizers) all compile this file.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ec_plan.h"
#include "planes_plan.h"

#define PACK_MAGIC 0x5A545742u           // "BWTZ"
#define PACK_VERSION 1u
#define PACK_VERSION_2 2u                // zero-run coding between the ranks and the coder: a directory entry names the coded bytes too
#define PACK_VERSION_3 3u                // version 2 with the byte-plane split in front of the transform: an entry names the width too
#define PACK_HEADER_BYTES 32u
#define PACK_ENTRY_BYTES 16u
#define PACK_ENTRY_BYTES_V2 32u
#define PACK_MIN_BLOCK 4096u
#define PACK_MAX_N (1ull << 32)
#define PACK_LEAST_FRAME 48u             // header and one directory entry
// what the predicates answer (the values of BWTS_OK, BWTS_E_RANGE and BWTS_E_FORMAT; pack.hip asserts that they are)
#define PACK_OK 0
#define PACK_RANGE -5
#define PACK_FORMAT -8

// ---- CRC-32 (zlib, gzip, PNG): reflected polynomial, a register's bit 31 is the coefficient of x^0 ----
#define CRC_POLY 0xEDB88320u
#define CRC_ONE 0x80000000u              // the polynomial 1
#define CRC_MAX_N (1ull << 36)
#define CRC_LOG_T 16u                    // tile: T = 65536 bytes, one wave
#define CRC_T (1u << CRC_LOG_T)
#define CRC_G 256u                       // tiles whose values one wave folds at the second level
#define CRC_ROW 1024u                    // a lane owns 16 consecutive bytes of every row

EC_HD uint64_t crc_tiles(uint64_t n) { return (n + CRC_T - 1u) >> CRC_LOG_T; }
EC_HD uint64_t crc_groups(uint64_t tiles) { return (tiles + CRC_G - 1u) / CRC_G; }

EC_HD uint32_t crc_times_x(uint32_t a) { return (a >> 1) ^ ((a & 1u) ? CRC_POLY : 0u); }
// a / x mod P: P has the constant term 1, so x is invertible
EC_HD uint32_t crc_over_x(uint32_t a) { return (a & CRC_ONE) ? ((a ^ CRC_POLY) << 1) | 1u : a << 1; }
// a b mod P
EC_HD uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= (a & (CRC_ONE >> i)) ? b : 0u;
        b = crc_times_x(b);
    }
    return p;
}
// x^(8 bytes) mod P, by squaring
EC_HD uint32_t crc_xpow8(uint64_t bytes)
{
    uint32_t r = CRC_ONE, sq = CRC_ONE >> 8;
    for (; bytes; bytes >>= 1) {
        if (bytes & 1u) r = crc_mul(r, sq);
        sq = crc_mul(sq, sq);
    }
    return r;
}
// the register after one more byte
EC_HD uint32_t crc_step_byte(uint32_t r, uint32_t byte)
{
    r ^= byte;
    for (int i = 0; i < 8; i++) r = crc_times_x(r);
    return r;
}
// crc(A B) from crc(A), crc(B) and the length of B (both finished values: the initial and final terms cancel)
EC_HD uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc_mul(crc_a, crc_xpow8(len_b)) ^ crc_b; }
// the checksum of a few bytes on the host (header and directory): four bits at a time
EC_HD uint32_t crc32_bytes(const uint8_t *p, uint64_t len)
{
    uint32_t nib[16];
    for (uint32_t v = 0; v < 16; v++) {
        uint32_t r = v;
        for (int i = 0; i < 4; i++) r = crc_times_x(r);
        nib[v] = r;
    }
    uint32_t r = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < len; i++) {
        r ^= p[i];
        r = nib[r & 15u] ^ (r >> 4);
        r = nib[r & 15u] ^ (r >> 4);
    }
    return ~r;
}

// ---- the frame ----
EC_HD uint64_t pack_le64(const uint8_t *p) { return (uint64_t)ec_le32(p) | (uint64_t)ec_le32(p + 4) << 32; }
EC_HD void pack_put64(uint8_t *p, uint64_t v) { ec_put32(p, (uint32_t)v); ec_put32(p + 4, (uint32_t)(v >> 32)); }

// the block length a pack of n bytes stores for the caller's block_bytes; 0: bad arguments
EC_HD uint64_t pack_block_len(uint64_t n, uint64_t block_bytes)
{
    if (n == 0 || n > PACK_MAX_N) return 0;
    if (block_bytes == 0 || block_bytes >= n) return n;
    return block_bytes < PACK_MIN_BLOCK ? 0 : block_bytes;
}
EC_HD uint64_t pack_blocks(uint64_t n, uint64_t B) { return (n + B - 1u) / B; }
EC_HD uint64_t pack_block_at(uint64_t n, uint64_t B, uint64_t b) { return n - b * B < B ? n - b * B : B; }      // bytes of block b
EC_HD uint64_t pack_fixed_bytes(uint64_t nblk) { return PACK_HEADER_BYTES + (uint64_t)PACK_ENTRY_BYTES * nblk; }
// all blocks but the last are B long: the coder's bound and least size, summed over the blocks, behind header and directory
EC_HD uint64_t pack_bound_bytes(uint64_t n, uint64_t B)
{
    const uint64_t nblk = pack_blocks(n, B);
    return pack_fixed_bytes(nblk) + (nblk - 1u) * ec_bound_bytes(B) + ec_bound_bytes(n - (nblk - 1u) * B);
}
EC_HD uint64_t pack_least_bytes(uint64_t n, uint64_t B)
{
    const uint64_t nblk = pack_blocks(n, B);
    return pack_fixed_bytes(nblk) + (nblk - 1u) * ec_least_bytes(B) + ec_least_bytes(n - (nblk - 1u) * B);
}

// ---- version 2: the same header with version = 2, entries of 32 bytes, the coder's streams over the zero-run coded bytes ----
// ---- version 3: version 2 with version = 3 and the width of the split in the word at entry offset 12; bound and least size are version 2's ----
// what a frame may say ...
EC_HD bool pack_version_ok(uint32_t version) { return version == PACK_VERSION || version == PACK_VERSION_2 || version == PACK_VERSION_3; }
// ... and what the _v calls may be asked for: version 3 has calls of its own, which take the width
EC_HD bool pack_version_asked_ok(uint32_t version) { return version == PACK_VERSION || version == PACK_VERSION_2; }
EC_HD uint32_t pack_entry_bytes(uint32_t version) { return version == PACK_VERSION ? PACK_ENTRY_BYTES : PACK_ENTRY_BYTES_V2; }
// the word at entry offset 12: zero in versions 1 and 2, the width in version 3
EC_HD bool pack_width_word_ok(uint32_t version, uint32_t word) { return version == PACK_VERSION_3 ? planes_width_ok(word) : word == 0u; }
EC_HD uint64_t pack_fixed_bytes_v(uint32_t version, uint64_t nblk) { return PACK_HEADER_BYTES + (uint64_t)pack_entry_bytes(version) * nblk; }
// the zero-run stage never expands, and the coder's bound grows with its input: the version-1 streams' bound holds
EC_HD uint64_t pack_bound_bytes_v2(uint64_t n, uint64_t B)
{
    const uint64_t nblk = pack_blocks(n, B);
    return pack_bound_bytes(n, B) + (uint64_t)(PACK_ENTRY_BYTES_V2 - PACK_ENTRY_BYTES) * nblk;
}
// every block at least one coded byte
EC_HD uint64_t pack_least_bytes_v2(uint64_t n, uint64_t B)
{
    const uint64_t nblk = pack_blocks(n, B);
    return pack_fixed_bytes_v(PACK_VERSION_2, nblk) + nblk * ec_least_bytes(1u);
}
// either, by the version
EC_HD uint64_t pack_bound_bytes_of(uint32_t version, uint64_t n, uint64_t B) { return version == PACK_VERSION ? pack_bound_bytes(n, B) : pack_bound_bytes_v2(n, B); }
EC_HD uint64_t pack_least_bytes_of(uint32_t version, uint64_t n, uint64_t B) { return version == PACK_VERSION ? pack_least_bytes(n, B) : pack_least_bytes_v2(n, B); }

EC_HD void pack_entry_write(uint8_t e[16], uint64_t stream_bytes, uint32_t crc)
{
    pack_put64(e, stream_bytes); ec_put32(e + 8, crc); ec_put32(e + 12, 0u);
}
EC_HD void pack_entry_write_v2(uint8_t e[32], uint64_t stream_bytes, uint32_t crc, uint64_t coded_bytes)
{
    pack_entry_write(e, stream_bytes, crc);
    pack_put64(e + 16, coded_bytes); pack_put64(e + 24, 0u);
}
EC_HD void pack_entry_write_v3(uint8_t e[32], uint64_t stream_bytes, uint32_t crc, uint64_t coded_bytes, uint32_t width)
{
    pack_entry_write_v2(e, stream_bytes, crc, coded_bytes);
    ec_put32(e + 12, width);
}
// the header of a frame whose directory (nblk entries) is complete
EC_HD void pack_header_write_v(uint8_t h[32], uint32_t version, uint64_t n, uint64_t B, const uint8_t *dir)
{
    ec_put32(h, PACK_MAGIC); ec_put32(h + 4, version); pack_put64(h + 8, n); pack_put64(h + 16, B);
    ec_put32(h + 24, crc32_bytes(dir, (uint64_t)pack_entry_bytes(version) * pack_blocks(n, B)));
    ec_put32(h + 28, crc32_bytes(h, 28));
}
EC_HD void pack_header_write(uint8_t h[32], uint64_t n, uint64_t B, const uint8_t *dir) { pack_header_write_v(h, PACK_VERSION, n, B, dir); }

struct PackHeader { uint64_t n, B, nblk; uint32_t dir_crc, version, width; };      // width: 0 until the directory has been judged, and in versions 1 and 2

// The header of a frame of which in_bytes bytes are at hand (h: the first 32 of them, read only when in_bytes allows a frame at all).
// PACK_OK and *H, PACK_FORMAT, or PACK_RANGE for a sound header that names more than 2^32 bytes.
EC_HD int pack_header_check(const uint8_t *h, uint64_t in_bytes, PackHeader *H)
{
    if (in_bytes < PACK_LEAST_FRAME || (in_bytes & 15u)) return PACK_FORMAT;
    if (ec_le32(h) != PACK_MAGIC || !pack_version_ok(ec_le32(h + 4))) return PACK_FORMAT;
    if (ec_le32(h + 28) != crc32_bytes(h, 28)) return PACK_FORMAT;
    const uint64_t n = pack_le64(h + 8), B = pack_le64(h + 16);
    if (n == 0) return PACK_FORMAT;
    if (n > PACK_MAX_N) return PACK_RANGE;
    if (B == 0 || B > n || (B < PACK_MIN_BLOCK && B != n)) return PACK_FORMAT;
    H->n = n; H->B = B; H->nblk = pack_blocks(n, B); H->dir_crc = ec_le32(h + 24); H->version = ec_le32(h + 4); H->width = 0u;
    if (pack_fixed_bytes_v(H->version, H->nblk) > in_bytes) return PACK_FORMAT;      // (judged with the version's entry size, before the directory is read)
    return PACK_OK;
}

// The directory behind a header that passed (dir: H.nblk entries, which in_bytes holds).  exact: the frame must be all of in_bytes
// (an unpack), else it may end earlier (stepping through concatenated frames).  PACK_OK, *frame_bytes and H.width, or PACK_FORMAT.
EC_HD int pack_directory_check(const uint8_t *dir, PackHeader &H, uint64_t in_bytes, bool exact, uint64_t *frame_bytes)
{
    const uint64_t entry = pack_entry_bytes(H.version);
    if (crc32_bytes(dir, entry * H.nblk) != H.dir_crc) return PACK_FORMAT;
    const uint32_t width = ec_le32(dir + 12);       // (every entry must say what the first one says)
    uint64_t total = pack_fixed_bytes_v(H.version, H.nblk);
    for (uint64_t b = 0; b < H.nblk; b++) {
        const uint8_t *e = dir + entry * b;
        const uint64_t sb = pack_le64(e);
        uint64_t len = pack_block_at(H.n, H.B, b);
        if (ec_le32(e + 12) != width || !pack_width_word_ok(H.version, width) || (sb & 15u)) return PACK_FORMAT;
        if (H.version != PACK_VERSION) {
            // the stream is the coder's over the zero-run coded bytes: 1 <= coded_bytes <= the block's length
            const uint64_t coded = pack_le64(e + 16);
            if (pack_le64(e + 24) != 0u || coded == 0u || coded > len) return PACK_FORMAT;
            len = coded;
        }
        if (sb < ec_least_bytes(len) || sb > ec_bound_bytes(len)) return PACK_FORMAT;      // (so the sum cannot overflow)
        total += sb;
    }
    if (exact ? total != in_bytes : total > in_bytes) return PACK_FORMAT;
    *frame_bytes = total;
    H.width = width;
    return PACK_OK;
}

// ---- ranges: which blocks a list of byte ranges touches, and what is moved for them (bwts_unpack_ranges) ----
#include <vector>

#define PACK_ARG -1                      // (the values of BWTS_E_ARG and BWTS_E_SPACE; pack.hip asserts that they are)
#define PACK_SPACE -9
#define PACK_MAX_RANGES (1ull << 20)
#define PACK_MAX_RANGE_BYTES (1ull << 32)
// copy_pieces_kernel (pieces.hip) cuts a piece into tiles of T = 16 KiB, no tile across a piece: a workgroup of 256 threads makes four
// aligned 16-byte stores per thread and tile.  The first tile of a piece is shorter by `lead`, its destination address modulo
// PIECES_LINE, so that every later tile begins on such a boundary of the destination and no store of a wave straddles a line.
#define PIECES_LOG_T 14u
#define PIECES_T (1u << PIECES_LOG_T)
#define PIECES_LINE 256u
EC_HD uint64_t pieces_first_bytes(uint64_t lead) { return PIECES_T - lead; }
EC_HD uint64_t pieces_tiles(uint64_t bytes, uint64_t lead)
{
    const uint64_t f = pieces_first_bytes(lead);
    return bytes <= f ? 1u : 1u + ((bytes - f + PIECES_T - 1u) >> PIECES_LOG_T);
}

// tile j of a piece of `bytes` bytes whose destination begins `lead` bytes into a line: where it begins in the piece, and its bytes
EC_HD uint32_t pieces_tile_at(uint64_t bytes, uint64_t lead, uint64_t j, uint64_t *at)
{
    const uint64_t f = pieces_first_bytes(lead);
    *at = j ? f + ((j - 1u) << PIECES_LOG_T) : 0u;
    const uint64_t left = bytes - *at, most = j ? (uint64_t)PIECES_T : f;
    return (uint32_t)(left < most ? left : most);
}

// scatter_pieces_kernel (pieces.hip) copies between buffers of which every piece is one of its own: the readable bytes of a piece are
// [ps, pe) and nothing else.  A tile of len bytes at source address s and destination address d is stored as copy_pieces_kernel stores
// it: `head` single bytes up to the destination's next 16-byte boundary, `vecs` aligned 16-byte stores, single bytes for the rest.
// Store v is put together from the aligned 16-byte source pieces at a + 16 v and, where sh != 0, a + 16 v + 16, a = s + head - sh.
// Those pieces lie inside the tile's own piece for every store but, at most, the first (a < ps) and the last (a + 16 vecs + 16 > pe,
// with sh != 0): stores [v_lo, v_hi) are made from aligned pieces, stores [0, v_lo) and [v_hi, vecs) in single bytes, and
// v_lo <= 1, vecs - v_hi <= 1.  A tile inside its piece, with bytes of the piece on both sides, loses nothing.
struct ScatterTile { uint32_t head, vecs, sh, v_lo, v_hi; };
EC_HD ScatterTile scatter_tile_plan(uint64_t s, uint64_t d, uint32_t len, uint64_t ps, uint64_t pe)
{
    ScatterTile t;
    t.head = (16u - (uint32_t)(d & 15u)) & 15u;
    if (t.head > len) t.head = len;
    t.vecs = (len - t.head) / 16u;
    t.sh = (uint32_t)((s + t.head) & 15u);
    const uint64_t a = s + t.head - t.sh;
    t.v_lo = t.vecs && a < ps ? 1u : 0u;
    t.v_hi = t.vecs - (t.vecs && t.sh && a + 16u * ((uint64_t)t.vecs + 1u) > pe ? 1u : 0u);
    if (t.v_hi < t.v_lo) t.v_hi = t.v_lo;
    return t;
}
// The single bytes of such a tile, one per lane of the workgroup's first wave: lanes 0 .. 15 the head, 16 .. 31 what is left behind the
// last store, 32 .. 47 store 0 where it is below v_lo, 48 .. 63 store vecs - 1 where it is not below v_hi.  *i: the byte's place in the tile.
EC_HD bool scatter_edge_byte(const ScatterTile &t, uint32_t len, uint32_t lane, uint32_t *i)
{
    const uint32_t k = lane & 15u, done = t.head + 16u * t.vecs;
    switch (lane >> 4) {
    case 0: *i = k; return k < t.head;
    case 1: *i = done + k; return k < len - done;
    case 2: *i = t.head + k; return t.v_lo != 0u;
    case 3: *i = t.head + 16u * t.v_hi + k; return t.v_hi < t.vecs;
    default: return false;
    }
}

struct PackRange { uint64_t offset, bytes; };           // bwts_range: bytes [offset, offset + bytes) of the unpacked input
struct PackPiece { uint64_t src, dst, bytes; };         // bytes [src, src + bytes) of one buffer to [dst, dst + bytes) of another
struct PackRun { uint64_t first, blocks; };             // blocks [first, first + blocks) of the frame

// The ranges of a call against the n bytes of a judged frame: PACK_ARG, PACK_RANGE, PACK_SPACE in this order, else PACK_OK and *sum,
// the bytes of all ranges.  No sum can overflow: at most 2^20 ranges count, each of at most n <= 2^32 bytes.
static inline int pack_ranges_check(uint64_t n, const PackRange *r, uint64_t count, uint64_t out_cap, uint64_t *sum)
{
    if (!r || count == 0) return PACK_ARG;
    if (count > PACK_MAX_RANGES) return PACK_RANGE;
    for (uint64_t i = 0; i < count; i++)
        if (r[i].bytes == 0) return PACK_ARG;
    uint64_t total = 0;
    for (uint64_t i = 0; i < count; i++) {
        if (r[i].bytes > n || r[i].offset > n - r[i].bytes) return PACK_RANGE;      // (by subtraction: offset + bytes may wrap)
        total += r[i].bytes;
    }
    if (total > PACK_MAX_RANGE_BYTES) return PACK_RANGE;
    if (total > out_cap) return PACK_SPACE;
    *sum = total;
    return PACK_OK;
}

// What a call with these ranges decodes and moves (ranges_plan in members_plan.h fills it, for a frame of either magic).  The covered
// blocks are those a range touches, as sorted maximal runs; they are decoded into one buffer, block behind block in the frame's order
// (covered bytes in all), so every range is one piece of that buffer.
struct PackRangesPlan {
    std::vector<PackRun> runs;
    std::vector<PackPiece> streams;     // one per run: src in the frame, dst in the gathered streams
    std::vector<PackPiece> out;         // one per range: src in the covered-block buffer, dst in the call's output
    std::vector<uint64_t> blocks;       // the covered blocks, ascending
    uint64_t covered_bytes, stream_bytes, coded_bytes, out_bytes;
};
