// crc.hip -- CRC-32 (zlib's) of device bytes, the checksum of the packed frame (include/bwts_pack.h; the arithmetic shared with the
// host is in pack_plan.h, DESIGN section 14 has the derivation).
//
// A CRC is the remainder of the message polynomial times x^32 modulo P, so it is linear: the register after A B is the register
// after A times x^(8 |B|), plus the register after B.  That makes the checksum a reduction whose operator depends on lengths:
//   tiles   one wave takes a tile of CRC_T bytes (no tile crosses a segment start).  Lane l owns the 16-byte pieces l, l + 64, ... of
//           the tile, counted from the 16-byte boundary at or below the tile's start, so every whole piece is one aligned 16-byte
//           load whatever the alignment of the input; the first and the last piece, where the tile does not fill them, are put
//           together from single bytes with zeros around them.  A lane runs its own register over its pieces: slicing by 16 with
//           tables made for a distance of CRC_ROW bytes (table k: byte k of a piece followed by CRC_ROW - 1 - k zero bytes), so the
//           register of the row before is absorbed into the next piece like in the serial algorithm: 16 lookups per 16 bytes and
//           nothing else.  Leading zeros leave a register that started at 0 alone; what a lane's register is too far along at the
//           end (the zeros behind its last piece) is taken back by one multiplication with a negative power of x from a table.  The
//           lanes' registers add up (xor) to the tile's, and one more multiplication moves that to the end of the segment.
//   fold    a segment's value is then the plain xor of its tiles' values, folded by one wave per CRC_G tiles and one wave over those,
//           or by one wave per segment; the last fold adds the terms of the initial and final 0xFFFFFFFF.
// Tables: 16 x 256 words in LDS, entry v of table k at word 256 k + v.  One lookup instruction reads one table for all lanes, so the
// 32 banks see v mod 32: equal bytes broadcast, and move-to-front ranks -- most of them below 32 -- fall into different banks.
#include "internal.h"
#include "device_utils.h"
#include "pack_plan.h"

#include <string.h>

// the tables' words: first 16 x 256, the slicing tables
#define CRC_TAB_BACK 4096u               // 1024: x^(-8 m)
#define CRC_TAB_POW 5120u                // 5 x 256: x^(8 v 256^j)
#define CRC_TAB_WORDS 6400u

__device__ __attribute__((aligned(16))) u32 g_crc_tab[CRC_TAB_WORDS];

// once per context (the table belongs to the device: contexts of one device write the same words)
__global__ __launch_bounds__(256) void crc_tables_kernel()
{
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= CRC_TAB_WORDS) return;
    u32 r;
    if (i < CRC_TAB_BACK) {
        const u32 k = i >> 8;
        r = i & 255u;
        for (u32 s = 0; s < 8u * (CRC_ROW - k); s++) r = crc_times_x(r);
    } else if (i < CRC_TAB_POW) {
        r = CRC_ONE;
        for (u32 s = 0; s < 8u * (i - CRC_TAB_BACK); s++) r = crc_over_x(r);
    } else {
        const u32 j = (i - CRC_TAB_POW) >> 8;
        u32 sq = CRC_ONE >> 8;
        for (u32 s = 0; s < 8u * j; s++) sq = crc_mul(sq, sq);
        r = CRC_ONE;
        for (u32 v = i & 255u; v; v >>= 1) {
            if (v & 1u) r = crc_mul(r, sq);
            sq = crc_mul(sq, sq);
        }
    }
    g_crc_tab[i] = r;
}

// x^(8 bytes) mod P for a wave-uniform count below 2^40: five table factors, multiplied up over eight lanes
__device__ __forceinline__ u32 crc_xpow8_wave(u64 bytes, int lane)
{
    u32 f = lane < 5 ? g_crc_tab[CRC_TAB_POW + 256u * (u32)lane + (u32)((bytes >> (8 * lane)) & 255u)] : CRC_ONE;
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) f = crc_mul(f, (u32)__shfl_xor((int)f, d, 64));
    return (u32)__builtin_amdgcn_readfirstlane((int)f);
}

// one piece into a lane's register
__device__ __forceinline__ u32 crc_absorb(const u32 *__restrict__ slice, u32 st, uint4 q)
{
    const u32 w[4] = {q.x ^ st, q.y, q.z, q.w};
    u32 r = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) r ^= slice[256 * k + ((w[k >> 2] >> (8 * (k & 3))) & 255u)];
    return r;
}

// piece j of a tile whose bytes are base[lead .. total): whole pieces in one load, the others byte by byte with zeros around them
__device__ __forceinline__ uint4 crc_piece(const u8 *__restrict__ base, u32 j, u32 lead, u32 total)
{
    const u32 lo = 16u * j;
    if (lo >= lead && lo + 16u <= total) return *(const uint4 *)(base + lo);
    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
    for (u32 b = 0; b < 16; b++) {
        const u32 pos = lo + b;
        if (pos >= lead && pos < total) w[b >> 2] |= (u32)base[pos] << (8 * (b & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// tseg of a segmented call (unit_table_kernel): the segment's number over its tiles
struct CrcTileTable {
    const u64 *first_tile;
    u32 *tseg;
    __device__ u64 first(u64 s) const { return first_tile[s]; }
    __device__ u64 units(u64 s) const { return first_tile[s + 1] - first_tile[s]; }
    __device__ void store(u64 s, u64 first, u64, u64 j) const { tseg[first + j] = (u32)s; }
};

// every tile's register, moved to the end of its segment.  seg_off == null: one input of n bytes.  (Left alone the compiler takes 89
// VGPRs for the four pieces in flight and their lookups: five waves per SIMD; held to eight it needs 62 and no scratch.)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
void crc_tile_kernel(const u8 *__restrict__ in, const u64 *__restrict__ seg_off, const u64 *__restrict__ first, const u32 *__restrict__ tseg, u64 n,
                     u64 tiles, u32 *__restrict__ tilecrc)
{
    __shared__ __attribute__((aligned(16))) u32 slice[4096];
    for (u32 i = threadIdx.x; i < 1024; i += 256) ((uint4 *)slice)[i] = ((const uint4 *)g_crc_tab)[i];
    __syncthreads();
    const int lane = lane_id();
    const u64 w0 = (u64)blockIdx.x * 4 + (u64)__builtin_amdgcn_readfirstlane(wave_id());
    for (u64 t = w0; t < tiles; t += (u64)gridDim.x * 4) {
        u64 begin, seg_end;
        if (!seg_off) {
            begin = t << CRC_LOG_T;
            seg_end = n;
        } else {
            const u64 s = tseg[t];
            begin = seg_off[s] + ((t - first[s]) << CRC_LOG_T);
            seg_end = seg_off[s + 1];
        }
        const u64 end = begin + CRC_T < seg_end ? begin + CRC_T : seg_end;
        const u8 *p = in + begin;
        const u32 lead = (u32)((uintptr_t)p & 15);
        const u8 *base = p - lead;                             // (nothing below p is read)
        const u32 total = lead + (u32)(end - begin), np = (total + 15u) >> 4, z = 16u * np - total;
        const u32 rw = (total >> 4) >> 6;                      // rows 0 .. rw - 1 hold only pieces that end inside the tile
        u32 st = 0, r = 0;
        if (lead) {
            if ((u32)lane < np) st = crc_absorb(slice, st, crc_piece(base, (u32)lane, lead, total));
            r = 1;
        }
        for (; r + 4 <= rw; r += 4) {
            const uint4 *row = (const uint4 *)base + 64u * r + (u32)lane;
            const uint4 q0 = row[0], q1 = row[64], q2 = row[128], q3 = row[192];
            st = crc_absorb(slice, st, q0);
            st = crc_absorb(slice, st, q1);
            st = crc_absorb(slice, st, q2);
            st = crc_absorb(slice, st, q3);
        }
        for (; r < rw; r++) st = crc_absorb(slice, st, ((const uint4 *)base)[64u * r + (u32)lane]);
        for (; 64u * r < np; r++) {
            const u32 j = 64u * r + (u32)lane;
            if (j < np) st = crc_absorb(slice, st, crc_piece(base, j, lead, total));
        }
        // a lane's register stands CRC_ROW bytes behind the start of its last piece: back to the tile's end
        const bool any = (u32)lane < np;
        const u32 last = any ? (u32)lane + 64u * ((np - 1u - (u32)lane) >> 6) : 0u;
        const u32 back = any ? 16u * last + CRC_ROW - 16u * np + z : 0u;
        u32 v = crc_mul(st, g_crc_tab[CRC_TAB_BACK + back]);
        v = wave_reduce(any ? v : 0u, OpXor());
        const u64 behind = seg_end - end;
        if (behind) v = crc_mul(v, crc_xpow8_wave(behind, lane));
        if (lane == 0) tilecrc[t] = v;
    }
}

// out[r] = xor of vals over range r: [first[r], first[r + 1]), or without a table [r stride, (r + 1) stride) below count_vals.
// finish: the ranges are whole segments (seg_off == null: the one input of n bytes) and get the initial and final terms.
__global__ __launch_bounds__(256) void crc_fold_kernel(const u32 *__restrict__ vals, u64 count_vals, const u64 *__restrict__ first, u64 stride, u64 ranges,
                                                       const u64 *__restrict__ seg_off, u64 n, int finish, u32 *__restrict__ out)
{
    const int lane = lane_id();
    const u64 w0 = (u64)blockIdx.x * 4 + (u64)__builtin_amdgcn_readfirstlane(wave_id());
    for (u64 r = w0; r < ranges; r += (u64)gridDim.x * 4) {
        const u64 a = first ? first[r] : r * stride;
        u64 b = first ? first[r + 1] : a + stride;
        if (b > count_vals) b = count_vals;
        u32 x = 0;
        for (u64 i = a + (u64)lane; i < b; i += 64) x ^= vals[i];
        x = wave_reduce(x, OpXor());
        if (finish) {
            const u64 len = seg_off ? seg_off[r + 1] - seg_off[r] : n;
            x ^= crc_mul(0xFFFFFFFFu, crc_xpow8_wave(len, lane)) ^ 0xFFFFFFFFu;
        }
        if (lane == 0) out[r] = x;
    }
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
void bwts_crc_plan(u64 n, u64 out[4])
{
    const u64 tiles = stage_cut_single(n, CRC_T).units[0];
    out[0] = CRC_T; out[1] = CRC_G; out[2] = tiles; out[3] = crc_groups(tiles);
}

struct CrcBufs {
    u32 *tilecrc, *gvals, *tseg, *out;
    void declare(BlockLayout &L, u64 tiles, u64 count, bool segments)
    {
        L.array(&tilecrc, tiles); L.array(&gvals, crc_groups(tiles)); L.array(&out, count);
        if (segments) L.array(&tseg, tiles);
        else tseg = nullptr;
    }
};

// crcs: one word (one input of n bytes) or one per segment of the context's table, on the host
int crc_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, SegMode segs, u32 *crcs)
{
    const StageCut cut = stage_cut_call(ctx, segs, n, CRC_T);
    const u64 count = cut.count, tiles = cut.units[0];
    const bool segments = segs.table();
    CrcBufs b;
    BlockLayout L;
    b.declare(L, tiles, count, segments);
    BWTS_TRY(arena_take(ctx, L));
    if (!ctx->crc_tables) {
        SpanGuard sp(ctx, BWTS_K_OTHER, CRC_TAB_WORDS, 4 * CRC_TAB_WORDS);
        crc_tables_kernel<<<dim3((CRC_TAB_WORDS + 255) / 256), dim3(256), 0, ctx->stream>>>();
        ctx->crc_tables = true;
    }
    const u64 *d_first = nullptr;
    if (segments) {
        u64 *d_words = nullptr;
        BWTS_TRY(seg_upload_extra(ctx, cut.first[0].data(), count + 1, &d_words));
        d_first = d_words;
        SpanGuard sp(ctx, BWTS_K_OTHER, tiles, 4 * tiles);
        unit_table_launch(ctx->stream, count, CrcTileTable{d_first, b.tseg});
    }
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, n);
        crc_tile_kernel<<<dim3(wave_grid(tiles)), dim3(256), 0, ctx->stream>>>(d_in, segments ? d_seg_off(ctx) : nullptr, d_first, b.tseg, n, tiles, b.tilecrc);
    }
    if (segments) {
        SpanGuard sp(ctx, BWTS_K_OTHER, tiles, 4 * tiles + 4 * count);
        crc_fold_kernel<<<dim3(wave_grid(count)), dim3(256), 0, ctx->stream>>>(b.tilecrc, tiles, d_first, 0, count, d_seg_off(ctx), n, 1, b.out);
    } else {
        const u32 *vals = b.tilecrc;
        u64 nvals = tiles;
        if (tiles > CRC_G) {
            SpanGuard sp(ctx, BWTS_K_OTHER, tiles, 4 * tiles);
            nvals = crc_groups(tiles);
            crc_fold_kernel<<<dim3(wave_grid(nvals)), dim3(256), 0, ctx->stream>>>(b.tilecrc, tiles, nullptr, CRC_G, nvals, nullptr, n, 0, b.gvals);
            vals = b.gvals;
        }
        SpanGuard sp(ctx, BWTS_K_OTHER, nvals, 4 * nvals);
        crc_fold_kernel<<<dim3(1), dim3(256), 0, ctx->stream>>>(vals, nvals, nullptr, nvals, 1, nullptr, n, 1, b.out);
    }
    HIPC(hipGetLastError());
    // the values come back through pinned memory: the small block, or for segments the read-back region behind the segment table,
    // which begins where the upload of the cut's first tiles ends (seg_layout.h)
    u32 *h = (u32 *)(ctx->h_small + SM_CRC_OUT);
    if (segments) BWTS_TRY(seg_pinned_region(ctx, seg_readback_at(count), seg_readback_words(count), (void **)&h));
    HIPC(hipMemcpyAsync(h, b.out, count * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    memcpy(crcs, h, count * sizeof(u32));
    return BWTS_OK;
}
