// pieces.hip -- copy_pieces_kernel: `count` pieces (src_off, dst_off, bytes) from one device buffer to another, at any alignment of
// either side of every piece (include/bwts_pack.h, "Ranges": it gathers the streams of covered blocks and cuts the ranges out of the
// decoded blocks).
//
// A piece is cut into tiles of PIECES_T bytes (pack_plan.h: the first one shorter, so that the later ones begin on a line of the
// destination), no tile across a piece; a workgroup of 256 threads takes tiles
// grid-stride and finds a tile's piece by bisecting the pieces' first tiles, as planes_tile does.  One stream per piece, so no LDS:
// the stores are the destination's -- single bytes up to the first 16-byte boundary of the tile (at most 15), aligned 16-byte stores
// behind them, each put together from the two aligned 16-byte source pieces around it by the funnel shift (load16.h), single bytes
// for what is left (at most 15).  No access wider than a byte is made at an address that is not a multiple of its width; nothing
// outside the source buffer is read (a tile whose aligned pieces would reach outside it, at the buffer's first or last bytes, is
// copied in single bytes); nothing outside a piece's destination bytes is written.
#include "internal.h"
#include "device_utils.h"
#include "load16.h"
#include "pack_plan.h"

// the pieces as the kernel sees them: four tables in the arena, or the one piece of a call that has no more (no table, no copy)
struct PiecesTable {
    const u64 *src, *dst, *bytes;       // [count]
    const u64 *first;                   // [count + 1] the piece's first tile, counted over the call
    u64 count, tiles;
    PackPiece one;
};

// planes_funnel for a shift that is the same in every lane (a tile has one): the five words the result is made of are chosen by a
// branch of the whole wave, not by selects in every lane
__device__ __forceinline__ uint4 pieces_funnel(uint4 a, uint4 b, u32 sh)
{
    const u32 bytes = sh & 3u;
    u32 D[5];
    switch (sh >> 2) {
    case 0: D[0] = a.x; D[1] = a.y; D[2] = a.z; D[3] = a.w; D[4] = b.x; break;
    case 1: D[0] = a.y; D[1] = a.z; D[2] = a.w; D[3] = b.x; D[4] = b.y; break;
    case 2: D[0] = a.z; D[1] = a.w; D[2] = b.x; D[3] = b.y; D[4] = b.z; break;
    default: D[0] = a.w; D[1] = b.x; D[2] = b.y; D[3] = b.z; D[4] = b.w; break;
    }
    return make_uint4(__builtin_amdgcn_alignbyte(D[1], D[0], bytes), __builtin_amdgcn_alignbyte(D[2], D[1], bytes),
                      __builtin_amdgcn_alignbyte(D[3], D[2], bytes), __builtin_amdgcn_alignbyte(D[4], D[3], bytes));
}

#define PIECES_GRID 8192u     // workgroups at most: four rounds of what the chip holds at 8 per CU; the rest of the tiles grid-stride

// The aligned stores of a tile: store v from the aligned source pieces v and, where the source is shifted against the destination,
// v + 1.  A thread has four 16-byte loads in flight before its first store: U stores' worth, of two loads each where SHIFT.
template <u32 U, bool SHIFT>
__device__ __forceinline__ void pieces_stores(const uint4 *__restrict__ av, uint4 *__restrict__ dv, u32 vecs, u32 sh)
{
    for (u32 v0 = threadIdx.x; v0 < vecs; v0 += 256u * U) {
        uint4 x[U], y[U];
#pragma unroll
        for (u32 k = 0; k < U; k++) {
            const u32 v = v0 + 256u * k;
            if (v < vecs) {
                x[k] = av[v];
                if (SHIFT) y[k] = av[v + 1u];
            }
        }
#pragma unroll
        for (u32 k = 0; k < U; k++) {
            const u32 v = v0 + 256u * k;
            if (v < vecs) dv[v] = SHIFT ? pieces_funnel(x[k], y[k], sh) : x[k];
        }
    }
}

__global__ __launch_bounds__(256, 8) void copy_pieces_kernel(const u8 *__restrict__ src, u64 src_bytes, PiecesTable P, u8 *__restrict__ dst)
{
    const u32 tid = threadIdx.x;
    for (u64 t = blockIdx.x; t < P.tiles; t += gridDim.x) {
        u64 first = 0;
        PackPiece p = P.one;
        if (P.count > 1) {
            // the piece of tile t: the last one whose first tile is not behind t (every piece has a tile, so the firsts differ)
            u64 lo = 0, hi = P.count;
            while (hi - lo > 1) {
                const u64 mid = lo + (hi - lo) / 2;
                if (P.first[mid] <= t) lo = mid;
                else hi = mid;
            }
            first = P.first[lo];
            p = PackPiece{P.src[lo], P.dst[lo], P.bytes[lo]};
        }
        // tile j of the piece: the first one ends where the destination's next line begins, T - lead bytes on
        const u64 j = t - first, f = pieces_first_bytes((uintptr_t)(dst + p.dst) & (PIECES_LINE - 1u));
        const u64 at = j ? f + ((j - 1u) << PIECES_LOG_T) : 0u, left = p.bytes - at, most = j ? (u64)PIECES_T : f;
        const u32 len = (u32)(left < most ? left : most);
        const u8 *s = src + p.src + at;
        u8 *d = dst + p.dst + at;
        u32 head = (16u - (u32)((uintptr_t)d & 15)) & 15u;
        if (head > len) head = len;
        const u32 vecs = (len - head) / 16u, done = head + 16u * vecs;
        // the single bytes at both ends: lanes 0 .. head - 1 and 16 .. 16 + (len - done) - 1, read first and written last, so that the
        // wait for them is not in front of the tile's loads
        const bool edge = tid < head || (tid >= 16u && tid - 16u < len - done);
        const u32 ei = tid < head ? tid : done + (tid - 16u);
        u8 eb = 0;
        if (edge) eb = s[ei];
        // store v holds the tile's bytes [head + 16 v, head + 16 v + 16): from the aligned source pieces v and v + 1 behind a
        const u32 sh = (u32)((uintptr_t)(s + head) & 15);
        const u8 *a = s + head - sh;
        uint4 *dv = (uint4 *)(d + head);
        if (a >= src && a + 16u * (vecs + (sh ? 1u : 0u)) <= src + src_bytes) {
            // every aligned piece the tile reads lies inside the source: plain loads, a batch of them in flight before the first store
            if (sh) pieces_stores<2, true>((const uint4 *)a, dv, vecs, sh);
            else pieces_stores<4, false>((const uint4 *)a, dv, vecs, 0);
        } else {
            // a tile at the source's first or last bytes, where an aligned piece would reach outside: two tiles of a call at most
            // (but for pieces that share those bytes), copied in single bytes
            for (u32 i = head + tid; i < done; i += 256) d[i] = s[i];
        }
        if (edge) d[ei] = eb;
    }
}

// The piece of tile t, as the bisection above finds it, by sections of 64: every lane of a wave reads one of 64 evenly spaced first
// tiles of the range, and a ballot says in which 64th t lies.  Two dependent reads for 4096 pieces where the bisection makes twelve: a
// workgroup has nothing else in flight while it looks for its tile's piece, and with a shifted source those reads showed in the time
// of the whole copy.  Every wave of the workgroup finds the same piece for itself; nothing is shared.
__device__ __forceinline__ u64 pieces_find(const u64 *__restrict__ first, u64 count, u64 t)
{
    const u32 lane = threadIdx.x & 63u;
    u64 lo = 0, hi = count;         // first[lo] <= t < first[hi]
    while (hi - lo > 1) {
        const u64 step = (hi - lo + 63u) >> 6;
        const u64 i = lo + lane * step;
        const bool below = i < hi && first[i] <= t;
        const u32 k = (u32)__popcll(__ballot(below));       // the lanes below are a prefix of the wave, lane 0 among them
        lo += (u64)(k - 1u) * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    return lo;
}

// scatter_pieces_kernel: the same copy between buffers of which every piece is one of its own (include/bwts_members.h, "Pointers";
// DESIGN section 23): P.src and P.dst hold absolute device addresses, and the readable bytes of a piece are its own and nothing
// else.  Tile cut and stores are those above; the tile's piece is found by pieces_find.  The guard of the aligned over-read is the piece's, not a buffer's, and it
// costs a store, not the tile (pack_plan.h, scatter_tile_plan): the first store of a tile where its lower aligned source piece begins
// in front of the piece, and the last one where its upper piece ends behind it, are made of single bytes by lanes 32 .. 63, which
// read and write them with the head and tail bytes of lanes 0 .. 31.  A tile that has bytes of its piece on both sides loses nothing.
__global__ __launch_bounds__(256, 8) void scatter_pieces_kernel(PiecesTable P)
{
    const u32 tid = threadIdx.x;
    for (u64 t = blockIdx.x; t < P.tiles; t += gridDim.x) {
        u64 first = 0;
        PackPiece p = P.one;
        if (P.count > 1) {
            const u64 lo = pieces_find(P.first, P.count, t);
            first = P.first[lo];
            p = PackPiece{P.src[lo], P.dst[lo], P.bytes[lo]};
        }
        u64 at = 0;
        const u32 len = pieces_tile_at(p.bytes, p.dst & (PIECES_LINE - 1u), t - first, &at);
        const ScatterTile k = scatter_tile_plan(p.src + at, p.dst + at, len, p.src, p.src + p.bytes);
        const u8 *s = (const u8 *)(uintptr_t)(p.src + at);
        u8 *d = (u8 *)(uintptr_t)(p.dst + at);
        // the single bytes: read first and written last, so that the wait for them is not in front of the tile's loads
        u32 ei = 0;
        const bool edge = tid < 64u && scatter_edge_byte(k, len, tid, &ei);
        u8 eb = 0;
        if (edge) eb = s[ei];
        const uint4 *av = (const uint4 *)(s + k.head - k.sh) + k.v_lo;
        uint4 *dv = (uint4 *)(d + k.head) + k.v_lo;
        if (k.sh) pieces_stores<2, true>(av, dv, k.v_hi - k.v_lo, k.sh);
        else pieces_stores<4, false>(av, dv, k.v_hi - k.v_lo, 0);
        if (edge) d[ei] = eb;
    }
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
// Every piece lies inside its buffer (the callers have seen to it: the plan of pack_plan.h, or the checks of bwts_debug_copy_pieces).
// The tables travel through the arena: a call may have 2^20 pieces, far more than the region behind a segment table of a few
// covered blocks holds.  The call drains the stream, so the host's tables may go when it returns.
int copy_pieces_impl(bwts_ctx *ctx, const u8 *d_src, u64 src_bytes, const PackPiece *pieces, u64 count, u8 *d_dst)
{
    std::vector<u64> h((size_t)(4 * count + 1));
    u64 *src = h.data(), *dst = src + count, *bytes = dst + count, *first = bytes + count;
    u64 tiles = 0, total = 0;
    for (u64 i = 0; i < count; i++) {
        src[i] = pieces[i].src; dst[i] = pieces[i].dst; bytes[i] = pieces[i].bytes;
        first[i] = tiles;
        tiles += pieces_tiles(pieces[i].bytes, (uintptr_t)(d_dst + pieces[i].dst) & (PIECES_LINE - 1u));
        total += pieces[i].bytes;
    }
    first[count] = tiles;
    PiecesTable P = {nullptr, nullptr, nullptr, nullptr, count, tiles, pieces[0]};
    if (count > 1) {
        // the four tables as one block, one copy
        u64 *d = nullptr;
        BlockLayout L;
        L.array(&d, h.size());
        BWTS_TRY(arena_take(ctx, L));
        HIPC(hipMemcpyAsync(d, h.data(), h.size() * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
        P.src = d; P.dst = d + count; P.bytes = d + 2 * count; P.first = d + 3 * count;
    }
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, total, 2 * total);
        copy_pieces_kernel<<<dim3((unsigned)(tiles < PIECES_GRID ? tiles : PIECES_GRID)), dim3(256), 0, ctx->stream>>>(d_src, src_bytes, P, d_dst);
    }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(ctx->stream));
    return BWTS_OK;
}

// The same for scatter_pieces_kernel: src and dst of a piece are absolute device addresses, every piece a buffer of its own (the
// callers have seen to it that no destination shares a byte with another or with a source: the checks of api.hip).
int scatter_pieces_impl(bwts_ctx *ctx, const PackPiece *pieces, u64 count)
{
    std::vector<u64> h((size_t)(4 * count + 1));
    u64 *src = h.data(), *dst = src + count, *bytes = dst + count, *first = bytes + count;
    u64 tiles = 0, total = 0;
    for (u64 i = 0; i < count; i++) {
        src[i] = pieces[i].src; dst[i] = pieces[i].dst; bytes[i] = pieces[i].bytes;
        first[i] = tiles;
        tiles += pieces_tiles(pieces[i].bytes, pieces[i].dst & (PIECES_LINE - 1u));
        total += pieces[i].bytes;
    }
    first[count] = tiles;
    PiecesTable P = {nullptr, nullptr, nullptr, nullptr, count, tiles, pieces[0]};
    if (count > 1) {
        u64 *d = nullptr;
        BlockLayout L;
        L.array(&d, h.size());
        BWTS_TRY(arena_take(ctx, L));
        HIPC(hipMemcpyAsync(d, h.data(), h.size() * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
        P.src = d; P.dst = d + count; P.bytes = d + 2 * count; P.first = d + 3 * count;
    }
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, total, 2 * total);
        scatter_pieces_kernel<<<dim3((unsigned)(tiles < PIECES_GRID ? tiles : PIECES_GRID)), dim3(256), 0, ctx->stream>>>(P);
    }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(ctx->stream));
    return BWTS_OK;
}
