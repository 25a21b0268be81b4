// planes.hip -- the byte-plane split of typed arrays and its inverse, the stage in front of the transform (include/bwts_planes.h; the
// definition is stated there and in DESIGN section 16, tests/planes_model.py is its executable form; the arithmetic shared with the
// host is in planes_plan.h).
//
// A streaming transpose: one read and one write of n bytes, no working memory.  A string is cut into tiles of E = 4096 elements of w
// bytes, no tile across a segment start; a workgroup of 256 threads works on one tile, every thread on 16 consecutive elements.
//   split: the thread takes its 16 w interleaved bytes as w 16-byte loads, regroups them with byte permutes into one 16-byte unit per
//          plane, and puts unit and plane into LDS; the tile's w plane pieces go out from there.
//   join:  the thread takes one 16-byte unit per plane, regroups them into its 16 w interleaved bytes and puts them into LDS; the
//          tile's interleaved bytes go out from there.
// Neither side of either direction is aligned but by luck (a plane starts at base + k q, a segment anywhere), and no access wider than
// a byte is ever made at an address that is not a multiple of its width:
//   reading  planes_load16 (load16.h) reads the two aligned 16-byte pieces around an address and shifts the bytes into place in registers; a
//            piece that does not lie inside the call's input is put together from the single bytes that do (the first and the last
//            piece of the whole input at most), so nothing outside the input is read.
//   writing  planes_stream_store (load16.h) sends a piece of len bytes from LDS: single bytes up to the destination's first 16-byte boundary (at
//            most 15), aligned 16-byte stores behind them, each shifted into place from two aligned LDS units, and single bytes for
//            what is left (at most 15).  At most 30 bytes of a piece of 4096 or more leave as single bytes.
// The tail of a string (its last L mod w bytes) is copied by the workgroup of its last tile.
#include "internal.h"
#include "device_utils.h"
#include "load16.h"
#include "planes_plan.h"
#include "../../include/bwts_planes.h"

#define PLANES_PLANE_SLOTS (PLANES_SLOT(PLANES_E / 16u) + 2u)           // a plane's piece of a split, and the unit behind it that a shift reads

// The segments of a call as the kernels see them.  off == null: one input of n bytes.
struct PlanesSegs {
    const u64 *off;         // [count + 1] where every segment starts
    const u64 *first;       // [count + 1] the segment's first tile, counted over the call
    u64 count, n;
};

struct PlanesTile {
    u64 seg, len, q, e0;    // the segment's start and length, its elements, the tile's first element
    u32 elems;              // the tile's elements (0: the tile is there for the tail alone)
    bool last;
};

// tile j of the string of len bytes at seg
template <int W>
__device__ __forceinline__ PlanesTile planes_tile_at(u64 seg, u64 len, u64 j)
{
    PlanesTile R;
    R.seg = seg; R.len = len;
    R.q = planes_q(R.len, W);
    R.e0 = j << PLANES_LOG_E;
    R.elems = planes_tile_elems(R.len, W, j);
    R.last = j + 1 == planes_tiles(R.len, W);
    return R;
}

template <int W>
__device__ __forceinline__ PlanesTile planes_tile(const PlanesSegs &S, u64 t)
{
    if (!S.off) return planes_tile_at<W>(0, S.n, t);
    const u64 lo = planes_tile_segment(S.first, S.count, t);
    return planes_tile_at<W>(S.off[lo], S.off[lo + 1] - S.off[lo], t - S.first[lo]);
}

// one word from byte ba of a, byte bb of b, byte bc of c and byte bd of d (constants after unrolling): three byte permutes
__device__ __forceinline__ u32 planes_pick4(u32 a, int ba, u32 b, int bb, u32 c, int bc, u32 d, int bd)
{
    const u32 lo = __builtin_amdgcn_perm(b, a, 0x0c0c0000u | (u32)ba | ((u32)(4 + bb) << 8));
    const u32 hi = __builtin_amdgcn_perm(d, c, 0x0c0c0000u | (u32)bc | ((u32)(4 + bd) << 8));
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}

// the tail of the tile's string: fewer than w bytes, copied
template <int W>
__device__ __forceinline__ void planes_copy_tail(const u8 *in, const PlanesTile &R, u8 *out)
{
    const u64 at = planes_tail_at(R.len, W);
    if (threadIdx.x < R.len - at) out[R.seg + at + threadIdx.x] = in[R.seg + at + threadIdx.x];
}

// one tile of a split; lds: W * PLANES_PLANE_SLOTS units; n: the bytes of the call's input
template <int W>
__device__ __forceinline__ void planes_split_tile(const u8 *__restrict__ in, u64 n, const PlanesTile &R, uint4 *lds, u8 *__restrict__ out)
{
    const u32 tid = threadIdx.x, at = 16u * tid;
    if (R.elems) {
        if (at < R.elems) {
            // (a tile's last thread may hold fewer than 16 elements: what it reads behind them lies in the input or reads as 0, and no
            // byte of it leaves the LDS)
            const u8 *p = in + R.seg + (R.e0 + at) * W;
            u32 D[4 * W];
#pragma unroll
            for (int v = 0; v < W; v++) {
                const uint4 x = planes_load16(p + 16 * v, in, in + n);
                D[4 * v] = x.x; D[4 * v + 1] = x.y; D[4 * v + 2] = x.z; D[4 * v + 3] = x.w;
            }
            // word j of plane k: byte k of the elements 4 j .. 4 j + 3
#pragma unroll
            for (int k = 0; k < W; k++) {
                u32 o[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int b0 = (4 * j) * W + k, b1 = b0 + W, b2 = b1 + W, b3 = b2 + W;
                    o[j] = planes_pick4(D[b0 >> 2], b0 & 3, D[b1 >> 2], b1 & 3, D[b2 >> 2], b2 & 3, D[b3 >> 2], b3 & 3);
                }
                lds[k * PLANES_PLANE_SLOTS + PLANES_SLOT(tid)] = make_uint4(o[0], o[1], o[2], o[3]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < W; k++) planes_stream_store(lds + k * PLANES_PLANE_SLOTS, out + R.seg + (u64)k * R.q + R.e0, R.elems);
    }
    if (R.last) planes_copy_tail<W>(in, R, out);
}

template <int W>
__global__ __launch_bounds__(256) void planes_split_kernel(const u8 *__restrict__ in, PlanesSegs S, u8 *__restrict__ out)
{
    __shared__ uint4 lds[W * PLANES_PLANE_SLOTS];
    planes_split_tile<W>(in, S.n, planes_tile<W>(S, blockIdx.x), lds, out);
}

#define PLANES_JOIN_SLOTS(w) (PLANES_SLOT((w) * (PLANES_E / 16u)) + 2u)

// one tile of a join; lds: PLANES_JOIN_SLOTS(W) units
template <int W>
__device__ __forceinline__ void planes_join_tile(const u8 *__restrict__ in, u64 n, const PlanesTile &R, uint4 *lds, u8 *__restrict__ out)
{
    const u32 tid = threadIdx.x, at = 16u * tid;
    if (R.elems) {
        if (at < R.elems) {
            const u8 *p = in + R.seg + R.e0 + at;
            u32 P[4 * W];
#pragma unroll
            for (int k = 0; k < W; k++) {
                const uint4 x = planes_load16(p + (u64)k * R.q, in, in + n);
                P[4 * k] = x.x; P[4 * k + 1] = x.y; P[4 * k + 2] = x.z; P[4 * k + 3] = x.w;
            }
            // interleaved byte b of the thread: byte b / w of plane b mod w
#pragma unroll
            for (int v = 0; v < W; v++) {
                u32 o[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int b0 = 16 * v + 4 * j, b1 = b0 + 1, b2 = b0 + 2, b3 = b0 + 3;
                    o[j] = planes_pick4(P[4 * (b0 % W) + ((b0 / W) >> 2)], (b0 / W) & 3, P[4 * (b1 % W) + ((b1 / W) >> 2)], (b1 / W) & 3,
                                        P[4 * (b2 % W) + ((b2 / W) >> 2)], (b2 / W) & 3, P[4 * (b3 % W) + ((b3 / W) >> 2)], (b3 / W) & 3);
                }
                lds[PLANES_SLOT((u32)W * tid + (u32)v)] = make_uint4(o[0], o[1], o[2], o[3]);
            }
        }
        __syncthreads();
        planes_stream_store(lds, out + R.seg + R.e0 * W, R.elems * W);
    }
    if (R.last) planes_copy_tail<W>(in, R, out);
}

template <int W>
__global__ __launch_bounds__(256) void planes_join_kernel(const u8 *__restrict__ in, PlanesSegs S, u8 *__restrict__ out)
{
    __shared__ uint4 lds[PLANES_JOIN_SLOTS(W)];
    planes_join_tile<W>(in, S.n, planes_tile<W>(S, blockIdx.x), lds, out);
}

// ---- a width per segment: one launch for all of them ----
// The segments of such a call: first and width lie behind the context's table, first[count + 1] and then one word per segment.
struct PlanesSegsW {
    const u64 *off, *first, *width;
    u64 count, n;
};

// LDS for the widest tile of either direction
#define PLANES_W_SLOTS (PLANES_MAX_W * PLANES_PLANE_SLOTS > PLANES_JOIN_SLOTS(PLANES_MAX_W) ? PLANES_MAX_W * PLANES_PLANE_SLOTS : PLANES_JOIN_SLOTS(PLANES_MAX_W))
static_assert(PLANES_JOIN_SLOTS(PLANES_MAX_W) >= PLANES_SLOT(PLANES_COPY_T / 16u) + 2u, "a copied tile fits the LDS of a join at the largest width");

template <bool JOIN>
__global__ __launch_bounds__(256) void planes_w_kernel(const u8 *__restrict__ in, PlanesSegsW S, u8 *__restrict__ out)
{
    __shared__ uint4 lds[PLANES_W_SLOTS];
    const u64 t = blockIdx.x, lo = planes_tile_segment(S.first, S.count, t);
    const u64 seg = S.off[lo], len = S.off[lo + 1] - seg, j = t - S.first[lo];
    // (the width is the same for the whole workgroup: one branch, taken together)
    switch ((u32)S.width[lo]) {
    case 1: planes_copy_tile(in, S.n, seg, len, j, lds, out); break;
    case 2: JOIN ? planes_join_tile<2>(in, S.n, planes_tile_at<2>(seg, len, j), lds, out) : planes_split_tile<2>(in, S.n, planes_tile_at<2>(seg, len, j), lds, out); break;
    case 4: JOIN ? planes_join_tile<4>(in, S.n, planes_tile_at<4>(seg, len, j), lds, out) : planes_split_tile<4>(in, S.n, planes_tile_at<4>(seg, len, j), lds, out); break;
    default: JOIN ? planes_join_tile<8>(in, S.n, planes_tile_at<8>(seg, len, j), lds, out) : planes_split_tile<8>(in, S.n, planes_tile_at<8>(seg, len, j), lds, out); break;
    }
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
void bwts_planes_plan(u64 n, u32 w, u64 out[4])
{
    out[0] = planes_tile_bytes(w); out[1] = planes_tiles(n, w); out[2] = planes_q(n, w); out[3] = n - planes_tail_at(n, w);
}

template <int W>
static void planes_launch(hipStream_t stream, bool join, unsigned grid, const u8 *d_in, const PlanesSegs &S, u8 *d_out)
{
    if (join) planes_join_kernel<W><<<dim3(grid), dim3(256), 0, stream>>>(d_in, S, d_out);
    else planes_split_kernel<W><<<dim3(grid), dim3(256), 0, stream>>>(d_in, S, d_out);
}

// one input of n bytes, or every segment of the context's table on its own
int planes_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u32 w, u8 *d_out, bool join, SegMode segs)
{
    if (!planes_width_ok(w)) return BWTS_E_ARG;
    const StageCut cut = stage_cut_call(ctx, segs, n, planes_tile_bytes(w));
    const u64 tiles = cut.units[0];
    if (tiles >= (1ull << 31)) return BWTS_E_RANGE;
    PlanesSegs S = {nullptr, nullptr, 0, n};
    if (segs.table()) {
        // behind the context's table: every segment's first tile and the total
        u64 *d_first = nullptr;
        BWTS_TRY(seg_upload_extra(ctx, cut.first[0].data(), cut.count + 1, &d_first));
        S.off = d_seg_off(ctx); S.first = d_first; S.count = cut.count;
    }
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, 2 * n);
        if (w == 2) planes_launch<2>(ctx->stream, join, (unsigned)tiles, d_in, S, d_out);
        else if (w == 4) planes_launch<4>(ctx->stream, join, (unsigned)tiles, d_in, S, d_out);
        else planes_launch<8>(ctx->stream, join, (unsigned)tiles, d_in, S, d_out);
    }
    HIPC(hipGetLastError());
    return BWTS_OK;
}

// every segment of the context's table at its own width (1: copied), in one launch; widths: one per segment, judged by the caller
int planes_w_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, const u32 *widths, u8 *d_out, bool join)
{
    const u64 count = ctx->seg_off.size() - 1;
    // behind the context's table: every segment's first tile and the total, then every segment's width
    std::vector<u64> words((size_t)(2 * count + 1));
    const u64 tiles = planes_cut_w(ctx->seg_off.data(), widths, count, words.data());
    if (tiles >= (1ull << 31)) return BWTS_E_RANGE;
    for (u64 s = 0; s < count; s++) words[(size_t)(count + 1 + s)] = widths[s];
    u64 *d_words = nullptr;
    BWTS_TRY(seg_upload_extra(ctx, words.data(), 2 * count + 1, &d_words));
    const PlanesSegsW S = {d_seg_off(ctx), d_words, d_words + count + 1, count, n};
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, 2 * n);
        if (join) planes_w_kernel<true><<<dim3((unsigned)tiles), dim3(256), 0, ctx->stream>>>(d_in, S, d_out);
        else planes_w_kernel<false><<<dim3((unsigned)tiles), dim3(256), 0, ctx->stream>>>(d_in, S, d_out);
    }
    HIPC(hipGetLastError());
    return BWTS_OK;
}
