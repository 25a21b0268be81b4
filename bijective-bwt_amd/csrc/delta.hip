// delta.hip -- the delta filter of integer arrays and its inverse, a stage in front of the byte-plane split (include/bwts_delta.h; the
// definition is stated there and in DESIGN section 19, tests/delta_model.py is its executable form; the arithmetic shared with the
// host is in delta_plan.h).
//
// A string is cut into tiles of E = 4096 elements of w bytes, no tile across a segment start; a workgroup of 256 threads works on one
// tile, every thread on 16 consecutive elements, which it takes as w 16-byte loads and leaves as w 16-byte units in LDS.
//   encode: one streaming kernel, one read and one write.  The element in front of a thread's first comes from the lane below; the
//           first lane of a wave reads it from memory, byte by byte (four threads of a tile do).
//   decode: an inclusive prefix sum per segment, in two sweeps and a scan of the tile sums, so that no workgroup waits for another:
//           1. delta_reduce: one u64 per tile, the sum of its un-zigzagged differences (read striped: a sum has no order);
//           2. scan_templ.h's exclusive scan over the tile sums of the whole call, in place;
//           3. delta_final: every thread sums its 16 elements in registers, the threads' sums are scanned across the waves, the
//              tile's carry is added and the elements go out.
//           Addition mod 2^64 is a group: the carry of tile t is scanned[t] - scanned[first tile of its segment], taken mod 2^{8w}.
//           The scan stays plain addition, and what a copied segment's tiles put into it (zeros) cancels.
// A thread's elements in registers (the word they are worked on in, element i of the loaded words, the zigzag at a constant width) are
// in delta_words.h, which estimate.hip shares.
// Reading and writing follow planes.hip (load16.h): planes_load16 reads the two aligned 16-byte pieces around an address, and nothing
// outside the call's input; planes_stream_store sends a tile from LDS with aligned 16-byte stores and at most 30 single bytes.  No
// access wider than a byte is made at an address that is not a multiple of its width.
// A segment without a filter is copied in tiles of PLANES_COPY_T bytes, by planes.hip's copy tile.
// Working memory: 8 bytes per tile in the context's arena for a decode (and the scan's upper levels); none for an encode.
#include "internal.h"
#include "device_utils.h"
#include "load16.h"
#include "scan_templ.h"
#include "delta_plan.h"
#include "delta_words.h"
#include "../../include/bwts_delta.h"

static_assert(DELTA_FILTER_NONE == BWTS_FILTER_NONE && DELTA_FILTER_DELTA == BWTS_FILTER_DELTA, "delta_plan.h names the header's filters");

// LDS units of a tile at width w (the interleaved side of a join at that width), and of the widest tile of a mixed call, copied ones included
#define DELTA_SLOTS(w) (PLANES_SLOT((w) * (PLANES_E / 16u)) + 2u)
static_assert(DELTA_SLOTS(PLANES_MAX_W) >= PLANES_SLOT(PLANES_COPY_T / 16u) + 2u, "a copied tile fits the LDS of a tile at the largest width");

struct DeltaTile {
    u64 seg, len, e0;       // the segment's start and length, the tile's first element
    u32 elems;              // the tile's elements (0: the tile is there for the tail alone)
    bool last;
};

// tile j of the string of len bytes at seg
template <int W>
__device__ __forceinline__ DeltaTile delta_tile_at(u64 seg, u64 len, u64 j)
{
    DeltaTile R;
    R.seg = seg; R.len = len;
    R.e0 = j << PLANES_LOG_E;
    R.elems = delta_tile_elems(len, W, j);
    R.last = j + 1 == delta_tiles(len, W);
    return R;
}

// the tail of the tile's string: fewer than w bytes, copied
template <int W>
__device__ __forceinline__ void delta_copy_tail(const u8 *in, const DeltaTile &R, u8 *out)
{
    const u64 at = delta_tail_at(R.len, W);
    if (threadIdx.x < R.len - at) out[R.seg + at + threadIdx.x] = in[R.seg + at + threadIdx.x];
}

// the thread's 16 elements: W 16-byte loads (a tile's last thread may hold fewer than 16: what it reads behind them lies in the input
// or reads as 0, and no byte made of it leaves the LDS)
template <int W>
__device__ __forceinline__ void delta_load_thread(const u8 *__restrict__ in, u64 n, const DeltaTile &R, u32 at, u32 *D)
{
    delta_load16<W>(in + R.seg + (R.e0 + at) * W, in, n, D);
}

// the thread's 16 elements into the tile's stream in LDS
template <int W>
__device__ __forceinline__ void delta_store_thread(uint4 *lds, u32 tid, const u32 *O)
{
#pragma unroll
    for (int v = 0; v < W; v++) lds[PLANES_SLOT((u32)W * tid + (u32)v)] = make_uint4(O[4 * v], O[4 * v + 1], O[4 * v + 2], O[4 * v + 3]);
}

// one tile of an encode; lds: DELTA_SLOTS(W) units; n: the bytes of the call's input
template <int W>
__device__ __forceinline__ void delta_encode_tile(const u8 *__restrict__ in, u64 n, const DeltaTile &R, uint4 *lds, u8 *__restrict__ out)
{
    typedef typename DeltaWord<W>::T T;
    const u32 tid = threadIdx.x, at = 16u * tid;
    if (R.elems) {
        if (at < R.elems) {
            u32 D[4 * W], O[4 * W];
            delta_load_thread<W>(in, n, R, at, D);
            // the element in front of the thread's first: the last one of the lane below (whose `at` is smaller: it is here too); a
            // wave's first lane reads it from memory, and the string's first element has 0 in front of it
            T prev = shfl_up_t(delta_get<W>(D, 15), 1);
            if (lane_id() == 0) {
                prev = 0;
                if (R.e0 + at) {
                    const u8 *p = in + R.seg + (R.e0 + at) * W - W;
#pragma unroll
                    for (int k = 0; k < W; k++) prev |= (T)p[k] << (8 * k);
                }
            }
#pragma unroll
            for (int j = 0; j < 4 * W; j++) O[j] = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const T a = delta_get<W>(D, i);
                delta_put<W>(O, i, delta_zig<W>((T)(a - prev) & delta_mask_t<W>()));
                prev = a;
            }
            delta_store_thread<W>(lds, tid, O);
        }
        __syncthreads();
        planes_stream_store(lds, out + R.seg + R.e0 * W, R.elems * W);
    }
    if (R.last) delta_copy_tail<W>(in, R, out);
}

// the sum of one tile's un-zigzagged differences, in every thread; sm: 4 words.  The tile's 16-byte units are read striped (unit
// 256 v + tid): a sum has no order, and the lanes' loads lie side by side.
template <int W>
__device__ __forceinline__ u64 delta_reduce_tile(const u8 *__restrict__ in, u64 n, const DeltaTile &R, u64 *sm)
{
    typedef typename DeltaWord<W>::T T;
    const u32 per = 16u / W;            // elements to a unit
    const u8 *p = in + R.seg + R.e0 * W;
    T sum = 0;
#pragma unroll
    for (int v = 0; v < W; v++) {
        const u32 u = 256u * (u32)v + threadIdx.x, e = u * per;
        if (e < R.elems) {
            const uint4 x = planes_load16(p + 16u * u, in, in + n);
            const u32 X[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int k = 0; k < (int)per; k++)
                if (e + (u32)k < R.elems) sum += delta_unzig<W>(delta_get<W>(X, k));
        }
    }
    T tot;
    block_scan_exclusive<T, OpAdd, 4>(sum, OpAdd(), (T)0, (T *)sm, &tot);
    return (u64)tot;
}

// one tile of a decode's last sweep; carry: the sum of the segment's elements in front of the tile (any bits above 8 W are dropped);
// lds: DELTA_SLOTS(W) units, sm: 4 words
template <int W>
__device__ __forceinline__ void delta_final_tile(const u8 *__restrict__ in, u64 n, const DeltaTile &R, u64 carry, uint4 *lds, u64 *sm, u8 *__restrict__ out)
{
    typedef typename DeltaWord<W>::T T;
    const u32 tid = threadIdx.x, at = 16u * tid;
    if (R.elems) {
        // (every thread takes part in the scan: one that holds no element adds 0, and one that holds fewer than 16 stands behind
        // every thread whose elements are written)
        T v[16], run = 0;
        if (at < R.elems) {
            u32 D[4 * W];
            delta_load_thread<W>(in, n, R, at, D);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                run += delta_unzig<W>(delta_get<W>(D, i));
                v[i] = run;
            }
        }
        T tot;
        const T base = (T)carry + block_scan_exclusive<T, OpAdd, 4>(run, OpAdd(), (T)0, (T *)sm, &tot);
        if (at < R.elems) {
            u32 O[4 * W];
#pragma unroll
            for (int j = 0; j < 4 * W; j++) O[j] = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) delta_put<W>(O, i, (T)(v[i] + base) & delta_mask_t<W>());
            delta_store_thread<W>(lds, tid, O);
        }
        __syncthreads();
        planes_stream_store(lds, out + R.seg + R.e0 * W, R.elems * W);
    }
    if (R.last) delta_copy_tail<W>(in, R, out);
}

enum { DELTA_ENCODE = 0, DELTA_REDUCE = 1, DELTA_FINAL = 2 };

// one sweep over tile `j` of a filtered string (tile t of the call, the string's first tile being t - j); sums: the call's tile
// sums, written by the reduce sweep and read, scanned, by the final one
template <int W, int SWEEP>
__device__ __forceinline__ void delta_sweep_tile(const u8 *__restrict__ in, u64 n, u64 seg, u64 len, u64 t, u64 j, u64 *sums, uint4 *lds, u64 *sm,
                                                 u8 *__restrict__ out)
{
    const DeltaTile R = delta_tile_at<W>(seg, len, j);
    if (SWEEP == DELTA_ENCODE) delta_encode_tile<W>(in, n, R, lds, out);
    else if (SWEEP == DELTA_REDUCE) {
        const u64 tot = delta_reduce_tile<W>(in, n, R, sm);
        if (threadIdx.x == 0) sums[t] = tot;
    } else delta_final_tile<W>(in, n, R, sums[t] - sums[t - j], lds, sm, out);
}

// one input of n bytes at width W
template <int W, int SWEEP>
__global__ __launch_bounds__(256) void delta_kernel(const u8 *__restrict__ in, u64 n, u64 *sums, u8 *__restrict__ out)
{
    __shared__ uint4 lds[SWEEP == DELTA_REDUCE ? 1 : DELTA_SLOTS(W)];
    __shared__ u64 sm[4];
    delta_sweep_tile<W, SWEEP>(in, n, 0, n, blockIdx.x, blockIdx.x, sums, lds, sm, out);
}

// ---- a width and a filter per segment: one launch per sweep for all of them ----
// The segments of such a call: first and wf lie behind the context's table, first[count + 1] and then one word per segment
// (delta_word: the width, and the filter above it).
struct DeltaSegsF {
    const u64 *off, *first, *wf;
    u64 count, n;
};

template <int SWEEP>
__global__ __launch_bounds__(256) void delta_f_kernel(const u8 *__restrict__ in, DeltaSegsF S, u64 *sums, u8 *__restrict__ out)
{
    __shared__ uint4 lds[SWEEP == DELTA_REDUCE ? 1 : DELTA_SLOTS(PLANES_MAX_W)];
    __shared__ u64 sm[4];
    const u64 t = blockIdx.x, lo = planes_tile_segment(S.first, S.count, t);
    const u64 seg = S.off[lo], len = S.off[lo + 1] - seg, j = t - S.first[lo];
    const u32 wf = (u32)S.wf[lo];
    // (width and filter are the same for the whole workgroup: one branch, taken together)
    if ((wf >> 8) == DELTA_FILTER_NONE) {
        if (SWEEP != DELTA_REDUCE) planes_copy_tile(in, S.n, seg, len, j, lds, out);
        else if (threadIdx.x == 0) sums[t] = 0;
        return;
    }
    switch (wf & 0xffu) {
    case 1: delta_sweep_tile<1, SWEEP>(in, S.n, seg, len, t, j, sums, lds, sm, out); break;
    case 2: delta_sweep_tile<2, SWEEP>(in, S.n, seg, len, t, j, sums, lds, sm, out); break;
    case 4: delta_sweep_tile<4, SWEEP>(in, S.n, seg, len, t, j, sums, lds, sm, out); break;
    default: delta_sweep_tile<8, SWEEP>(in, S.n, seg, len, t, j, sums, lds, sm, out); break;
    }
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
// the tile sums of a decode of `tiles` tiles, and behind them the scan's upper levels where one workgroup does not take them all
static size_t delta_sums_bytes(u64 tiles)
{
    return align_up((size_t)(tiles + 1) * sizeof(u64), 256) + (tiles > SCAN_SINGLE_BLOCK_MAX ? scan_temp_bytes_t(tiles, sizeof(u64)) : 0);
}

static int delta_sums_take(bwts_ctx *ctx, u64 tiles, u64 **sums)
{
    BlockLayout L;
    L.raw(sums, delta_sums_bytes(tiles));
    return arena_take(ctx, L);
}

static int delta_sums_scan(bwts_ctx *ctx, u64 tiles, u64 *sums)
{
    SpanGuard sp(ctx, BWTS_K_OTHER, tiles, 16 * tiles);
    return device_scan_partials<u64, OpAdd>(ctx, tiles, OpAdd(), (u64)0, sums);
}

template <int W>
static void delta_launch(hipStream_t stream, int sweep, unsigned grid, const u8 *d_in, u64 n, u64 *sums, u8 *d_out)
{
    if (sweep == DELTA_ENCODE) delta_kernel<W, DELTA_ENCODE><<<dim3(grid), dim3(256), 0, stream>>>(d_in, n, sums, d_out);
    else if (sweep == DELTA_REDUCE) delta_kernel<W, DELTA_REDUCE><<<dim3(grid), dim3(256), 0, stream>>>(d_in, n, sums, d_out);
    else delta_kernel<W, DELTA_FINAL><<<dim3(grid), dim3(256), 0, stream>>>(d_in, n, sums, d_out);
}

static void delta_launch_w(hipStream_t stream, u32 w, int sweep, unsigned grid, const u8 *d_in, u64 n, u64 *sums, u8 *d_out)
{
    if (w == 1) delta_launch<1>(stream, sweep, grid, d_in, n, sums, d_out);
    else if (w == 2) delta_launch<2>(stream, sweep, grid, d_in, n, sums, d_out);
    else if (w == 4) delta_launch<4>(stream, sweep, grid, d_in, n, sums, d_out);
    else delta_launch<8>(stream, sweep, grid, d_in, n, sums, d_out);
}

// one input of n bytes
int delta_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u32 w, u8 *d_out, bool decode)
{
    if (!delta_width_ok(w)) return BWTS_E_ARG;
    const u64 tiles = delta_tiles(n, w);
    if (tiles >= (1ull << 31)) return BWTS_E_RANGE;
    if (!decode) {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, 2 * n);
        delta_launch_w(ctx->stream, w, DELTA_ENCODE, (unsigned)tiles, d_in, n, nullptr, d_out);
    } else {
        u64 *sums = nullptr;
        BWTS_TRY(delta_sums_take(ctx, tiles, &sums));
        {
            SpanGuard sp(ctx, BWTS_K_OTHER, n, n);
            delta_launch_w(ctx->stream, w, DELTA_REDUCE, (unsigned)tiles, d_in, n, sums, d_out);
        }
        BWTS_TRY(delta_sums_scan(ctx, tiles, sums));
        SpanGuard sp(ctx, BWTS_K_OTHER, n, 2 * n);
        delta_launch_w(ctx->stream, w, DELTA_FINAL, (unsigned)tiles, d_in, n, sums, d_out);
    }
    HIPC(hipGetLastError());
    return BWTS_OK;
}

// every segment of the context's table at its own width and filter (none: copied), one launch per sweep; widths and filters: one per
// segment, judged by the caller
int delta_f_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, const u32 *widths, const u32 *filters, u8 *d_out, bool decode)
{
    const u64 count = ctx->seg_off.size() - 1;
    // behind the context's table: every segment's first tile and the total, then every segment's width and filter
    std::vector<u64> words((size_t)(2 * count + 1));
    const u64 tiles = delta_cut_f(ctx->seg_off.data(), widths, filters, count, words.data());
    if (tiles >= (1ull << 31)) return BWTS_E_RANGE;
    for (u64 s = 0; s < count; s++) words[(size_t)(count + 1 + s)] = delta_word(widths[s], filters[s]);
    u64 *d_words = nullptr, *sums = nullptr;
    BWTS_TRY(seg_upload_extra(ctx, words.data(), 2 * count + 1, &d_words));
    const DeltaSegsF S = {d_seg_off(ctx), d_words, d_words + count + 1, count, n};
    const dim3 grid((unsigned)tiles), block(256);
    if (!decode) {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, 2 * n);
        delta_f_kernel<DELTA_ENCODE><<<grid, block, 0, ctx->stream>>>(d_in, S, sums, d_out);
    } else {
        BWTS_TRY(delta_sums_take(ctx, tiles, &sums));
        {
            SpanGuard sp(ctx, BWTS_K_OTHER, n, n);
            delta_f_kernel<DELTA_REDUCE><<<grid, block, 0, ctx->stream>>>(d_in, S, sums, d_out);
        }
        BWTS_TRY(delta_sums_scan(ctx, tiles, sums));
        SpanGuard sp(ctx, BWTS_K_OTHER, n, 2 * n);
        delta_f_kernel<DELTA_FINAL><<<grid, block, 0, ctx->stream>>>(d_in, S, sums, d_out);
    }
    HIPC(hipGetLastError());
    return BWTS_OK;
}
