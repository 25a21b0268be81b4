// mtf.hip -- move-to-front, the stage behind the transform (include/bwts_mtf.h), as a scan over 256-byte list states.
//
// The input is cut into tiles of MTF_T bytes; no tile crosses a segment start.  A tile's effect on the list is a STATE, and states
// compose associatively (not commutatively), so the list at every tile's start is an exclusive scan over tile states:
//   forward  state = (list after running MTF over the tile from the identity list, d = distinct symbols seen).
//            A then B = B.list[0 .. d_B) followed by the symbols of A.list that B has not seen, in A.list's order.
//   inverse  the tile's ranks are decoded on a list of PLACEHOLDERS 0 .. 255: that gives a placeholder index per position and a final
//            permutation pi with end[k] = start[pi[k]].  (A then B)[k] = A[B[k]]: a 256-byte gather.
//   a tile that starts a segment resets the prefix to the identity list: a flag beside the state.
// The scan has two levels: one wave composes the MTF_G states of a group one after the other (states in LDS), one wave runs over the
// group states, and a third kernel writes every tile's exclusive prefix over its state.  At 2^36 bytes that is 2^24 tiles in 2^15
// groups: two levels serve every length.
//   forward:  tile states (last occurrences, ranked) -> scan -> in-tile kernel from the real start list
//   inverse:  in-tile kernel on placeholders (indices to d_out, pi to the states) -> scan -> d_out[i] = start_t[d_out[i]]
// The in-tile kernel (one wave per tile, the list in registers, four entries per lane) is the hot path of both.
#include "internal.h"
#include "device_utils.h"

#define MTF_T 4096u
#define MTF_G 512u
#define MTF_RESET (1ull << 63)       // tile table: the tile starts a segment
#define MTF_MAX_N (1ull << 36)
#define DPP_WAVE_SHR1 0x138

// the identity list, lane l's four entries 4l .. 4l+3 (entry e in byte e & 3)
__device__ __forceinline__ u32 mtf_identity(int lane) { return 0x03020100u + 0x04040404u * (u32)lane; }

// [begin, end) of tile t and whether it starts a segment; without a table the input is one segment cut at multiples of MTF_T
__device__ __forceinline__ bool mtf_tile_span(const u64 *__restrict__ tile_off, u64 t, u64 n, u64 &begin, u64 &end)
{
    if (!tile_off) {
        begin = t * MTF_T;
        end = begin + MTF_T < n ? begin + MTF_T : n;
        return t == 0;
    }
    const u64 a = tile_off[t];
    begin = a & ~MTF_RESET;
    end = tile_off[t + 1] & ~MTF_RESET;
    return (a >> 63) != 0;
}

// ------------------------------------------------------------------------------------
// forward tile states
// ------------------------------------------------------------------------------------
// After MTF over a tile from the identity list the symbols seen stand in front, the most recent first, and the others behind them in
// ascending order.  key[s] = MTF_T - 1 - (last position of s) for a seen symbol, MTF_T + s for the others: distinct, and the list is
// the symbols in ascending key order.  Only a byte whose successor differs can be a last occurrence, so runs cost no LDS atomics.
__global__ __launch_bounds__(256) void mtf_tile_state_kernel(const u8 *__restrict__ in, const u64 *__restrict__ tile_off, u64 n, u64 tiles,
                                                             u8 *__restrict__ states, u32 *__restrict__ dcnt)
{
    __shared__ __attribute__((aligned(16))) u32 key[256];
    __shared__ u32 list32[64];
    u8 *list = (u8 *)list32;
    const u32 tid = threadIdx.x;
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        u64 begin, end;
        (void)mtf_tile_span(tile_off, t, n, begin, end);
        key[tid] = MTF_T + tid;
        __syncthreads();
        const u32 len = (u32)(end - begin);
        const u8 *p = in + begin;
        // 16 bytes per thread where the tile's address allows, single bytes in front of and behind that
        u32 head = (16u - (u32)((uintptr_t)p & 15)) & 15u;
        if (head > len) head = len;
        const u32 vecs = (len - head) / 16, done = head + vecs * 16;
        for (u32 v = tid; v < vecs; v += 256) {
            const uint4 q = ((const uint4 *)(p + head))[v];
            const u32 qw[4] = {q.x, q.y, q.z, q.w};
            const u32 base = head + 16 * v;
            const u32 behind = base + 16 < len ? (u32)p[base + 16] : 256u;      // (256: the tile's last byte has no equal behind it)
#pragma unroll
            for (int b = 0; b < 16; b++) {
                const u32 c = (qw[b >> 2] >> (8 * (b & 3))) & 255u;
                const u32 nx = b < 15 ? (qw[(b + 1) >> 2] >> (8 * ((b + 1) & 3))) & 255u : behind;
                if (c != nx) atomicMin(&key[c], MTF_T - 1 - (base + (u32)b));
            }
        }
#pragma unroll
        for (int side = 0; side < 2; side++) {
            const u32 i = side == 0 ? tid : done + tid;
            if (side == 0 ? tid < head : i < len) {
                const u8 c = p[i];
                if (i + 1 == len || p[i + 1] != c) atomicMin(&key[c], MTF_T - 1 - i);
            }
        }
        __syncthreads();
        const u32 mine = key[tid];
        u32 r = 0;
#pragma unroll 8
        for (int s = 0; s < 256; s += 4) {
            const uint4 k4 = *(const uint4 *)&key[s];
            r += (u32)(k4.x < mine) + (u32)(k4.y < mine) + (u32)(k4.z < mine) + (u32)(k4.w < mine);
        }
        list[r] = (u8)tid;
        const int d = __syncthreads_count(mine < MTF_T);
        if (tid < 64) ((u32 *)(states + t * 256))[tid] = list32[tid];
        if (tid == 0) dcnt[t] = (u32)d;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------
// the scan over states: one skeleton, two operators
// ------------------------------------------------------------------------------------
// acc (LDS, 256 bytes) becomes acc-then-B; B comes in registers, lane l holding its entries 4l .. 4l+3.  One wave, whole.
template <bool INV>
__device__ __forceinline__ void mtf_compose(u8 *&acc, u8 *&spare, u8 *seen, u32 &accd, u32 bl, u32 bd, int lane)
{
    if (INV) {
        const u32 r = (u32)acc[bl & 255] | ((u32)acc[(bl >> 8) & 255] << 8) | ((u32)acc[(bl >> 16) & 255] << 16) | ((u32)acc[bl >> 24] << 24);
        __syncthreads();
        ((u32 *)acc)[lane] = r;
        __syncthreads();
        return;
    }
    ((u32 *)seen)[lane] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const u32 e = 4u * (u32)lane + (u32)j, s = (bl >> (8 * j)) & 255;
        if (e < bd) { seen[s] = 1; spare[e] = (u8)s; }
    }
    __syncthreads();
    u32 base = bd, dnew = bd;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const u32 i = 64u * (u32)r + (u32)lane;
        const u32 s = acc[i];
        const bool keep = seen[s] == 0;
        const u64 m = __ballot(keep);
        if (keep) spare[base + (u32)__popcll(m & lanemask_lt())] = (u8)s;
        dnew += (u32)__popcll(__ballot(keep && i < accd));
        base += (u32)__popcll(m);
    }
    __syncthreads();
    u8 *x = acc; acc = spare; spare = x;
    accd = dnew;
}

struct MtfScanLds {
    u32 buf[3][64];
};

// what the running prefix is after tile (or group) B: B alone behind a reset, else acc-then-B
template <bool INV>
__device__ __forceinline__ void mtf_advance(u8 *&acc, u8 *&spare, u8 *seen, u32 &accd, u32 bl, u32 bd, bool reset, int lane)
{
    if (reset) {
        __syncthreads();
        ((u32 *)acc)[lane] = bl;
        accd = bd;
        __syncthreads();
    } else {
        mtf_compose<INV>(acc, spare, seen, accd, bl, bd, lane);
    }
}

// level 1: the state of every group of MTF_G consecutive tiles (and whether a segment starts inside it)
template <bool INV>
__global__ __launch_bounds__(64) void mtf_group_reduce_kernel(const u8 *__restrict__ states, const u32 *__restrict__ dcnt, const u64 *__restrict__ tile_off,
                                                              u64 tiles, u8 *__restrict__ gstates, u32 *__restrict__ gd, u32 *__restrict__ gflag)
{
    __shared__ MtfScanLds lds;
    const int lane = (int)threadIdx.x;
    const u64 g = blockIdx.x, t0 = g * MTF_G, t1 = t0 + MTF_G < tiles ? t0 + MTF_G : tiles;
    u8 *acc = (u8 *)lds.buf[0], *spare = (u8 *)lds.buf[1], *seen = (u8 *)lds.buf[2];
    ((u32 *)acc)[lane] = mtf_identity(lane);
    u32 accd = 0, any = 0;
    u64 b_, e_;
    u32 nb = ((const u32 *)(states + t0 * 256))[lane], nd = INV ? 0u : dcnt[t0];
    bool nf = mtf_tile_span(tile_off, t0, 0, b_, e_);
    __syncthreads();
    for (u64 t = t0; t < t1; t++) {
        const u32 bl = nb, bd = nd;
        const bool f = nf;
        if (t + 1 < t1) {
            nb = ((const u32 *)(states + (t + 1) * 256))[lane];
            nd = INV ? 0u : dcnt[t + 1];
            nf = mtf_tile_span(tile_off, t + 1, 0, b_, e_);
        }
        any |= f ? 1u : 0u;
        mtf_advance<INV>(acc, spare, seen, accd, bl, bd, f, lane);
    }
    ((u32 *)(gstates + g * 256))[lane] = ((u32 *)acc)[lane];
    if (lane == 0) { gd[g] = accd; gflag[g] = any; }
}

// level 2: one wave over the group states; every group's state is replaced by its exclusive prefix
template <bool INV>
__global__ __launch_bounds__(64) void mtf_top_scan_kernel(u8 *gstates, const u32 *__restrict__ gd, const u32 *__restrict__ gflag, u64 groups)
{
    __shared__ MtfScanLds lds;
    const int lane = (int)threadIdx.x;
    u8 *acc = (u8 *)lds.buf[0], *spare = (u8 *)lds.buf[1], *seen = (u8 *)lds.buf[2];
    ((u32 *)acc)[lane] = mtf_identity(lane);
    u32 accd = 0;
    u32 nb = ((const u32 *)gstates)[lane], nd = gd[0], nf = gflag[0];
    __syncthreads();
    for (u64 g = 0; g < groups; g++) {
        const u32 bl = nb, bd = nd, f = nf;
        if (g + 1 < groups) {
            nb = ((const u32 *)(gstates + (g + 1) * 256))[lane];
            nd = gd[g + 1];
            nf = gflag[g + 1];
        }
        ((u32 *)(gstates + g * 256))[lane] = ((u32 *)acc)[lane];
        mtf_advance<INV>(acc, spare, seen, accd, bl, bd, f != 0, lane);
    }
}

// level 3: every tile's state is replaced by its exclusive prefix, the list at the tile's start (the identity where a segment starts)
template <bool INV>
__global__ __launch_bounds__(64) void mtf_prefix_write_kernel(u8 *states, const u32 *__restrict__ dcnt, const u64 *__restrict__ tile_off, u64 tiles,
                                                              const u8 *__restrict__ gprefix)
{
    __shared__ MtfScanLds lds;
    const int lane = (int)threadIdx.x;
    const u64 g = blockIdx.x, t0 = g * MTF_G, t1 = t0 + MTF_G < tiles ? t0 + MTF_G : tiles;
    u8 *acc = (u8 *)lds.buf[0], *spare = (u8 *)lds.buf[1], *seen = (u8 *)lds.buf[2];
    ((u32 *)acc)[lane] = ((const u32 *)(gprefix + g * 256))[lane];
    u32 accd = 0;
    u64 b_, e_;
    u32 nb = ((const u32 *)(states + t0 * 256))[lane], nd = INV ? 0u : dcnt[t0];
    bool nf = mtf_tile_span(tile_off, t0, 0, b_, e_);
    __syncthreads();
    for (u64 t = t0; t < t1; t++) {
        const u32 bl = nb, bd = nd;
        const bool f = nf;
        if (t + 1 < t1) {
            nb = ((const u32 *)(states + (t + 1) * 256))[lane];
            nd = INV ? 0u : dcnt[t + 1];
            nf = mtf_tile_span(tile_off, t + 1, 0, b_, e_);
        }
        ((u32 *)(states + t * 256))[lane] = f ? mtf_identity(lane) : ((u32 *)acc)[lane];
        mtf_advance<INV>(acc, spare, seen, accd, bl, bd, f, lane);
    }
}

// ------------------------------------------------------------------------------------
// the in-tile kernel: one wave per tile, the list in registers
// ------------------------------------------------------------------------------------
// Symbol c moves to the front from list place 4h + j: every word one place up (byte 3 of the lane below comes in at byte 0, lane 0
// takes c), in the lanes below h whole (`below`: their mask, wave-uniform), in lane h (`here`) under the mask lm of bytes 0 .. j, not at
// all above.
__device__ __forceinline__ u32 mtf_move_to_front(u32 w, u32 c, u64 below, bool here, u32 lm)
{
    const u32 prev = (u32)__builtin_amdgcn_update_dpp((int)(c << 24), (int)w, DPP_WAVE_SHR1, 0xf, 0xf, false);
    const u32 sh = __builtin_amdgcn_alignbit(w, prev, 24);
    const u32 mixed = (sh & lm) | (w & ~lm);
    return __builtin_amdgcn_inverse_ballot_w64(below) ? sh : (here ? mixed : w);
}

// INV = false: in bytes -> ranks, from the list at starts[t] (null: the identity).  INV = true: ranks -> list entries, from the identity
// (the placeholders), and the final list goes to ends[t] when asked for.  64 bytes are loaded at a time, one per lane, the next 64
// before the current ones are stepped through; a byte of rank 0 changes nothing, so every step first skips to the next byte that
// is not the list's front (forward) or not 0 (inverse) with one ballot.
// The kernel is bound by instruction issue, scalar instructions included (about 2.2 cycles per instruction and SIMD at eight waves; two
// tiles per wave in lockstep, tried for latency, made it 45 % slower): what counts is the length of the step, so the loop tests
// its condition once, at the bottom.
template <bool INV>
__global__ __launch_bounds__(256) void mtf_tile_kernel(const u8 *__restrict__ in, u8 *__restrict__ out, const u64 *__restrict__ tile_off, u64 n, u64 tiles,
                                                       const u8 *__restrict__ starts, u8 *__restrict__ ends)
{
    const int lane = lane_id();
    const u64 t = (u64)blockIdx.x * 4 + (u64)__builtin_amdgcn_readfirstlane(wave_id());      // (wave-uniform, and known to be: scalar registers)
    if (t >= tiles) return;
    u64 begin, end;
    (void)mtf_tile_span(tile_off, t, n, begin, end);
    u32 w = starts ? ((const u32 *)(starts + t * 256))[lane] : mtf_identity(lane);
    u32 front = (u32)__builtin_amdgcn_readfirstlane((int)w) & 255u;       // the list's first entry, kept beside it
    u64 pos = begin;
    u32 nxt = pos + (u64)lane < end ? (u32)in[pos + (u64)lane] : 0u;
    while (pos < end) {
        const u32 byte = nxt;
        const u64 npos = pos + 64;
        nxt = npos + (u64)lane < end ? (u32)in[npos + (u64)lane] : 0u;
        const u64 left = end - pos;
        const u64 valid = left >= 64 ? ~0ull : (1ull << left) - 1ull;
        u32 outv;
        if (!INV) {
            outv = 0;
            u64 todo = valid;
            u64 ne = __ballot(byte != front) & todo;
            while (ne) {
                const int i = __builtin_ctzll(ne);
                todo &= ~((2ull << i) - 1ull);
                const u32 c = (u32)__builtin_amdgcn_readlane((int)byte, i);
                const u32 x = w ^ (c * 0x01010101u);
                const u32 z = (x - 0x01010101u) & ~x & 0x80808080u;       // bit 8j+7 of the lowest zero byte j; none in a word without one
                const u64 hit = __ballot(z != 0);                          // (the list is a permutation: exactly one lane)
                const int h = __builtin_ctzll(hit);
                const int j8 = __builtin_ctz((u32)__builtin_amdgcn_readlane((int)z, h));      // 8j + 7
                const u32 lm = 0xFFFFFFFFu >> (24 & ~j8);                  // bytes 0 .. j
                w = mtf_move_to_front(w, c, (1ull << h) - 1ull, z != 0, lm);
                outv = __builtin_amdgcn_inverse_ballot_w64(1ull << i) ? (u32)((h << 2) + (j8 >> 3)) : outv;
                front = c;
                ne = __ballot(byte != front) & todo;
            }
        } else {
            outv = front;
            u64 nz = __ballot(byte != 0) & valid;
            while (nz) {
                const int i = __builtin_ctzll(nz);
                nz &= nz - 1;
                const u32 k = (u32)__builtin_amdgcn_readlane((int)byte, i) & 255u;
                const int h = (int)(k >> 2), j = (int)(k & 3);
                const u32 c = ((u32)__builtin_amdgcn_readlane((int)w, h) >> (8 * j)) & 255u;
                const u32 lm = 0xFFFFFFFFu >> (24 - 8 * j);
                w = mtf_move_to_front(w, c, (1ull << h) - 1ull, __builtin_amdgcn_inverse_ballot_w64(1ull << h), lm);
                outv = __builtin_amdgcn_inverse_ballot_w64(~0ull << i) ? c : outv;
                front = c;
            }
        }
        if ((u64)lane < left) out[pos + (u64)lane] = (u8)outv;
        pos = npos;
    }
    if (INV && ends) ((u32 *)(ends + t * 256))[lane] = w;
}

// inverse, last pass: out[i] = start_t[out[i]] in place, the tile's 256-byte table in LDS, 16 bytes per access where the tile allows
__device__ __forceinline__ u32 mtf_map4(const u8 *lut, u32 v)
{
    return (u32)lut[v & 255] | ((u32)lut[(v >> 8) & 255] << 8) | ((u32)lut[(v >> 16) & 255] << 16) | ((u32)lut[v >> 24] << 24);
}

__global__ __launch_bounds__(256) void mtf_remap_kernel(u8 *out, const u64 *__restrict__ tile_off, u64 n, u64 tiles, const u8 *__restrict__ starts)
{
    __shared__ u32 lut32[64];
    const u8 *lut = (const u8 *)lut32;
    const u32 tid = threadIdx.x;
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        u64 begin, end;
        (void)mtf_tile_span(tile_off, t, n, begin, end);
        if (tid < 64) lut32[tid] = ((const u32 *)(starts + t * 256))[tid];
        __syncthreads();
        u8 *p = out + begin;
        const u32 len = (u32)(end - begin);
        u32 head = (16u - (u32)((uintptr_t)p & 15)) & 15u;
        if (head > len) head = len;
        if (tid < head) p[tid] = lut[p[tid]];
        const u32 vecs = (len - head) / 16;
        uint4 *v = (uint4 *)(p + head);
        for (u32 i = tid; i < vecs; i += 256) {
            uint4 q = v[i];
            q.x = mtf_map4(lut, q.x); q.y = mtf_map4(lut, q.y); q.z = mtf_map4(lut, q.z); q.w = mtf_map4(lut, q.w);
            v[i] = q;
        }
        const u32 done = head + vecs * 16;
        if (tid < len - done) p[done + tid] = lut[p[done + tid]];
        __syncthreads();
    }
}

// The tile table of a segmented call (unit_table_kernel): where every tile starts, a segment's first tile marked; the last entry is n.
struct MtfTileTable {
    const u64 *seg_off, *first_tile;
    u64 count, n;
    u64 *tile_off;
    __device__ u64 first(u64 s) const { return first_tile[s]; }
    __device__ u64 units(u64 s) const { return (seg_off[s + 1] - seg_off[s] + MTF_T - 1) / MTF_T; }
    __device__ void store(u64 s, u64 first, u64 units, u64 j) const
    {
        tile_off[first + j] = (seg_off[s] + j * MTF_T) | (j == 0 ? MTF_RESET : 0ull);
        if (s + 1 == count && j + 1 == units) tile_off[first + units] = n;
    }
};

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
struct MtfPlan { u64 tiles, groups; };

static MtfPlan mtf_plan_tiles(u64 tiles)
{
    MtfPlan p;
    p.tiles = tiles;
    p.groups = (tiles + MTF_G - 1) / MTF_G;
    return p;
}

struct MtfBufs {
    u8  *states, *gstates;
    u32 *dcnt, *gd, *gflag;
    u64 *tile_off;
    void declare(BlockLayout &L, const MtfPlan &p, bool table)
    {
        L.array(&states, p.tiles * 256); L.array(&dcnt, p.tiles);
        L.array(&gstates, p.groups * 256); L.arrays(p.groups, &gd, &gflag);
        if (table) L.array(&tile_off, p.tiles + 1);
        else tile_off = nullptr;
    }
};

void bwts_mtf_plan(u64 n, u64 out[4])
{
    const MtfPlan p = mtf_plan_tiles(stage_cut_single(n, MTF_T).units[0]);
    out[0] = MTF_T; out[1] = MTF_G; out[2] = p.tiles; out[3] = p.groups;
}

size_t mtf_arena_bytes(const bwts_ctx *ctx, u64 n, SegMode segs)
{
    if (n == 0 || n > MTF_MAX_N) return 0;
    segs = segs.one_as_single();
    const MtfPlan p = mtf_plan_tiles(stage_cut_call(ctx, segs, n, MTF_T).units[0]);
    MtfBufs b;
    BlockLayout L;
    b.declare(L, p, segs.table());
    return L.bytes();
}

static unsigned mtf_grid(u64 blocks) { return (unsigned)(blocks < (1ull << 30) ? blocks : (1ull << 30)); }

template <bool INV>
static int mtf_scan(bwts_ctx *ctx, const MtfBufs &b, const MtfPlan &p)
{
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, p.tiles, p.tiles * 256);
        mtf_group_reduce_kernel<INV><<<dim3((unsigned)p.groups), dim3(64), 0, ctx->stream>>>(b.states, b.dcnt, b.tile_off, p.tiles, b.gstates, b.gd, b.gflag);
    }
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, p.groups, p.groups * 512);
        mtf_top_scan_kernel<INV><<<dim3(1), dim3(64), 0, ctx->stream>>>(b.gstates, b.gd, b.gflag, p.groups);
    }
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, p.tiles, p.tiles * 512);
        mtf_prefix_write_kernel<INV><<<dim3((unsigned)p.groups), dim3(64), 0, ctx->stream>>>(b.states, b.dcnt, b.tile_off, p.tiles, b.gstates);
    }
    HIPC(hipGetLastError());
    return BWTS_OK;
}

int mtf_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, bool inverse, SegMode segs)
{
    if (n > MTF_MAX_N) return BWTS_E_RANGE;
    if (ranges_overlap(d_in, n, d_out, n)) return BWTS_E_ARG;
    segs = segs.one_as_single();
    const StageCut cut = stage_cut_call(ctx, segs, n, MTF_T);
    const MtfPlan p = mtf_plan_tiles(cut.units[0]);
    if (p.groups > 0x7fffffffull) return BWTS_E_RANGE;
    const unsigned wave_blocks = mtf_grid((p.tiles + 3) / 4);
    if ((u64)wave_blocks * 4 < p.tiles) return BWTS_E_RANGE;
    if (p.tiles == 1) {
        // one tile: its start list is the identity, and the placeholders are the symbols themselves
        SpanGuard sp(ctx, BWTS_K_OTHER, n, 2 * n);
        if (inverse) mtf_tile_kernel<true><<<dim3(1), dim3(256), 0, ctx->stream>>>(d_in, d_out, nullptr, n, 1, nullptr, nullptr);
        else mtf_tile_kernel<false><<<dim3(1), dim3(256), 0, ctx->stream>>>(d_in, d_out, nullptr, n, 1, nullptr, nullptr);
        HIPC(hipGetLastError());
        return BWTS_OK;
    }
    MtfBufs b;
    BlockLayout L;
    b.declare(L, p, segs.table());
    BWTS_TRY(arena_take(ctx, L));
    if (segs.table()) {
        // every segment's first tile goes up behind the segment table (pinned, on the stream); the table itself is made on the device
        u64 *d_first = nullptr;
        BWTS_TRY(seg_upload_extra(ctx, cut.first[0].data(), cut.count, &d_first));
        SpanGuard sp(ctx, BWTS_K_OTHER, p.tiles, 8 * p.tiles);
        unit_table_launch(ctx->stream, cut.count, MtfTileTable{d_seg_off(ctx), d_first, cut.count, n, b.tile_off});
    }
    const unsigned tile_blocks = mtf_grid(p.tiles);
    if (!inverse) {
        {
            SpanGuard sp(ctx, BWTS_K_OTHER, n, n);
            mtf_tile_state_kernel<<<dim3(tile_blocks), dim3(256), 0, ctx->stream>>>(d_in, b.tile_off, n, p.tiles, b.states, b.dcnt);
        }
        BWTS_TRY(mtf_scan<false>(ctx, b, p));
        SpanGuard sp(ctx, BWTS_K_OTHER, n, 2 * n);
        mtf_tile_kernel<false><<<dim3(wave_blocks), dim3(256), 0, ctx->stream>>>(d_in, d_out, b.tile_off, n, p.tiles, b.states, nullptr);
    } else {
        {
            SpanGuard sp(ctx, BWTS_K_OTHER, n, 2 * n);
            mtf_tile_kernel<true><<<dim3(wave_blocks), dim3(256), 0, ctx->stream>>>(d_in, d_out, b.tile_off, n, p.tiles, nullptr, b.states);
        }
        BWTS_TRY(mtf_scan<true>(ctx, b, p));
        SpanGuard sp(ctx, BWTS_K_OTHER, n, 2 * n);
        mtf_remap_kernel<<<dim3(tile_blocks), dim3(256), 0, ctx->stream>>>(d_out, b.tile_off, n, p.tiles, b.states);
    }
    HIPC(hipGetLastError());
    return BWTS_OK;
}
