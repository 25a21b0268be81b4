// zrl.hip -- zero-run coding of move-to-front ranks, the stage between mtf.hip and ec.hip (include/bwts_zrl.h; the coded form is
// stated there and in DESIGN section 15, tests/zrl_model.py is its executable form; the arithmetic shared with the host is in
// zrl_plan.h).
//
// One side of a call is cut into tiles of ZRL_T bytes, no tile across a segment start: the ranks of an encode, the coded bytes of a
// decode.  A workgroup of 256 threads works on one tile, every thread on 64 consecutive bytes that it keeps in registers and walks
// one after the other.
//   encode: tile summaries (where the tile's last rank that is not 0 lies, the bytes that everything but the tile's leading run of
//           zeros becomes, that run's length where it ends in the tile) -> a max-scan gives every tile the start of the run carried
//           into it -> a sum-scan of the tiles' bytes, the leading runs' digits now known, gives the offsets and the total -> the host
//           (one input) or a kernel (segments) decides coded or stored and refuses what does not fit -> the storing pass walks the
//           tile again into LDS and writes it out in 16-byte units, or copies a stored segment's tile.
//   decode: tile weights (the zeros and ranks the tile's bytes stand for; every check of the form is made here) -> a saturating
//           sum-scan gives the offsets; the total and the flags go to the host, which refuses a wrong input before a byte is written
//           -> the output is cleared -> the writing pass puts every rank that is not 0 at its place.  A digit writes nothing, so one
//           that stands for 2^36 zeros costs what any other byte costs; the zeros come from the clear, at the speed of a fill.
// A decoding thread needs from the bytes in front of its own only whether the last one is 255 and how many digits stand directly
// in front (zrl_state_at: at most 37 bytes back), and from the other tiles only the scanned offsets.
#include "internal.h"
#include "device_utils.h"
#include "scan_templ.h"
#include "zrl_plan.h"
#include "../../include/bwts_zrl.h"

#define ZRL_CHUNK 64u                    // bytes a thread walks: ZRL_T / 256
#define ZRL_STAGE_BYTES (2u * ZRL_T + 64u)   // a tile's coded bytes (at most 2 T + 36) behind up to 15 bytes that align LDS with the output

// The segments of a call as the kernels see them.  a: the side that is cut into tiles; b: the other side (encode: the output, decode:
// the ranks).  tseg == null: one input of a_bytes, its other side b_bytes long.
struct ZrlSegs {
    const u64 *a_off;       // [count + 1] where every segment starts on the tiled side
    const u64 *first;       // [count] the segment's first tile, counted over the call
    const u32 *tseg;        // [tiles] the segment of every tile
    const u64 *b_off;       // [count + 1] where every segment starts on the other side
    u64 a_bytes, b_bytes, tiles;
};

struct ZrlTile {
    u64 seg_a, seg_a_len, begin, seg_b, seg_b_len, first_tile;
    u32 len;
    bool first;
};

__device__ __forceinline__ ZrlTile zrl_tile(const ZrlSegs &S, u64 t)
{
    ZrlTile R;
    if (!S.tseg) {
        R.seg_a = 0; R.seg_a_len = S.a_bytes; R.seg_b = 0; R.seg_b_len = S.b_bytes; R.first_tile = 0;
    } else {
        const u64 s = S.tseg[t];
        R.seg_a = S.a_off[s]; R.seg_a_len = S.a_off[s + 1] - R.seg_a;
        R.seg_b = S.b_off[s]; R.seg_b_len = S.b_off[s + 1] - R.seg_b;
        R.first_tile = S.first[s];
    }
    const u64 at = (t - R.first_tile) << ZRL_LOG_T;
    R.begin = R.seg_a + at;
    R.len = R.seg_a_len - at < ZRL_T ? (u32)(R.seg_a_len - at) : ZRL_T;
    R.first = at == 0;
    return R;
}

// tseg of a segmented call (unit_table_kernel)
struct ZrlTileTable {
    const u64 *a_off, *first_tile;
    u32 *tseg;
    __device__ u64 first(u64 s) const { return first_tile[s]; }
    __device__ u64 units(u64 s) const { return zrl_tiles(a_off[s + 1] - a_off[s]); }
    __device__ void store(u64 s, u64 first, u64, u64 j) const { tseg[first + j] = (u32)s; }
};

// byte k of a chunk in registers (k a constant after unrolling: q never leaves the registers)
#define ZRL_BYTE(q, k) (((q)[(k) >> 2] >> (8 * ((k) & 3))) & 255u)

// A thread's 64 bytes (zero past `valid`): four 16-byte loads where the chunk is whole and its address allows, single bytes otherwise.
__device__ __forceinline__ void zrl_load_chunk(const u8 *p, u32 valid, u32 (&q)[16])
{
    if (valid == ZRL_CHUNK && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const uint4 x = ((const uint4 *)p)[v];
            q[4 * v] = x.x; q[4 * v + 1] = x.y; q[4 * v + 2] = x.z; q[4 * v + 3] = x.w;
        }
        return;
    }
#pragma unroll
    for (int w = 0; w < 16; w++) q[w] = 0;
#pragma unroll
    for (int k = 0; k < 64; k++)
        if ((u32)k < valid) q[k >> 2] |= (u32)p[k] << (8 * (k & 3));
}

// len bytes from src to dst, the whole workgroup: 16 bytes per access where both addresses allow
__device__ __forceinline__ void zrl_copy_tile(const u8 *src, u8 *dst, u32 len)
{
    const u32 tid = threadIdx.x;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const u32 vecs = len / 16;
        for (u32 v = tid; v < vecs; v += 256) ((uint4 *)dst)[v] = ((const uint4 *)src)[v];
        if (tid < len - vecs * 16) dst[vecs * 16 + tid] = src[vecs * 16 + tid];
        return;
    }
    for (u32 i = tid; i < len; i += 256) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------
// the encoder
// ------------------------------------------------------------------------------------
template <bool EMIT>
__device__ __forceinline__ u32 zrl_put_run(u8 *dst, u32 o, u64 L)
{
    const u32 k = zrl_digits(L);
    if (EMIT)
        for (u32 i = 0; i < k; i++) dst[o + i] = (u8)zrl_digit(L, i);
    return o + k;
}

// The walk over a thread's ranks.  L: the zeros directly in front of the chunk that belong to its first run (dropped where the chunk
// does not start with a zero: that run has ended in front of it); skip: the first run is the tile's leading run, which the summary
// leaves out; next_ends: a run that reaches the chunk's end ends there.  Returns o moved over the bytes the chunk's ranks and
// the runs that end in it become; EMIT writes them to dst.
template <bool EMIT>
__device__ __forceinline__ u32 zrl_encode_walk(const u32 (&q)[16], u32 valid, u64 L, bool skip, bool next_ends, u8 *dst, u32 o)
{
    if (valid == 0) return o;
    if (ZRL_BYTE(q, 0) != 0) { L = 0; skip = false; }
#pragma unroll
    for (int k = 0; k < 64; k++) {
        if ((u32)k < valid) {
            const u32 c = ZRL_BYTE(q, k);
            if (c == 0) {
                L++;
            } else {
                if (L) {
                    if (!skip) o = zrl_put_run<EMIT>(dst, o, L);
                    L = 0;
                }
                skip = false;
                if (EMIT) {
                    if (c >= 254u) { dst[o] = 255u; dst[o + 1] = (u8)(c - 254u); }
                    else dst[o] = (u8)(c + 1u);
                }
                o += zrl_literal_bytes(c);
            }
        }
    }
    if (L && next_ends && !skip) o = zrl_put_run<EMIT>(dst, o, L);
    return o;
}

// What both encoder kernels know of a thread's chunk before they walk it.
struct ZrlEncThread {
    u32 valid;
    u32 before;         // where, in the tile, the last rank that is not 0 in front of the chunk ends (0: there is none)
    u32 tile_last;      // the same for the whole tile
    u32 tile_lead;      // the tile's leading zeros
    bool next_ends, tile_next_ends;
};

struct ZrlEncLds {
    u32 scan[4];
    u32 first_nz[257];
    u32 lead, next_ends;
};

__device__ __forceinline__ ZrlEncThread zrl_encode_prepare(const u8 *in, const ZrlTile &R, u32 (&q)[16], ZrlEncLds &lds)
{
    const u32 tid = threadIdx.x, at = tid * ZRL_CHUNK;
    ZrlEncThread E;
    E.valid = at >= R.len ? 0u : (R.len - at < ZRL_CHUNK ? R.len - at : ZRL_CHUNK);
    zrl_load_chunk(in + R.begin + at, E.valid, q);
    u32 last = 0, lead = E.valid;       // (bytes past `valid` are zero)
#pragma unroll
    for (int k = 63; k >= 0; k--)
        if (ZRL_BYTE(q, k) != 0) lead = (u32)k;
#pragma unroll
    for (int k = 0; k < 64; k++)
        if (ZRL_BYTE(q, k) != 0) last = (u32)k + 1u;
    if (tid == 0) {
        lds.lead = R.len;
        // the byte behind the tile: a run that reaches the tile's end ends there unless the segment goes on with a zero
        lds.next_ends = R.begin + R.len == R.seg_a + R.seg_a_len || in[R.begin + R.len] != 0 ? 1u : 0u;
    }
    lds.first_nz[tid] = E.valid && ZRL_BYTE(q, 0) != 0 ? 1u : 0u;
    __syncthreads();
    if (lead < E.valid) atomicMin(&lds.lead, at + lead);
    E.before = block_scan_exclusive<u32, OpMax, 4>(last ? at + last : 0u, OpMax(), 0u, lds.scan, &E.tile_last);
    E.tile_lead = lds.lead;
    E.tile_next_ends = lds.next_ends != 0;
    E.next_ends = at + ZRL_CHUNK < R.len ? lds.first_nz[tid + 1] != 0 : E.tile_next_ends;
    return E;
}

// per tile: last[t] = where the tile's last rank that is not 0 ends, counted over the call (a segment's first tile: at least its
// start, so that no run is carried across a segment start; 0: no such rank), cnt[t] = the bytes of everything but the leading run,
// lead[t] = the leading run's zeros inside the tile where it ends in the tile (0: no leading run, or it goes on)
__global__ __launch_bounds__(256) void zrl_summary_kernel(const u8 *__restrict__ in, ZrlSegs S, u64 *__restrict__ last, u32 *__restrict__ cnt, u32 *__restrict__ lead)
{
    __shared__ ZrlEncLds lds;
    const u64 t = blockIdx.x;
    const ZrlTile R = zrl_tile(S, t);
    u32 q[16];
    const ZrlEncThread E = zrl_encode_prepare(in, R, q, lds);
    const u32 at = threadIdx.x * ZRL_CHUNK;
    const u32 mine = zrl_encode_walk<false>(q, E.valid, (u64)(at - E.before), E.before == 0, E.next_ends, nullptr, 0u);
    u32 total;
    (void)block_scan_exclusive<u32, OpAdd, 4>(mine, OpAdd(), 0u, lds.scan, &total);
    if (threadIdx.x == 0) {
        last[t] = E.tile_last ? R.begin + E.tile_last : (R.first ? R.begin : 0ull);
        cnt[t] = total;
        lead[t] = E.tile_lead < R.len || E.tile_next_ends ? E.tile_lead : 0u;
    }
}

// the zeros in front of tile t that belong to its leading run
__device__ __forceinline__ u64 zrl_carried(const ZrlTile &R, const u64 *__restrict__ run_start, u64 t) { return R.first ? 0ull : R.begin - run_start[t]; }

// sum-scan input: the bytes tile i becomes, the leading run's digits from the scanned run starts
struct ZrlBytesIn {
    ZrlSegs S;
    const u64 *run_start;
    const u32 *cnt, *lead;
    __device__ __forceinline__ u64 operator()(u64 i) const
    {
        if (i >= S.tiles) return 0;
        const u32 l = lead[i];
        return (u64)cnt[i] + (l ? zrl_digits((u64)l + zrl_carried(zrl_tile(S, i), run_start, i)) : 0u);
    }
};

struct ZrlOffOut {
    u64 *offs, nt, *total;
    __device__ __forceinline__ void operator()(u64 i, u64 v) const
    {
        offs[i] = v;
        if (i == nt) *total = v;
    }
};

// the bytes every segment of a segmented encode puts out: its coded bytes where they are fewer than its ranks, else the ranks
__global__ __launch_bounds__(256) void zrl_out_lengths_kernel(const u64 *__restrict__ a_off, const u64 *__restrict__ first, u64 count, const u64 *__restrict__ offs,
                                                              u64 *__restrict__ out_len)
{
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= count) return;
    const u64 len = a_off[s + 1] - a_off[s], m = offs[first[s + 1]] - offs[first[s]];
    out_len[s] = m < len ? m : len;
}

struct ZrlLenIn {
    const u64 *v;
    u64 count;
    __device__ __forceinline__ u64 operator()(u64 i) const { return i < count ? v[i] : 0ull; }
};

// the storing pass: a coded segment's tile is walked into LDS, at the output's alignment, and goes out from there; a stored segment's
// tile is copied
__global__ __launch_bounds__(256) void zrl_store_kernel(const u8 *__restrict__ in, ZrlSegs S, const u64 *__restrict__ run_start, const u64 *__restrict__ offs,
                                                        u8 *__restrict__ out)
{
    __shared__ ZrlEncLds lds;
    __shared__ __attribute__((aligned(16))) u8 stage[ZRL_STAGE_BYTES];
    const u64 t = blockIdx.x;
    const u32 tid = threadIdx.x;
    const ZrlTile R = zrl_tile(S, t);
    if (R.seg_b_len >= R.seg_a_len) {
        zrl_copy_tile(in + R.begin, out + R.seg_b + (R.begin - R.seg_a), R.len);
        return;
    }
    u32 q[16];
    const ZrlEncThread E = zrl_encode_prepare(in, R, q, lds);
    const u32 at = tid * ZRL_CHUNK;
    const u64 L = E.before ? (u64)(at - E.before) : (u64)at + zrl_carried(R, run_start, t);
    const u32 mine = zrl_encode_walk<false>(q, E.valid, L, false, E.next_ends, nullptr, 0u);
    u32 total;
    const u32 prefix = block_scan_exclusive<u32, OpAdd, 4>(mine, OpAdd(), 0u, lds.scan, &total);
    const u64 off = offs[t] - offs[R.first_tile];
    // (what the tile wrote must be what the scan gave it, and must end inside the segment's coded bytes: both hold by construction,
    // and neither is relied on for an address)
    if (total != (u32)(offs[t + 1] - offs[t]) || total > 2u * ZRL_T + ZRL_MAX_DIGITS || off + total > R.seg_b_len) return;
    u8 *dst = out + R.seg_b + off;
    const u32 shift = (u32)((uintptr_t)dst & 15);
    (void)zrl_encode_walk<true>(q, E.valid, L, false, E.next_ends, stage + shift, prefix);
    __syncthreads();
    u32 head = (16u - shift) & 15u;
    if (head > total) head = total;
    if (tid < head) dst[tid] = stage[shift + tid];
    const u32 vecs = (total - head) / 16, done = head + vecs * 16;
    for (u32 v = tid; v < vecs; v += 256) ((uint4 *)(dst + head))[v] = ((const uint4 *)(stage + shift + head))[v];
    if (tid < total - done) dst[done + tid] = stage[shift + done + tid];
}

// ------------------------------------------------------------------------------------
// the decoder
// ------------------------------------------------------------------------------------
// The walk over a thread's coded bytes from the state s in front of them; WRITE puts every rank that is not 0 at its place below
// out_len (pos comes from weights that were checked, and is tested all the same).
template <bool WRITE>
__device__ __forceinline__ void zrl_decode_walk(const u32 (&q)[16], u32 valid, zrl_state &s, u8 *out, u64 out_len)
{
#pragma unroll
    for (int k = 0; k < 64; k++) {
        if ((u32)k < valid) {
            const u64 at = s.pos;
            const u32 v = zrl_step(s, ZRL_BYTE(q, k));
            if (WRITE && v && at < out_len) out[at] = (u8)v;
        }
    }
}

// a thread's chunk of a coded tile and the state in front of it
__device__ __forceinline__ zrl_state zrl_decode_prepare(const u8 *in, const ZrlTile &R, u32 (&q)[16], u32 &valid)
{
    const u32 at = threadIdx.x * ZRL_CHUNK;
    valid = at >= R.len ? 0u : (R.len - at < ZRL_CHUNK ? R.len - at : ZRL_CHUNK);
    zrl_load_chunk(in + R.begin + at, valid, q);
    zrl_state s = {0u, 0u, 0u, 0ull};
    if (valid) {
        const u64 p = R.begin - R.seg_a + at;       // in the segment's coded bytes
        const u8 *z = in + R.seg_a;
        s.prev = p > 0 ? z[p - 1] : 0u;
        // (only a chunk that starts with a digit needs the digits in front of it)
        if (s.prev != 255u && ZRL_BYTE(q, 0) <= 1u) s.i = zrl_digits_before(z, p);
    }
    return s;
}

struct OpAddSat {       // weights add up to at most 2^50 per tile: the sum stays put at 2^62, and no addition wraps
    __device__ __forceinline__ u64 operator()(u64 a, u64 b) const { const u64 c = a + b; return c < (1ull << 62) ? c : (1ull << 62); }
};

// per tile: the zeros and ranks its bytes stand for (a stored segment's tile: its bytes); whatever is wrong with the form goes to *err
__global__ __launch_bounds__(256) void zrl_weigh_kernel(const u8 *__restrict__ in, ZrlSegs S, u64 *__restrict__ weight, u32 *__restrict__ err)
{
    __shared__ u64 scan[4];
    const u64 t = blockIdx.x;
    const ZrlTile R = zrl_tile(S, t);
    if (R.seg_a_len >= R.seg_b_len) {
        if (threadIdx.x == 0) weight[t] = R.len;
        return;
    }
    u32 q[16], valid;
    zrl_state s = zrl_decode_prepare(in, R, q, valid);
    zrl_decode_walk<false>(q, valid, s, nullptr, 0);
    const u64 end = R.begin - R.seg_a + threadIdx.x * ZRL_CHUNK + valid;
    if (valid && end == R.seg_a_len && s.prev == 255u) s.err |= ZRL_BAD_END;
    if (s.err) atomicOr(err, s.err);
    u64 total;
    (void)block_scan_exclusive<u64, OpAdd, 4>(s.pos, OpAdd(), 0ull, scan, &total);
    if (threadIdx.x == 0) weight[t] = total;
}

struct ZrlWeightIn {
    const u64 *v;
    u64 nt;
    __device__ __forceinline__ u64 operator()(u64 i) const { return i < nt ? v[i] : 0ull; }
};

// every segment's weights must sum to its length (the call's total has been seen to be the lengths' sum: nothing has saturated)
__global__ __launch_bounds__(256) void zrl_segment_sums_kernel(ZrlSegs S, u64 count, const u64 *__restrict__ offs, u32 *__restrict__ err)
{
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= count) return;
    const u64 t0 = S.first[s], t1 = s + 1 < count ? S.first[s + 1] : S.tiles;
    if (offs[t1] - offs[t0] != S.b_off[s + 1] - S.b_off[s]) atomicOr(err, ZRL_BAD_SUM);
}

// the writing pass, into an output that has been cleared
__global__ __launch_bounds__(256) void zrl_write_kernel(const u8 *__restrict__ in, ZrlSegs S, const u64 *__restrict__ offs, u8 *__restrict__ out)
{
    __shared__ u64 scan[4];
    const u64 t = blockIdx.x;
    const ZrlTile R = zrl_tile(S, t);
    if (R.seg_a_len >= R.seg_b_len) {
        const u64 at = R.begin - R.seg_a;
        if (at + R.len <= R.seg_b_len) zrl_copy_tile(in + R.begin, out + R.seg_b + at, R.len);
        return;
    }
    u32 q[16], valid;
    const zrl_state s0 = zrl_decode_prepare(in, R, q, valid);
    zrl_state s = s0;
    zrl_decode_walk<false>(q, valid, s, nullptr, 0);
    u64 total;
    const u64 prefix = block_scan_exclusive<u64, OpAdd, 4>(s.pos, OpAdd(), 0ull, scan, &total);
    s = s0;
    s.pos = offs[t] - offs[R.first_tile] + prefix;
    zrl_decode_walk<true>(q, valid, s, out + R.seg_b, R.seg_b_len);
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
// how a call is cut: a_off holds the tiled side's offsets (segments), words what goes up behind the context's table
struct ZrlPlan {
    u64 count, tiles;
    std::vector<u64> words;
};

struct ZrlBufs {
    u64 *last, *run_start, *offs, *out_len, *b_off;
    u32 *cnt, *lead, *tseg;
    void *scan_temp;
    void declare(BlockLayout &L, const ZrlPlan &p, bool encode, bool segments)
    {
        L.array(&offs, p.tiles + 1); L.array(&last, p.tiles);       // (decode: last holds the weights)
        const u64 longest = p.tiles + 1 > p.count + 1 ? p.tiles + 1 : p.count + 1;
        L.raw(&scan_temp, scan_temp_bytes_t(longest, sizeof(u64)));
        if (encode) { L.array(&run_start, p.tiles); L.arrays(p.tiles, &cnt, &lead); }
        if (segments) L.array(&tseg, p.tiles);
        if (segments && encode) { L.array(&out_len, p.count); L.array(&b_off, p.count + 1); }
    }
};

void bwts_zrl_plan(u64 n, u64 out[2])
{
    out[0] = ZRL_T; out[1] = stage_cut_single(n, ZRL_T).units[0];
}

static int zrl_prepare(bwts_ctx *ctx, ZrlPlan &p, const StageCut &cut, const u64 *a_off, bool encode, bool segments, ZrlBufs &b, ZrlSegs &S)
{
    p.count = cut.count; p.tiles = cut.units[0];
    if (p.tiles >= (1ull << 31)) return BWTS_E_RANGE;
    BlockLayout L;
    b.declare(L, p, encode, segments);
    BWTS_TRY(arena_take(ctx, L));
    S.a_off = S.first = S.b_off = nullptr; S.tseg = nullptr; S.tiles = p.tiles;
    if (!segments) return BWTS_OK;
    // behind the context's table: encode: every segment's first tile and the total; decode: the coded side's offsets, then the first tiles
    u64 *d_words = nullptr;
    if (encode) {
        p.words.assign(cut.first[0].begin(), cut.first[0].end());
        BWTS_TRY(seg_upload_extra(ctx, p.words.data(), p.count + 1, &d_words));
        S.a_off = d_seg_off(ctx); S.first = d_words; S.b_off = b.b_off;
    } else {
        p.words.assign(a_off, a_off + p.count + 1);
        p.words.insert(p.words.end(), cut.first[0].begin(), cut.first[0].begin() + (long)p.count);
        BWTS_TRY(seg_upload_extra(ctx, p.words.data(), 2 * p.count + 1, &d_words));
        S.a_off = d_words; S.first = d_words + p.count + 1; S.b_off = d_seg_off(ctx);
    }
    S.tseg = b.tseg;
    SpanGuard sp(ctx, BWTS_K_OTHER, p.tiles, 4 * p.tiles);
    unit_table_launch(ctx->stream, p.count, ZrlTileTable{S.a_off, S.first, b.tseg});
    return BWTS_OK;
}

// sizes: the bytes the one input becomes, or every segment's (sizes[count])
int zrl_encode_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, u64 out_cap, SegMode segs, u64 *sizes)
{
    const bool segments = segs.table();
    const StageCut cut = stage_cut_call(ctx, segs, n, ZRL_T);
    ZrlPlan p;
    ZrlBufs b;
    ZrlSegs S;
    BWTS_TRY(zrl_prepare(ctx, p, cut, nullptr, true, segments, b, S));
    S.a_bytes = n; S.b_bytes = 0;
    const unsigned grid = (unsigned)p.tiles;
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, n);
        zrl_summary_kernel<<<dim3(grid), dim3(256), 0, ctx->stream>>>(d_in, S, b.last, b.cnt, b.lead);
    }
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, p.tiles, 16 * p.tiles);
        BWTS_TRY((device_scan<false, u64>(ctx, p.tiles, ScanLoadArr<u64>{b.last}, ScanStoreArr<u64>{b.run_start}, OpMax(), (u64)0, b.scan_temp)));
    }
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, p.tiles, 24 * p.tiles);
        BWTS_TRY((device_scan<false, u64>(ctx, p.tiles + 1, ZrlBytesIn{S, b.run_start, b.cnt, b.lead}, ZrlOffOut{b.offs, p.tiles, ctx->d_small + SM_ZRL_TOTAL},
                                          OpAdd(), (u64)0, b.scan_temp)));
    }
    u64 total = 0;
    if (segments) {
        {
            SpanGuard sp(ctx, BWTS_K_OTHER, p.count, 32 * p.count);
            zrl_out_lengths_kernel<<<dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, ctx->stream>>>(S.a_off, S.first, p.count, b.offs, b.out_len);
        }
        {
            SpanGuard sp(ctx, BWTS_K_OTHER, p.count, 16 * p.count);
            BWTS_TRY((device_scan<false, u64>(ctx, p.count + 1, ZrlLenIn{b.out_len, p.count}, ZrlOffOut{b.b_off, p.count, ctx->d_small + SM_ZRL_TOTAL},
                                              OpAdd(), (u64)0, b.scan_temp)));
        }
        HIPC(hipGetLastError());
        BWTS_TRY(read_small(ctx, SM_ZRL_TOTAL, 1));
        total = ctx->h_small[SM_ZRL_TOTAL];
    } else {
        HIPC(hipGetLastError());
        BWTS_TRY(read_small(ctx, SM_ZRL_TOTAL, 1));
        const u64 m = ctx->h_small[SM_ZRL_TOTAL];
        total = m < n ? m : n;
        S.b_bytes = total;
    }
    if (total > out_cap) return BWTS_E_SPACE;
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, n + total);
        zrl_store_kernel<<<dim3(grid), dim3(256), 0, ctx->stream>>>(d_in, S, b.run_start, b.offs, d_out);
    }
    HIPC(hipGetLastError());
    if (segments) {
        HIPC(hipMemcpyAsync(sizes, b.out_len, p.count * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
        HIPC(hipStreamSynchronize(ctx->stream));
    } else {
        *sizes = total;
    }
    return BWTS_OK;
}

// one coded input of in_bytes that stands for n ranks, or one per segment of the context's table (in_lengths[count]; in_bytes: their sum)
int zrl_decode_impl(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, u8 *d_out, u64 n, SegMode segs, const u64 *in_lengths)
{
    const bool segments = segs.table();
    std::vector<u64> a_off;
    bool any_coded = !segments && in_bytes < n;
    if (segments) {
        a_off.resize((size_t)segs.count + 1);
        a_off[0] = 0;
        for (u64 s = 0; s < segs.count; s++) {
            a_off[s + 1] = a_off[s] + in_lengths[s];
            any_coded = any_coded || in_lengths[s] < ctx->seg_off[s + 1] - ctx->seg_off[s];
        }
    }
    const StageCut cut = segments ? stage_cut(a_off.data(), segs.count, ZRL_T) : stage_cut_single(in_bytes, ZRL_T);
    ZrlPlan p;
    ZrlBufs b;
    ZrlSegs S;
    BWTS_TRY(zrl_prepare(ctx, p, cut, a_off.data(), false, segments, b, S));
    S.a_bytes = in_bytes; S.b_bytes = n;
    const unsigned grid = (unsigned)p.tiles;
    u32 *d_flag = (u32 *)(ctx->d_small + SM_ZRL_FLAG);
    HIPC(hipMemsetAsync(d_flag, 0, sizeof(u64), ctx->stream));
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, in_bytes, in_bytes);
        zrl_weigh_kernel<<<dim3(grid), dim3(256), 0, ctx->stream>>>(d_in, S, b.last, d_flag);
    }
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, p.tiles, 24 * p.tiles);
        BWTS_TRY((device_scan<false, u64>(ctx, p.tiles + 1, ZrlWeightIn{b.last, p.tiles}, ZrlOffOut{b.offs, p.tiles, ctx->d_small + SM_ZRL_TOTAL}, OpAddSat(),
                                          (u64)0, b.scan_temp)));
    }
    HIPC(hipGetLastError());
    BWTS_TRY(read_small(ctx, SM_ZRL_TOTAL, 2));
    if ((u32)ctx->h_small[SM_ZRL_FLAG] != 0 || ctx->h_small[SM_ZRL_TOTAL] != n) return BWTS_E_FORMAT;
    if (segments && any_coded) {
        {
            SpanGuard sp(ctx, BWTS_K_OTHER, p.count, 32 * p.count);
            zrl_segment_sums_kernel<<<dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, ctx->stream>>>(S, p.count, b.offs, d_flag);
        }
        HIPC(hipGetLastError());
        BWTS_TRY(read_small(ctx, SM_ZRL_FLAG, 1));
        if ((u32)ctx->h_small[SM_ZRL_FLAG] != 0) return BWTS_E_FORMAT;
    }
    if (any_coded) {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, n);
        HIPC(hipMemsetAsync(d_out, 0, n, ctx->stream));
    }
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, in_bytes, in_bytes + n);
        zrl_write_kernel<<<dim3(grid), dim3(256), 0, ctx->stream>>>(d_in, S, b.offs, d_out);
    }
    HIPC(hipGetLastError());
    return BWTS_OK;
}
