// ec.hip -- static order-0 rANS over 16 KiB tiles, the stage behind move-to-front (include/bwts_ec.h; the stream is stated there and in
// DESIGN section 13, tests/ec_model.py is its executable form; the arithmetic shared with the host is in ec_plan.h).
//
// One wave codes one tile, its 64 lanes the 64 interleaved rANS states; a workgroup is four consecutive tiles of one block, so the
// block's table is in LDS once per workgroup.  A call works on the tiles of all its segments at once: block b of the call belongs to
// segment bseg[b] (one input: the only one), and a workgroup finds its tiles from that.
//   encode: block histograms -> one wave per block normalises (u16 table for the stream, packed f, c and reciprocal for the encoder)
//           -> a counting pass of the encoder (words per tile) -> scan of the payload sizes -> the total goes to the host, which
//           refuses a stream that does not fit -> the same encoder again, now writing every word at its final place, backwards from the
//           end of its payload, together with header, tables and directory.  No slot arena and no compaction copy.
//   decode: the directory entries are gathered and scanned to offsets; the decoding workgroups validate what they use before they use
//           it (header, table sum, their own size against the stream's end, the last tile the sum of all sizes) and raise a flag.
// Every address the decoder forms comes from a value that was checked or clamped first: slots are masked to 12 bits, word indices are
// tested against the payload's word count, output positions are below the tile's length.
#include "internal.h"
#include "device_utils.h"
#include "scan_templ.h"
#include "ec_plan.h"
#include "../../include/bwts_ec.h"

#define EC_BAD_HEADER 1u
#define EC_BAD_TABLE 2u
#define EC_BAD_DIRECTORY 4u
#define EC_BAD_PAYLOAD 8u

// the segments of a call as the kernels see them; seg_off == null: one input of n bytes (its stream, for the decoder, stream_bytes long)
struct EcSegs {
    const u64 *seg_off;     // [count + 1] where every segment's bytes start
    const u64 *first;       // [count] first tile | first block << 32, counted over the call
    const u64 *base;        // [count + 1] encode: bytes of the fixed parts of all earlier segments; decode: where the segment's stream starts
    const u32 *bseg;        // [blocks] the segment of every block
    u64 n, stream_bytes;
};

struct EcBlock { u64 in_off, len, jb, first_tile, base, base_next; };

__device__ __forceinline__ EcBlock ec_block(const EcSegs &S, u64 b)
{
    EcBlock R;
    if (!S.seg_off) {
        R.in_off = 0; R.len = S.n; R.jb = b; R.first_tile = 0; R.base = 0; R.base_next = S.stream_bytes;
        return R;
    }
    const u64 s = S.bseg[b], a = S.seg_off[s], w = S.first[s];
    R.in_off = a; R.len = S.seg_off[s + 1] - a; R.first_tile = w & 0xffffffffull; R.jb = b - (w >> 32);
    R.base = S.base[s]; R.base_next = S.base[s + 1];
    return R;
}

// lanes below mine among those of mask
__device__ __forceinline__ u32 ec_rank_in(u64 mask) { return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u)); }

// ------------------------------------------------------------------------------------
// tables
// ------------------------------------------------------------------------------------
// bseg of a segmented call (unit_table_kernel): the segment's number over its blocks
struct EcBlockTable {
    const u64 *seg_off, *first_words;
    u32 *bseg;
    __device__ u64 first(u64 s) const { return first_words[s] >> 32; }
    __device__ u64 units(u64 s) const { return ec_blocks(ec_tiles(seg_off[s + 1] - seg_off[s])); }
    __device__ void store(u64 s, u64 first, u64, u64 j) const { bseg[first + j] = (u32)s; }
};

// Byte counts of one block (256 KiB of one segment) per workgroup.  Ranks are mostly zeros: every thread adds a run's length when
// the run ends, not one per byte, into its wave's own 256 counters.
__device__ __forceinline__ void ec_count(u32 *bins, u32 &cur, u32 &cnt, u32 c)
{
    if (c == cur) { cnt++; return; }
    if (cnt) atomicAdd(&bins[cur], cnt);
    cur = c;
    cnt = 1;
}

__global__ __launch_bounds__(256) void ec_hist_kernel(const u8 *__restrict__ in, EcSegs S, u32 *__restrict__ hist)
{
    __shared__ u32 h[4][256];
    const u32 tid = threadIdx.x;
    const u64 b = blockIdx.x;
    const EcBlock R = ec_block(S, b);
    const u64 begin = R.jb * ((u64)EC_K << EC_LOG_T);
    const u32 len = (u32)(R.len - begin < ((u64)EC_K << EC_LOG_T) ? R.len - begin : ((u64)EC_K << EC_LOG_T));
    const u8 *p = in + R.in_off + begin;
#pragma unroll
    for (int w = 0; w < 4; w++) h[w][tid] = 0;
    __syncthreads();
    u32 *bins = h[wave_id()];
    u32 cur = 0, cnt = 0;
    u32 head = (16u - (u32)((uintptr_t)p & 15)) & 15u;
    if (head > len) head = len;
    const u32 vecs = (len - head) / 16, done = head + vecs * 16;
    for (u32 v = tid; v < vecs; v += 256) {
        const uint4 q = ((const uint4 *)(p + head))[v];
        const u32 qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 16; k++) ec_count(bins, cur, cnt, (qw[k >> 2] >> (8 * (k & 3))) & 255u);
    }
    if (tid < head) ec_count(bins, cur, cnt, p[tid]);
    if (tid < len - done) ec_count(bins, cur, cnt, p[done + tid]);
    if (cnt) atomicAdd(&bins[cur], cnt);
    __syncthreads();
    hist[b * 256 + tid] = h[0][tid] + h[1][tid] + h[2][tid] + h[3][tid];
}

// One wave per block: counts -> frequencies (ec_normalise of ec_plan.h is the serial statement), lane l holding symbols 4l .. 4l+3.
// The largest f, lowest symbol on ties, is the wave maximum of f << 8 | 255 - s.
__global__ __launch_bounds__(64) void ec_normalise_kernel(const u32 *__restrict__ hist, u16 *__restrict__ tab16, uint2 *__restrict__ etab)
{
    const u64 b = blockIdx.x;
    const u32 lane = (u32)lane_id();
    const uint4 hv = ((const uint4 *)(hist + b * 256))[lane];
    const u32 h[4] = {hv.x, hv.y, hv.z, hv.w};
    const u32 m = wave_reduce(h[0] + h[1] + h[2] + h[3], OpAdd());      // at most 2^18: h << 12 fits 32 bits
    u32 f[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const u32 v = h[i] ? (h[i] << EC_PROB_BITS) / m : 0u;
        f[i] = h[i] && v == 0 ? 1u : v;
    }
    int d = (int)EC_M - (int)wave_reduce(f[0] + f[1] + f[2] + f[3], OpAdd());
    while (d != 0) {
        u32 key = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const u32 k = f[i] << 8 | (255u - (4u * lane + (u32)i));
            key = k > key ? k : key;
        }
        const u32 s = 255u - (wave_reduce(key, OpMax()) & 255u);
        const int step = d > 0 ? d : -1;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (4u * lane + (u32)i == s) f[i] = (u32)((int)f[i] + step);
        d -= step;
    }
    const u32 mine = f[0] + f[1] + f[2] + f[3];
    u32 c = wave_scan_inclusive(mine, OpAdd()) - mine;
    ((uint2 *)(tab16 + b * 256))[lane] = make_uint2(f[0] | f[1] << 16, f[2] | f[3] << 16);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint2 e = make_uint2(0u, 0u);
        if (f[i]) {
            const ec_recip r = ec_recip_make(f[i]);
            e = make_uint2(f[i] | (c & 0xfffu) << 13 | r.sh1 << 25 | r.sh2 << 26, r.m);
        }
        etab[b * 256 + 4u * lane + (u32)i] = e;
        c += f[i];
    }
}

// ------------------------------------------------------------------------------------
// the encoder
// ------------------------------------------------------------------------------------
// The lane's 16 bytes of row r of a tile (zero where the tile has ended): one 16-byte load where the whole row exists and the tile's
// address allows, single bytes otherwise (a tile's last row, a segment that starts at an odd address).
__device__ __forceinline__ uint4 ec_load_row(const u8 *src, u32 r, u32 len, bool aligned, u32 lane)
{
    const u32 base = r * EC_ROW + lane * 16u;
    if (aligned && (r + 1u) * EC_ROW <= len) return *(const uint4 *)(src + base);
    u32 w[4] = {0u, 0u, 0u, 0u};
    const u32 nvalid = base >= len ? 0u : (len - base < 16u ? len - base : 16u);
#pragma unroll
    for (int k = 0; k < 16; k++)
        if ((u32)k < nvalid) w[k >> 2] |= (u32)src[base + (u32)k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// COUNT: the words every tile emits, nothing else.  Otherwise the stream: a tile's words from the end of its payload backwards (a
// step's words in ascending lane order in front of all earlier ones: the order the decoder reads), its states, padding and directory
// entry; the block's table by the workgroup of its first four tiles; the header with a segment's first tile.
template <bool COUNT>
__global__ __launch_bounds__(256) void ec_encode_kernel(const u8 *__restrict__ in, EcSegs S, const uint2 *__restrict__ etab, const u16 *__restrict__ tab16,
                                                        u32 *__restrict__ nwords, const u64 *__restrict__ offs, u8 *__restrict__ out)
{
    __shared__ uint2 tab[256];
    const u32 tid = threadIdx.x, lane = (u32)lane_id();
    const u64 b = blockIdx.x >> 2;
    const u32 quad = blockIdx.x & 3u;
    const EcBlock R = ec_block(S, b);
    const u64 nt = ec_tiles(R.len), j0 = R.jb * EC_K + quad * 4u;
    if (j0 >= nt) return;
    tab[tid] = etab[b * 256 + tid];
    u8 *stream = nullptr;
    if (!COUNT) {
        stream = out + R.base + offs[R.first_tile];
        if (quad == 0) ((u16 *)(stream + EC_HEADER_BYTES + (u64)EC_TABLE_BYTES * R.jb))[tid] = tab16[b * 256 + tid];
    }
    __syncthreads();
    const u64 j = j0 + (u64)wave_id();
    if (j >= nt) return;
    const u64 t = R.first_tile + j;
    const u32 len = ec_tile_len(R.len, j);
    const u8 *src = in + R.in_off + (j << EC_LOG_T);
    u8 *payload = nullptr;
    u16 *wp = nullptr;
    u32 nw = 0;
    if (!COUNT) {
        payload = stream + ec_fixed_bytes(R.len) + (offs[t] - offs[R.first_tile]);
        nw = nwords[t];
        wp = (u16 *)(payload + EC_STATE_BYTES) + nw;
    }
    const bool aligned = ((uintptr_t)src & 15) == 0;
    u32 x = EC_L, total = 0;
    uint4 next = ec_load_row(src, ec_rows(len) - 1u, len, aligned, lane);
    for (u32 r = ec_rows(len); r-- > 0;) {
        const uint4 q = next;
        if (r > 0) next = ec_load_row(src, r - 1u, len, aligned, lane);
        const u32 base = r * EC_ROW + lane * 16u;
        const u32 nvalid = base >= len ? 0u : (len - base < 16u ? len - base : 16u);
        const u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 15; k >= 0; k--) {
            const bool active = (u32)k < nvalid;
            const uint2 e = tab[(w[k >> 2] >> (8 * (k & 3))) & 255u];
            const u32 f = e.x & 0x1fffu, c = (e.x >> 13) & 0xfffu;
            const bool emit = active && f < EC_M && x >= f << 20;
            const u64 mask = __ballot(emit);
            if (mask) {
                const u32 cnt = (u32)__popcll(mask);
                if (!COUNT) {
                    wp -= cnt;
                    if (emit) wp[ec_rank_in(mask)] = (u16)x;
                }
                total += cnt;
            }
            if (emit) x >>= 16;
            if (active) x = ec_encode_step(x, f, c, e.y, (e.x >> 25) & 1u, e.x >> 26);
        }
    }
    if (COUNT) {
        if (lane == 0) nwords[t] = total;
        return;
    }
    ((u32 *)payload)[lane] = x;
    const u32 size = ec_payload_bytes(nw);
    if (lane < (size - EC_STATE_BYTES) / 2u - nw) ((u16 *)(payload + EC_STATE_BYTES))[nw + lane] = 0;
    u32 *dir = (u32 *)(stream + EC_HEADER_BYTES + (u64)EC_TABLE_BYTES * ec_blocks(nt));
    if (lane == 0) dir[j] = size;
    if (j + 1 == nt && j + 1 + lane < ec_pad16(4u * nt) / 4u) dir[j + 1 + lane] = 0;
    if (j == 0 && lane < 4) ((u32 *)stream)[lane] = lane == 0 ? EC_MAGIC : lane == 1 ? EC_PARAMS : lane == 2 ? (u32)R.len : (u32)(R.len >> 32);
}

// the stream sizes of a segmented encode
__global__ __launch_bounds__(256) void ec_stream_sizes_kernel(const u64 *__restrict__ seg_off, const u64 *__restrict__ first, u64 count, const u64 *__restrict__ offs,
                                                              u64 *__restrict__ sizes)
{
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= count) return;
    const u64 len = seg_off[s + 1] - seg_off[s], ft = first[s] & 0xffffffffull;
    sizes[s] = ec_fixed_bytes(len) + offs[ft + ec_tiles(len)] - offs[ft];
}

// ------------------------------------------------------------------------------------
// the decoder
// ------------------------------------------------------------------------------------
// the directory entries of all segments, in tile order (the host has made sure that every stream holds its fixed parts)
__global__ __launch_bounds__(256) void ec_dir_gather_kernel(const u8 *__restrict__ in, EcSegs S, u64 blocks, u32 *__restrict__ dsz)
{
    const u64 b = (u64)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (b >= blocks) return;
    const EcBlock R = ec_block(S, b);
    const u64 nt = ec_tiles(R.len), j = R.jb * EC_K + (threadIdx.x & 15u);
    if (j >= nt) return;
    dsz[R.first_tile + j] = ((const u32 *)(in + R.base + EC_HEADER_BYTES + (u64)EC_TABLE_BYTES * ec_blocks(nt)))[j];
}

// slot -> symbol | (f - 1) << 8 | (slot - c) << 20: one LDS read per decoded symbol
__global__ __launch_bounds__(256) void ec_decode_kernel(const u8 *__restrict__ in, EcSegs S, const u64 *__restrict__ offs, u8 *__restrict__ out, u32 *__restrict__ err)
{
    __shared__ u32 slot[EC_M];
    __shared__ u32 cum[257];
    __shared__ u32 scan_tmp[4];
    const u32 tid = threadIdx.x, lane = (u32)lane_id();
    const u64 b = blockIdx.x >> 2;
    const u32 quad = blockIdx.x & 3u;
    const EcBlock R = ec_block(S, b);
    const u64 nt = ec_tiles(R.len), j0 = R.jb * EC_K + quad * 4u;
    if (j0 >= nt) return;
    const u8 *stream = in + R.base;
    const u64 fixed = ec_fixed_bytes(R.len), ptotal = R.base_next - R.base - fixed;
    if (j0 == 0 && tid == 0) {
        u64 n = 0;
        if (ec_header_parse(stream, &n) != 0 || n != R.len) atomicOr(err, EC_BAD_HEADER);
    }
    const u32 f = ((const u16 *)(stream + EC_HEADER_BYTES + (u64)EC_TABLE_BYTES * R.jb))[tid];
    u32 sum = 0;
    const u32 c = block_scan_exclusive<u32, OpAdd, 4>(f, OpAdd(), 0u, scan_tmp, &sum);
    if (sum != EC_M) {          // (the same in every thread)
        if (tid == 0) atomicOr(err, EC_BAD_TABLE);
        return;
    }
    cum[tid] = c;
    if (tid == 255) cum[256] = sum;
    __syncthreads();
#pragma unroll 4
    for (u32 i = 0; i < EC_M / 256u; i++) {
        const u32 sl = i * 256u + tid;
        u32 s = 0;
#pragma unroll
        for (u32 step = 128; step; step >>= 1)
            if (cum[s + step] <= sl) s += step;
        slot[sl] = s | (cum[s + 1] - cum[s] - 1u) << 8 | (sl - cum[s]) << 20;
    }
    __syncthreads();
    const u64 j = j0 + (u64)wave_id();
    if (j >= nt) return;
    const u64 t = R.first_tile + j;
    const u32 len = ec_tile_len(R.len, j);
    // where the payload lies, from the scanned directory: nothing of it is read before it is known to end inside the stream
    const u64 po = offs[t] - offs[R.first_tile], pe = offs[t + 1] - offs[R.first_tile];
    if (!ec_size_ok(pe - po, len) || pe > ptotal || (j + 1 == nt && pe != ptotal)) {
        if (lane == 0) atomicOr(err, EC_BAD_DIRECTORY);
        return;
    }
    if (j + 1 == nt) {
        const u32 *dir = (const u32 *)(stream + EC_HEADER_BYTES + (u64)EC_TABLE_BYTES * ec_blocks(nt));
        if (j + 1 + lane < ec_pad16(4u * nt) / 4u && dir[j + 1 + lane] != 0) atomicOr(err, EC_BAD_DIRECTORY);
    }
    const u32 size = (u32)(pe - po), navail = (size - EC_STATE_BYTES) / 2u;
    const u8 *payload = stream + fixed + po;
    const u16 *words = (const u16 *)(payload + EC_STATE_BYTES);
    u8 *dst = out + R.in_off + (j << EC_LOG_T);
    const bool aligned = ((uintptr_t)dst & 15) == 0;
    u32 x = ((const u32 *)payload)[lane], rp = 0;
    bool bad = false;
    const u32 rows = ec_rows(len);
    for (u32 r = 0; r < rows; r++) {
        const u32 base = r * EC_ROW + lane * 16u;
        const u32 nvalid = base >= len ? 0u : (len - base < 16u ? len - base : 16u);
        u32 w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const bool active = (u32)k < nvalid;
            if (active) {
                const u32 e = slot[x & (EC_M - 1u)];
                x = (((e >> 8) & 0xfffu) + 1u) * (x >> EC_PROB_BITS) + (e >> 20);
                w[k >> 2] |= (e & 255u) << (8 * (k & 3));
            }
            const bool need = active && x < EC_L;
            const u64 mask = __ballot(need);
            if (mask) {
                const u32 idx = rp + ec_rank_in(mask);
                if (need) {
                    if (idx < navail) x = x << 16 | (u32)words[idx];
                    else bad = true;
                }
                rp += (u32)__popcll(mask);
            }
        }
        if (aligned && (r + 1u) * EC_ROW <= len) {
            *(uint4 *)(dst + base) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++)
                if ((u32)k < nvalid) dst[base + (u32)k] = (u8)(w[k >> 2] >> (8 * (k & 3)));
        }
    }
    // every lane back at L, all words taken, and zeros behind them
    bool wrong = bad || x != EC_L || rp > navail || ec_payload_bytes(rp) != size;
    if (!wrong && lane < navail - rp && words[rp + lane] != 0) wrong = true;
    if (__ballot(wrong) && lane == 0) atomicOr(err, EC_BAD_PAYLOAD);
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
struct EcSizeIn {
    const u32 *v;
    u64 nt;
    bool words;     // v holds words per tile (encode) or payload sizes as the directory gives them (decode)
    __device__ __forceinline__ u64 operator()(u64 i) const
    {
        if (i >= nt) return 0;
        const u32 x = v[i];
        return words ? (u64)ec_payload_bytes(x) : (u64)x;
    }
};

struct EcOffOut {
    u64 *offs;
    u64 nt;
    u64 *total;
    __device__ __forceinline__ void operator()(u64 i, u64 v) const
    {
        offs[i] = v;
        if (i == nt) *total = v;
    }
};

// how a call is cut: tiles and blocks over all its segments, and per segment where its tiles and blocks start
struct EcPlan {
    u64 count, tiles, blocks, fixed, least;
    std::vector<u64> words;      // segmented: first[count], then base[count + 1]
};

// The cut at the coder's two units (a block of K tiles of one segment is the same cut at K T bytes), and the byte arithmetic over it.
// base: encode: the fixed parts of the earlier segments; decode: the streams' starts (stream_bytes given)
static int ec_plan_call(const bwts_ctx *ctx, u64 n, SegMode segs, const u64 *stream_bytes, EcPlan &p)
{
    const StageCut cut = stage_cut_call(ctx, segs, n, EC_T, (u64)EC_T << EC_LOG_K);
    const std::vector<u64> &tile = cut.first[0], &block = cut.first[1];
    p.count = cut.count; p.tiles = cut.units[0]; p.blocks = cut.units[1];
    p.fixed = p.least = 0;
    if (segs.table()) p.words.resize((size_t)(2 * p.count + 1));
    u64 at = 0;
    for (u64 s = 0; s < p.count; s++) {
        const u64 len = segs.table() ? ctx->seg_off[s + 1] - ctx->seg_off[s] : n;
        if (segs.table()) {
            p.words[s] = tile[s] | block[s] << 32;
            p.words[p.count + s] = stream_bytes ? at : p.fixed;
        }
        if (stream_bytes) {
            const u64 sb = stream_bytes[s];
            if ((sb & 15) || sb < ec_least_bytes(len) || sb > ec_bound_bytes(len)) return BWTS_E_FORMAT;
            at += sb;
        }
        p.fixed += ec_fixed_bytes(len);
        p.least += ec_least_bytes(len);
        if (tile[s + 1] >= (1ull << 31) || block[s + 1] >= (1ull << 29)) return BWTS_E_RANGE;
    }
    if (segs.table()) p.words[2 * p.count] = stream_bytes ? at : p.fixed;
    return BWTS_OK;
}

struct EcBufs {
    u32 *hist, *per_tile, *bseg;
    uint2 *etab;
    u16 *tab16;
    u64 *offs, *ssize;
    void *scan_temp;
    void declare(BlockLayout &L, const EcPlan &p, bool encode, bool segments)
    {
        L.array(&per_tile, p.tiles); L.array(&offs, p.tiles + 1); L.raw(&scan_temp, scan_temp_bytes_t(p.tiles + 1, sizeof(u64)));
        if (encode) { L.array(&hist, p.blocks * 256); L.array(&etab, p.blocks * 256); L.array(&tab16, p.blocks * 256); }
        if (segments) L.array(&bseg, p.blocks);
        if (segments && encode) L.array(&ssize, p.count);
    }
};

void bwts_ec_plan(u64 n, u64 out[5])
{
    const StageCut cut = stage_cut_single(n, EC_T, (u64)EC_T << EC_LOG_K);
    out[0] = EC_T; out[1] = EC_K; out[2] = cut.units[0]; out[3] = cut.units[1]; out[4] = ec_bound_bytes(n);
}

static unsigned ec_grid(u64 blocks) { return (unsigned)blocks; }      // (ec_plan_call keeps 4 blocks below 2^31)

// what both directions do first: the arena, and for segments the two tables
static int ec_prepare(bwts_ctx *ctx, const EcPlan &p, bool encode, bool segments, u64 n, EcBufs &b, EcSegs &S)
{
    BlockLayout L;
    b.declare(L, p, encode, segments);
    BWTS_TRY(arena_take(ctx, L));
    S = EcSegs{nullptr, nullptr, nullptr, nullptr, n, 0};
    if (segments) {
        u64 *d_words = nullptr;
        BWTS_TRY(seg_upload_extra(ctx, p.words.data(), 2 * p.count + 1, &d_words));
        S.seg_off = d_seg_off(ctx); S.first = d_words; S.base = d_words + p.count; S.bseg = b.bseg;
        SpanGuard sp(ctx, BWTS_K_OTHER, p.blocks, 4 * p.blocks);
        unit_table_launch(ctx->stream, p.count, EcBlockTable{S.seg_off, S.first, b.bseg});
    }
    return BWTS_OK;
}

static int ec_scan_sizes(bwts_ctx *ctx, const EcPlan &p, const EcBufs &b, bool words, u64 *d_total)
{
    SpanGuard sp(ctx, BWTS_K_OTHER, p.tiles, 12 * p.tiles);
    return device_scan<false, u64>(ctx, p.tiles + 1, EcSizeIn{b.per_tile, p.tiles, words}, EcOffOut{b.offs, p.tiles, d_total}, OpAdd(), (u64)0, b.scan_temp);
}

// sizes: the bytes of the one input's stream, or of every segment's (sizes[count])
int ec_encode_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, u64 out_cap, SegMode segs, u64 *sizes)
{
    const bool segments = segs.table();
    EcPlan p;
    BWTS_TRY(ec_plan_call(ctx, n, segs, nullptr, p));
    if (out_cap < p.least) return BWTS_E_SPACE;
    EcBufs b;
    EcSegs S;
    BWTS_TRY(ec_prepare(ctx, p, true, segments, n, b, S));
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, n);
        ec_hist_kernel<<<dim3(ec_grid(p.blocks)), dim3(256), 0, ctx->stream>>>(d_in, S, b.hist);
    }
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, p.blocks * 256, p.blocks * 3584);
        ec_normalise_kernel<<<dim3(ec_grid(p.blocks)), dim3(64), 0, ctx->stream>>>(b.hist, b.tab16, b.etab);
    }
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, n);
        ec_encode_kernel<true><<<dim3(ec_grid(4 * p.blocks)), dim3(256), 0, ctx->stream>>>(d_in, S, b.etab, b.tab16, b.per_tile, b.offs, d_out);
    }
    BWTS_TRY(ec_scan_sizes(ctx, p, b, true, ctx->d_small + SM_EC_TOTAL));
    HIPC(hipGetLastError());
    BWTS_TRY(read_small(ctx, SM_EC_TOTAL, 1));
    const u64 total = p.fixed + ctx->h_small[SM_EC_TOTAL];
    if (total > out_cap) return BWTS_E_SPACE;
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, n + total);
        ec_encode_kernel<false><<<dim3(ec_grid(4 * p.blocks)), dim3(256), 0, ctx->stream>>>(d_in, S, b.etab, b.tab16, b.per_tile, b.offs, d_out);
    }
    if (segments) {
        {
            SpanGuard sp(ctx, BWTS_K_OTHER, p.count, 24 * p.count);
            ec_stream_sizes_kernel<<<dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, ctx->stream>>>(d_seg_off(ctx), S.first, p.count, b.offs, b.ssize);
        }
        HIPC(hipMemcpyAsync(sizes, b.ssize, p.count * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
        HIPC(hipStreamSynchronize(ctx->stream));
    } else {
        *sizes = total;
    }
    HIPC(hipGetLastError());
    return BWTS_OK;
}

// one stream of in_bytes (its n goes to *n_out, and must not exceed out_cap; stream_bytes is not read) or one per segment of the
// context's table, stream_bytes[count], whose lengths the headers must repeat
int ec_decode_impl(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, u8 *d_out, u64 out_cap, u64 *n_out, SegMode segs, const u64 *stream_bytes)
{
    const bool segments = segs.table();
    u64 n = in_bytes;       // segmented: the sum of the lengths
    if (!segments) {
        if (in_bytes < EC_HEADER_BYTES || (in_bytes & 15)) return BWTS_E_FORMAT;
        HIPC(hipMemcpyAsync(ctx->h_small + SM_EC_HEAD, d_in, EC_HEADER_BYTES, hipMemcpyDeviceToHost, ctx->stream));
        HIPC(hipStreamSynchronize(ctx->stream));
        if (ec_header_parse((const u8 *)(ctx->h_small + SM_EC_HEAD), &n) != 0) return BWTS_E_FORMAT;
        if (n > EC_MAX_N) return BWTS_E_RANGE;
        if (n > out_cap) return BWTS_E_SPACE;
        if (in_bytes < ec_least_bytes(n) || in_bytes > ec_bound_bytes(n)) return BWTS_E_FORMAT;
        ctx->tm.n = n;
    }
    EcPlan p;
    BWTS_TRY(ec_plan_call(ctx, n, segs, segments ? stream_bytes : nullptr, p));
    EcBufs b;
    EcSegs S;
    BWTS_TRY(ec_prepare(ctx, p, false, segments, n, b, S));
    S.stream_bytes = in_bytes;
    u32 *d_flag = (u32 *)(ctx->d_small + SM_EC_FLAG);
    HIPC(hipMemsetAsync(d_flag, 0, sizeof(u64), ctx->stream));
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, p.tiles, 8 * p.tiles);
        ec_dir_gather_kernel<<<dim3((unsigned)((p.blocks + 15) / 16)), dim3(256), 0, ctx->stream>>>(d_in, S, p.blocks, b.per_tile);
    }
    BWTS_TRY(ec_scan_sizes(ctx, p, b, false, ctx->d_small + SM_EC_TOTAL));
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, 2 * n);
        ec_decode_kernel<<<dim3(ec_grid(4 * p.blocks)), dim3(256), 0, ctx->stream>>>(d_in, S, b.offs, d_out, d_flag);
    }
    HIPC(hipGetLastError());
    BWTS_TRY(read_small(ctx, SM_EC_FLAG, 1));
    if ((u32)ctx->h_small[SM_EC_FLAG] != 0) return BWTS_E_FORMAT;
    if (n_out) *n_out = n;
    return BWTS_OK;
}
