// forward.hip -- BWTS forward transform on the GPU.
//
// Replaces divsufsort() + make_bwts_sa() + move_lyndonword_head()
// (/root/reference/mk_bwts_sa.c:48, :114-195, :74-112).  Instead of suffix-sorting and then
// patching SA/ISA sequentially, the engine
//   1. finds the Lyndon factors.  The reference reads them off the suffix array as the strict
//      prefix minima of ISA (mk_bwts_sa.c:126-129); the fast path here gets the same set without
//      a suffix sort: a device-wide prefix-min over packed m-symbol keys leaves a handful of
//      candidates, which one workgroup settles with exact suffix comparisons.  Inputs with too
//      many candidates (a^n, (ab)^n ...) take the general path: suffix sort + prefix-min of ISA;
//   2. sorts all positions directly by their infinite cyclic word rot(p)^omega with prefix
//      doubling on a CYCLIC successor (no fix-up needed: the result IS the fixed-up order);
//   3. emits bwts[r] = T[cprev(sa[r])] (mk_bwts_sa.c:172-188) as a gather.
// All index work is u32 with u64 loop bounds; bytes are unsigned.
#include "internal.h"
#include "device_utils.h"
#include "scan_templ.h"
#include "key_plan.h"
#include "../../include/bwts_test.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

// ------------------------------------------------------------------------------------
// small-word layout in ctx->d_small / h_small (u64 words)
// ------------------------------------------------------------------------------------
#define SM_HIST      0      // 256 words: byte histogram
#define SM_CODES     256    // 32 words = 256 bytes: byte -> symbol code
#define SM_COUNTERS  320    // scratch counters
#define   CNT_ACTIVE   (SM_COUNTERS + 0)
#define   CNT_SPLITS   (SM_COUNTERS + 1)
#define   CNT_TOTAL    (SM_COUNTERS + 2)
#define   CNT_CAND     (SM_COUNTERS + 4)
#define   CNT_LYN_K    (SM_COUNTERS + 5)
#define   CNT_LYN_OVF  (SM_COUNTERS + 6)

#define SM_DGCNT  2816      // 8 + 1024 words: counters of the group-local dense rounds (dense_round_kernel)
#define SM_SEGCNT 2560      // 256 words: large-group element counts of seg_small_sort_kernel (spread: one address would serialise)
#define SM_VTAB 2048        // 256 words: (length << 32) | code of each byte value (variable-length codes)

// ------------------------------------------------------------------------------------
// byte histogram (also used by the inverse: unbwts.c:34-36)
// ------------------------------------------------------------------------------------
// 16 copies of the bins, picked by the lane id: on skewed text a quarter of a wave's lanes would otherwise hit the same
// counter in one LDS instruction and serialise
#define BH_COPIES 16
__global__ __launch_bounds__(256) void byte_hist_kernel(const u8 *__restrict__ T, u64 n, u64 *__restrict__ hist)
{
    __shared__ u32 bins[BH_COPIES][256];
    const int tid = threadIdx.x;
    u32 *mine = bins[tid & (BH_COPIES - 1)];
    for (int i = tid; i < BH_COPIES * 256; i += 256) ((u32 *)bins)[i] = 0;
    __syncthreads();
    // 16 bytes per thread per step when aligned; tail and head handled bytewise
    const u64 nvec = n / 16;
    const uint4 *T16 = (const uint4 *)T;   // hipMalloc'd / arena pointers are 256-B aligned
    const bool aligned = ((uintptr_t)T & 15) == 0;
    if (aligned) {
        for (u64 v = (u64)blockIdx.x * 256 + tid; v < nvec; v += (u64)gridDim.x * 256) {
            const uint4 q = T16[v];
            const u32 ws[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int a = 0; a < 4; a++) {
#pragma unroll
                for (int b = 0; b < 4; b++) atomicAdd(&mine[(ws[a] >> (8 * b)) & 255u], 1u);
            }
        }
        for (u64 i = nvec * 16 + (u64)blockIdx.x * 256 + tid; i < n; i += (u64)gridDim.x * 256) atomicAdd(&mine[T[i]], 1u);
    } else {
        for (u64 i = (u64)blockIdx.x * 256 + tid; i < n; i += (u64)gridDim.x * 256) atomicAdd(&mine[T[i]], 1u);
    }
    __syncthreads();
    u32 s = 0;
#pragma unroll
    for (int c = 0; c < BH_COPIES; c++) s += bins[c][tid];
    if (s) atomicAdd((unsigned long long *)&hist[tid], (unsigned long long)s);
}

int byte_histogram_device(bwts_ctx *ctx, const u8 *d_T, u64 n, u64 *d_hist256)
{
    HIPC(hipMemsetAsync(d_hist256, 0, 256 * sizeof(u64), ctx->stream));
    u64 blocks = (n + 256 * 64 - 1) / (256 * 64);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    SpanGuard g(ctx, BWTS_K_HISTOGRAM, n, n);
    byte_hist_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(d_T, n, d_hist256);
    HIPC(hipGetLastError());
    return BWTS_OK;
}

// the byte histogram of the text, in h_small[SM_HIST ..]
static int read_histogram(bwts_ctx *ctx, const u8 *d_T, u64 n)
{
    BWTS_TRY(byte_histogram_device(ctx, d_T, n, ctx->d_small + SM_HIST));
    return read_small(ctx, SM_HIST, 256);
}

#define KEY_SAMPLES (1u << 17)
#define CNT_SAMPLE (SM_COUNTERS + 16)      // 5 words: adjacent sample keys agreeing on their first 24/32/40/48/56 bits
__global__ void sample_keys_kernel(const u8 *T, u64 n, const u64 *vtab, u32 samples, u64 *out);
__global__ void count_prefix_matches_kernel(const u64 *keys, u32 samples, unsigned long long *counters);

// The model knows nothing about repeated phrases.  Where the input is large enough to matter, sort the keys
// of 2^17 sampled positions and count neighbours that agree on their first B bits: if the sample shows
// clearly more ties than the model allows, take the empirical figure (real text wants the full 64 bits).
// scratch: the round-0 sort buffers, free at that point; vtab: the code table in h_small.  The only part that launches kernels.
// partners_of[b] (b = 32, 40, 48, 56): the equal keys of b bits a position is expected to meet, by the sample where it saw enough, else by the model.
static int sampled_key_bits(bwts_ctx *ctx, const u8 *d_T, u64 n, const SortBufs &scratch, const u64 *vtab, const double share[65], int *kb_emp,
                            double partners_of[65])
{
    HIPC(hipMemcpyAsync(ctx->d_small + SM_VTAB, vtab, 256 * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemsetAsync(ctx->d_small + CNT_SAMPLE, 0, 8 * sizeof(u64), ctx->stream));
    SpanGuard g(ctx, BWTS_K_KEYBUILD, KEY_SAMPLES, 0);
    sample_keys_kernel<<<dim3(KEY_SAMPLES / 256), dim3(256), 0, ctx->stream>>>(d_T, n, ctx->d_small + SM_VTAB, KEY_SAMPLES, scratch.keys[0]);
    int sres = 0;
    BWTS_TRY(radix_sort_pairs(ctx, scratch.plan(), KEY_SAMPLES, 64, &sres));
    count_prefix_matches_kernel<<<dim3(KEY_SAMPLES / 256), dim3(256), 0, ctx->stream>>>(
        scratch.keys[sres], KEY_SAMPLES, (unsigned long long *)(ctx->d_small + CNT_SAMPLE));
    HIPC(hipGetLastError());
    BWTS_TRY(read_small(ctx, CNT_SAMPLE, 5));
    const double pairs = 0.5 * (double)KEY_SAMPLES * (double)KEY_SAMPLES;
    *kb_emp = 64;
    for (int b = 32, w = 1; b <= 56; b += 8, w++) {
        const double m = (double)ctx->h_small[CNT_SAMPLE + w];
        const double partners = m >= 8.0 ? (double)n * m / pairs : (double)n * share[b];   // few hits: trust the model
        partners_of[b] = partners;
        if (*kb_emp == 64 && key_few_ties(partners)) *kb_emp = b;
    }
    return BWTS_OK;
}

// The alphabet and the round-0 key of a sort, from the histogram in h_small: key_plan.h decides, this adds the sampled measurement
// (it needs both d_T and scratch) and the copies to the device.
static int set_alphabet(bwts_ctx *ctx, bool reserve_pad, u64 n, Alphabet *al, const u8 *d_T = nullptr, const SortBufs *scratch = nullptr)
{
    const u64 *hist = ctx->h_small + SM_HIST;
    KeyKnobs knobs;
    knobs.key_symbols = key_knob_int(bwts_knob(ctx, "BWTS_KEY_SYMBOLS"));
    knobs.varlen = key_knob_varlen(bwts_knob(ctx, "BWTS_VARLEN"));
    knobs.key_bits = key_knob_int(bwts_knob(ctx, "BWTS_KEY_BITS"));
    KeyPlan P;
    key_plan_begin(hist, n, reserve_pad, knobs, &P);
    KeySample sample;
    u64 *vtab = ctx->h_small + SM_VTAB;          // (length << 32) | code of each byte value
    if (P.code_built) {
        memcpy(vtab, P.vtab, sizeof P.vtab);
        if (d_T && scratch && n >= (1ull << 22)) BWTS_TRY(sampled_key_bits(ctx, d_T, n, *scratch, vtab, P.share, &sample.kb_emp, sample.partners_of));
    }
    key_plan_finish(&P, sample);
    *al = P.al;
    if (al->varlen) HIPC(hipMemcpyAsync(ctx->d_small + SM_VTAB, vtab, 256 * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    memcpy(ctx->h_small + SM_CODES, P.codes, 256);
    HIPC(hipMemcpyAsync(ctx->d_small + SM_CODES, ctx->h_small + SM_CODES, 256, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));   // h_small is reused by later read-backs
    return BWTS_OK;
}

// ------------------------------------------------------------------------------------
// factor lookup: fstart[0..k) sorted factor starts, factor f = [fstart[f], f+1<k ? fstart[f+1] : n)
// ------------------------------------------------------------------------------------
__device__ __forceinline__ u64 factor_of(const u32 *__restrict__ fstart, u64 k, u64 p)
{
    u64 lo = 0, hi = k - 1;
    while (lo < hi) {
        const u64 mid = (lo + hi + 1) >> 1;
        if ((u64)fstart[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ u64 factor_end(const u32 *__restrict__ fstart, u64 k, u64 n, u64 f)
{
    return f + 1 < k ? (u64)fstart[f + 1] : n;
}

// ------------------------------------------------------------------------------------
// round 0: key[p] = first msym symbols of the suffix at p (zero-filled past the end), value = p
// Round-0 keys in original order.  Wide: one u64 each.  Split: when the packed sort will take them (at most 40 bits,
// radix_packed_applicable()), keybuild writes the two streams the packed passes travel with --
//   lo  u32  key bits 0..31
//   c   u16  key bits 32..39 | carried byte << 8      (c16)      or  u8: the carried byte alone (keys of <= 32 bits)
// where the carried byte of position p is T[cprev(p)] (mk_bwts_sa.c:172-188): T[p-1], fixed at factor heads afterwards.
// The first pass then reads 6 (5) bytes per element like any other pass, and no separate previous-symbol array exists.
struct KeyStore { u64 *wide; u32 *lo; u8 *c; bool c16; u8 *wprev; /* beside wide keys: the carried bytes, or null */ };
__device__ __forceinline__ void ks_store(const KeyStore &ks, u64 i, u64 key)        // the key only (patches)
{
    if (ks.wide) ks.wide[i] = key;
    else { ks.lo[i] = (u32)key; if (ks.c16) ks.c[2 * i] = (u8)(key >> 32); }
}
__device__ __forceinline__ void ks_store_with_prev(const KeyStore &ks, u64 i, u64 key, u32 prev)   // key + carried byte (keybuild)
{
    if (ks.wide) { ks.wide[i] = key; if (ks.wprev) ks.wprev[i] = (u8)prev; }
    else {
        ks.lo[i] = (u32)key;
        if (ks.c16) ((u16 *)ks.c)[i] = (u16)(((u32)(key >> 32) & 255u) | (prev << 8));
        else ks.c[i] = (u8)prev;
    }
}
__device__ __forceinline__ u64 ks_load(const KeyStore &ks, u64 i)
{
    return ks.wide ? ks.wide[i] : ((u64)ks.lo[i] | (ks.c16 ? (u64)ks.c[2 * i] << 32 : 0ull));
}
static KeyStore key_store_of(u64 *keys0, u64 n, bool split, int key_bits)
{
    KeyStore ks;
    ks.wide = split ? nullptr : keys0;
    ks.lo = (u32 *)keys0;
    ks.c = (u8 *)keys0 + align_up((size_t)n * 4, 256);
    ks.c16 = key_bits > 32;
    ks.wprev = nullptr;
    return ks;
}
// the carried byte of a factor's first position is the factor's last byte
__global__ __launch_bounds__(256) void carried_head_fix_kernel(const u8 *__restrict__ T, u64 n, const u32 *__restrict__ fstart, u64 k, KeyStore ks);

// ------------------------------------------------------------------------------------
#define KB_THREADS 256
#define KB_ITEMS   8
#define KB_TILE    (KB_THREADS * KB_ITEMS)
#define KB_HALO    64

// The value array of round 0 is the identity and is never written: the first radix pass uses the element index.
// pos0 / lim: the launch covers positions [pos0, lim) (pos0 a multiple of KB_TILE) and stores the key of position q at index
// q - pos0, tile minima at tile - pos0 / KB_TILE: the wide path (n > 2^32) materialises keys one segment at a time.
// A workgroup builds the KB_SUB tiles of one radix tile (KB_RX_TILE positions) one after the other.  hist0 (may be null; only with
// pos0 = 0): it also counts the key's bits 0..7 -- the first radix pass's digit -- and leaves the radix tile's row of that pass's
// [tile][digit] table, so the pass needs no sweep of its own over the keys (SortPlan::first_hist).
#define KB_RX_TILE 8192                               // = the packed radix passes' tile (radix.hip)
#define KB_SUB     (KB_RX_TILE / KB_TILE)
__device__ __forceinline__ void kb_hist_clear(u32 (*bins)[256])
{
    for (int i = threadIdx.x; i < KB_THREADS / 64 * 256; i += KB_THREADS) ((u32 *)bins)[i] = 0;
}
__device__ __forceinline__ void kb_hist_flush(u32 (*bins)[256], u32 *__restrict__ hist0)
{
    __syncthreads();
    u32 s = 0;
#pragma unroll
    for (int w = 0; w < KB_THREADS / 64; w++) s += bins[w][threadIdx.x];
    hist0[(u64)blockIdx.x * 256 + threadIdx.x] = s;
}
static_assert(KB_THREADS == 256, "one thread per digit of the first pass's table row");

__global__ __launch_bounds__(KB_THREADS) void keybuild0_kernel(const u8 *__restrict__ T, u64 n, const u8 *__restrict__ codes_g,
                                                               int bits, int msym, int pad_add,
                                                               KeyStore keys, u64 *__restrict__ tile_min /* may be null */, u64 pos0, u64 lim,
                                                               u32 *__restrict__ hist0)
{
    __shared__ u16 sc[KB_TILE + KB_HALO + 16];
    __shared__ u64 skey[KB_TILE + KB_TILE / 8];     // blocked -> striped transpose (one pad slot per 8)
    __shared__ u8 codes[256];
    __shared__ u64 wmin[KB_THREADS / 64];
    __shared__ __attribute__((aligned(16))) u8 sraw[KB_TILE + KB_HALO + 16];     // the tile's raw bytes (split keys: carried byte = T[q - 1])
    __shared__ u8 before_tile;
    __shared__ u32 bins[KB_THREADS / 64][256];

    const int tid = threadIdx.x;
    codes[tid] = codes_g[tid];
    if (hist0) kb_hist_clear(bins);
    const int key_bits = bits * msym;
    const u64 mask = key_bits >= 64 ? ~0ull : ((1ull << key_bits) - 1ull);

    for (int sub = 0; sub < KB_SUB; sub++) {
        const u64 tile = (u64)blockIdx.x * KB_SUB + (u64)sub;
        const u64 base = pos0 + tile * KB_TILE;
        if (base >= lim) break;
        const u64 end = base + KB_TILE < lim ? base + KB_TILE : lim;
        __syncthreads();                                // (the previous tile's readers of the LDS arrays are done)
        if (tid == 0) before_tile = base ? T[base - 1] : T[n - 1];

        // symbol codes of the tile and its halo; past the end of the text the code is 0.  16 bytes per lane
        // where the text allows it (tile bases are multiples of 2048, device buffers are 16-byte aligned).
        const u32 span = (u32)(end - base) + (u32)msym;
        const bool vec_ok = ((uintptr_t)T & 15) == 0;
        for (u32 c = tid; c * 16 < span; c += KB_THREADS) {
            const u64 q0 = base + (u64)c * 16;
            if (vec_ok && q0 + 16 <= n) {
                const uint4 v = *(const uint4 *)(T + q0);
                *(uint4 *)(sraw + c * 16) = v;
                const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int bb = 0; bb < 4; bb++)
                        sc[c * 16 + a * 4 + bb] = (u16)((u32)codes[(w[a] >> (8 * bb)) & 255u] + (u32)pad_add);
            } else {
                for (int bb = 0; bb < 16; bb++) {
                    const u64 q = q0 + bb;
                    const u8 t = q < n ? T[q] : (u8)0;
                    sraw[c * 16 + bb] = t;
                    sc[c * 16 + bb] = q < n ? (u16)((u32)codes[t] + (u32)pad_add) : (u16)0;
                }
            }
        }
        __syncthreads();
        const u32 o = (u32)tid * KB_ITEMS;
        u64 lo = ~0ull;
        if (base + o < end) {
            u64 key = 0;
            for (int j = 0; j < msym; j++) key = (key << bits) | sc[o + j];
#pragma unroll
            for (int e = 0; e < KB_ITEMS; e++) {
                if (base + o + e < end) {
                    skey[o + e + ((o + e) >> 3)] = key;
                    lo = key < lo ? key : lo;
                    key = ((key << bits) | sc[o + e + msym]) & mask;   // stays inside the loaded span / halo
                }
            }
        }
        if (tile_min) {
            lo = wave_scan_inclusive(lo, OpMin());
            if (lane_id() == 63) wmin[wave_id()] = lo;
        }
        __syncthreads();
        // lane-consecutive (coalesced) key stores
#pragma unroll
        for (int j = 0; j < KB_ITEMS; j++) {
            const u32 e = (u32)j * KB_THREADS + tid;
            const bool valid = base + e < end;
            u64 key = 0;
            if (valid) {
                const u64 q = base + e;
                key = skey[e + (e >> 3)];
                const u32 prev = e ? (u32)sraw[e - 1] : (u32)before_tile;          // T[q - 1], from the tile already in LDS
                ks_store_with_prev(keys, q - pos0, key, prev);
            }
            if (hist0) hist_add_runs(bins[wave_id()], (u32)key & 255u, valid);
        }
        // smallest key of the tile: the Lyndon candidate search starts from these (same tile size as the scan)
        if (tile_min && tid == 0) {
            u64 t = wmin[0];
            for (int w = 1; w < KB_THREADS / 64; w++) t = wmin[w] < t ? wmin[w] : t;
            tile_min[tile] = t;
        }
    }
    if (hist0) kb_hist_flush(bins, hist0);
}

// ---- variable-length codes -------------------------------------------------------------------------------------
// key = the first key_bits bits of the concatenated code words starting at position q (right-aligned in the u64)
__device__ __forceinline__ u64 vl_key_plain(const u8 *__restrict__ T, u64 n, const u64 *__restrict__ vtab, int key_bits, u64 q)
{
    u64 acc = 0;
    int filled = 0;
    while (filled < key_bits) {
        if (q >= n) { acc <<= (key_bits - filled); break; }         // past the text: zero bits
        const u64 e = vtab[T[q++]];
        const int l = (int)(e >> 32), room = key_bits - filled;
        const u64 c = (u32)e;
        if (l <= room) { acc = (acc << l) | c; filled += l; }
        else { acc = (acc << room) | (c >> (l - room)); filled = key_bits; }
    }
    return acc;
}
__device__ __forceinline__ u64 vl_key_cyclic(const u8 *__restrict__ T, const u64 *__restrict__ vtab, int key_bits, u64 q, u64 s, u64 e_)
{
    u64 acc = 0;
    int filled = 0;
    while (filled < key_bits) {
        const u64 e = vtab[T[q]];
        if (++q == e_) q = s;
        const int l = (int)(e >> 32), room = key_bits - filled;
        const u64 c = (u32)e;
        if (l <= room) { acc = (acc << l) | c; filled += l; }
        else { acc = (acc << room) | (c >> (l - room)); filled = key_bits; }
    }
    return acc;
}

// same key, for the common case that 16 text bytes from q lie inside the factor: one unaligned 16-byte read, table in LDS
struct __attribute__((packed, aligned(1))) TextChunk16 { u64 w[2]; };
__device__ __forceinline__ u64 vl_key_cyclic_fast(const u8 *__restrict__ T, const u64 *vtab_lds, const u64 *__restrict__ vtab_g, int key_bits,
                                                  u64 q, u64 s, u64 e_)
{
    if (q + 16 > e_) return vl_key_cyclic(T, vtab_g, key_bits, q, s, e_);
    const TextChunk16 ch = *(const TextChunk16 *)(T + q);
    u64 acc = 0;
    int filled = 0;
#pragma unroll
    for (int b = 0; b < 16; b++) {
        if (filled < key_bits) {
            const u32 sym = (u32)((b < 8 ? ch.w[0] >> (8 * b) : ch.w[1] >> (8 * (b - 8))) & 255u);
            const u64 e = vtab_lds[sym];
            const int l = (int)(e >> 32), room = key_bits - filled;
            const u64 c = (u32)e;
            if (l <= room) { acc = (acc << l) | c; filled += l; }
            else { acc = (acc << room) | (c >> (l - room)); filled = key_bits; }
        }
    }
    if (filled < key_bits) return vl_key_cyclic(T, vtab_g, key_bits, q, s, e_);     // codes shorter than 4 bits on average: rare
    return acc;
}

__global__ __launch_bounds__(256) void sample_keys_kernel(const u8 *__restrict__ T, u64 n, const u64 *__restrict__ vtab, u32 samples,
                                                          u64 *__restrict__ out)
{
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= samples) return;
    const u64 pos = (((u64)i * 0x9E3779B97F4A7C15ull) >> 11) % n;       // scattered, reproducible sample positions
    out[i] = vl_key_plain(T, n, vtab, 64, pos);
}
__global__ __launch_bounds__(256) void count_prefix_matches_kernel(const u64 *__restrict__ keys, u32 samples,
                                                                   unsigned long long *__restrict__ counters)
{
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    const bool ok = i > 0 && i < samples;
    const u64 a = ok ? keys[i] : 0, b = ok ? keys[i - 1] : ~0ull;
#pragma unroll
    for (int w = 0; w < 5; w++) {
        const int bits = 24 + 8 * w;
        const u64 m = __ballot(ok && (a >> (64 - bits)) == (b >> (64 - bits)));
        if (m && lane_id() == 0) atomicAdd(&counters[w], (unsigned long long)__popcll(m));
    }
}

// Round-0 keys from variable-length codes.  The tile's code words (tile + halo, KB_SYMS symbols) are laid out once as a
// bit stream in LDS -- per-thread serial prefix of the code lengths, a workgroup scan for the bit offsets, each word OR-ed
// in at its offset -- and the key of a position is the stream's first key_bits bits from that position's offset: a
// 64-bit window out of three stream words.  Symbols past the end of the text have length 0 (zero bits follow).
// (The first version kept a shifting 128-bit reservoir per thread: 118 VALU instructions per position, 91 % VALU busy.)
// Same outputs as keybuild0_kernel.
#define KB_SYMS      (KB_TILE + KB_HALO)                    // 2112
#define KB_SYM_PER   ((KB_SYMS + KB_THREADS - 1) / KB_THREADS)      // symbols a thread lays out: 9
#define KB_BS_WORDS  ((KB_SYMS * VL_MAXLEN + 31) / 32 + 4)   // stream words incl. zero padding for the last windows
__global__ __launch_bounds__(KB_THREADS) void keybuild0v_kernel(const u8 *__restrict__ T, u64 n, const u64 *__restrict__ vtab_g,
                                                                int key_bits, KeyStore keys, u64 *__restrict__ tile_min, u64 pos0, u64 lim,
                                                                u32 *__restrict__ hist0)
{
    __shared__ u64 vtab[256];
    __shared__ __attribute__((aligned(16))) u8 sb[KB_SYMS + 16];
    __shared__ u32 bs[KB_BS_WORDS];                 // bit stream, most significant bit of a word first
    __shared__ u16 symoff[KB_SYMS + 8];             // bit offset of every symbol's code word
    __shared__ u64 wmin[KB_THREADS / 64];
    __shared__ u32 scan_sm[KB_THREADS / 64];
    __shared__ u8 before_tile;                      // T[base - 1]: the carried byte of the tile's first position
    __shared__ u32 bins[KB_THREADS / 64][256];      // hist0: per-wave counts of the keys' bits 0..7

    const int tid = threadIdx.x;
    vtab[tid] = vtab_g[tid];
    if (hist0) kb_hist_clear(bins);
    for (int sub = 0; sub < KB_SUB; sub++) {
        const u64 tile = (u64)blockIdx.x * KB_SUB + (u64)sub;
        const u64 base = pos0 + tile * KB_TILE;
        if (base >= lim) break;
        const u64 end = base + KB_TILE < lim ? base + KB_TILE : lim;
        __syncthreads();                                // (the previous tile's readers of the LDS arrays are done)
        if (tid == 0) before_tile = base ? T[base - 1] : T[n - 1];
        const u32 span = KB_SYMS;
        const u64 avail = n - base;                                 // symbols of the text from the tile's start
        const u32 nvalid = avail < span ? (u32)avail : span;
        const bool vec_ok = ((uintptr_t)T & 15) == 0;
        for (u32 c = tid; c * 16 < span; c += KB_THREADS) {
            const u64 q0 = base + (u64)c * 16;
            if (vec_ok && q0 + 16 <= n) {
                *(uint4 *)(sb + c * 16) = *(const uint4 *)(T + q0);
            } else {
                for (int bb = 0; bb < 16; bb++) sb[c * 16 + bb] = q0 + bb < n ? T[q0 + bb] : (u8)0;
            }
        }
        for (u32 i = tid; i < KB_BS_WORDS; i += KB_THREADS) bs[i] = 0;
        __syncthreads();

        // lay out symbols [s0, s0 + KB_SYM_PER)
        const u32 s0 = (u32)tid * KB_SYM_PER;
        u32 ent_len[KB_SYM_PER], ent_code[KB_SYM_PER];
        u32 mine = 0;
#pragma unroll
        for (int i = 0; i < KB_SYM_PER; i++) {
            const u32 sidx = s0 + i;
            u64 ent = 0;
            if (sidx < nvalid) ent = vtab[sb[sidx]];            // past the text (or past the halo): length 0
            ent_len[i] = (u32)(ent >> 32);
            ent_code[i] = (u32)ent;
            mine += ent_len[i];
        }
        u32 total;
        u32 off = block_scan_exclusive<u32, OpAdd, KB_THREADS / 64>(mine, OpAdd(), 0u, scan_sm, &total);
#pragma unroll
        for (int i = 0; i < KB_SYM_PER; i++) {
            const u32 sidx = s0 + i;
            if (sidx < KB_SYMS) symoff[sidx] = (u16)off;
            const u32 l = ent_len[i];
            if (l) {
                const u32 wd = off >> 5, r = off & 31u;
                if (r + l <= 32) atomicOr(&bs[wd], ent_code[i] << (32 - r - l));
                else {
                    atomicOr(&bs[wd], ent_code[i] >> (r + l - 32));
                    atomicOr(&bs[wd + 1], ent_code[i] << (64 - r - l));
                }
            }
            off += l;
        }
        __syncthreads();

        // keys, lane-consecutive over the tile's positions (any thread can cut any position's window out of the stream):
        // coalesced stores straight from registers
        u64 lo = ~0ull;
#pragma unroll
        for (int j = 0; j < KB_ITEMS; j++) {
            const u32 e = (u32)j * KB_THREADS + tid;
            const bool valid = base + e < end;
            u64 key = 0;
            if (valid) {
                const u32 bo = symoff[e];
                const u32 wd = bo >> 5, r = bo & 31u;
                const u64 hi64 = ((u64)bs[wd] << 32) | (u64)bs[wd + 1];
                const u64 win = r ? (hi64 << r) | ((u64)bs[wd + 2] >> (32 - r)) : hi64;      // 64 stream bits from bo
                key = win >> (64 - key_bits);
                lo = key < lo ? key : lo;
                const u32 prev = e ? (u32)sb[e - 1] : (u32)before_tile;            // T[q - 1], from the tile already in LDS
                ks_store_with_prev(keys, base + e - pos0, key, prev);
            }
            if (hist0) hist_add_runs(bins[wave_id()], (u32)key & 255u, valid);
        }
        if (tile_min) {
            lo = wave_scan_inclusive(lo, OpMin());
            if (lane_id() == 63) wmin[wave_id()] = lo;
            __syncthreads();
            // smallest key of the tile: the Lyndon candidate search starts from these (same tile size as the scan)
            if (tid == 0) {
                u64 t = wmin[0];
                for (int w = 1; w < KB_THREADS / 64; w++) t = wmin[w] < t ? wmin[w] : t;
                tile_min[tile] = t;
            }
        }
    }
    if (hist0) kb_hist_flush(bins, hist0);
}

// A patch rewrites a key the key builder counted into the first radix pass's table (hist0, may be null): the count moves from
// the old key's bits 0..7 to the new one's.  (Every position is rewritten at most once, so the old key is the counted one.)
__device__ __forceinline__ void ks_patch(const KeyStore &ks, u64 p, u64 key, u32 *__restrict__ hist0)
{
    if (hist0) {
        const u32 od = (u32)ks_load(ks, p) & 255u, nd = (u32)key & 255u;
        if (od != nd) {
            u32 *row = hist0 + p / KB_RX_TILE * 256;
            atomicSub(&row[od], 1u);
            atomicAdd(&row[nd], 1u);
        }
    }
    ks_store(ks, p, key);
}

// keys of the (up to 64) positions in front of each factor end wrap around inside the factor
__global__ __launch_bounds__(256) void cyclic_patch_vl_kernel(const u8 *__restrict__ T, u64 n, const u64 *__restrict__ vtab, int key_bits,
                                                              const u32 *__restrict__ fstart, u64 k, KeyStore keys, u32 *__restrict__ hist0)
{
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    if (t >= k * 64) return;
    const u64 f = t / 64, j = t % 64;
    const u64 s = fstart[f], e = factor_end(fstart, k, n, f);
    if (j >= e - s) return;
    const u64 p = e - 1 - j;
    ks_patch(keys, p, vl_key_cyclic(T, vtab, key_bits, p, s, e), hist0);
}

// first msym symbols of rot(p)^omega for a position of factor [s, e)
__device__ __forceinline__ u64 cyclic_key(const u8 *__restrict__ T, const u8 *__restrict__ codes, int bits, int msym,
                                          u64 p, u64 s, u64 e)
{
    u64 key = 0, q = p;
    for (int j = 0; j < msym; j++) {
        key = (key << bits) | (u64)codes[T[q]];
        if (++q == e) q = s;
    }
    return key;
}

// positions closer than msym to their factor's end wrap around: rewrite their round-0 keys
__global__ __launch_bounds__(256) void cyclic_patch_kernel(const u8 *__restrict__ T, u64 n, const u8 *__restrict__ codes,
                                                           int bits, int msym, const u32 *__restrict__ fstart, u64 k,
                                                           KeyStore keys, u32 *__restrict__ hist0)
{
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 per = (u64)(msym - 1);
    if (per == 0 || t >= k * per) return;
    const u64 f = t / per, j = t % per;
    const u64 s = fstart[f], e = factor_end(fstart, k, n, f);
    if (j >= e - s) return;
    const u64 p = e - 1 - j;
    ks_patch(keys, p, cyclic_key(T, codes, bits, msym, p, s, e), hist0);
}

// ------------------------------------------------------------------------------------
// later rounds: key = (group head, rank of the h-th (cyclic) successor)
// ------------------------------------------------------------------------------------
// Sparse rank mode (few tied elements): no rank array exists.  The rank of a position that round 0 left alone is
// its slot = the number of sorted round-0 keys below its own key (binary search in the sorted key array); the rank
// of a position that round 0 left tied comes from a small map: tpos = those positions, sorted; trank = their current
// ranks, refreshed by every round.  So round 0 never scatters ranks (n random 4-byte writes), and a third or fourth
// round for a handful of stubborn ties costs a handful of binary searches, not an n-sized rank build.
// pdir (may be null): pdir[k] = first map entry whose position is >= k << psh, pdir[last + 1] = a0
__device__ __forceinline__ u64 tied_find(const u32 *__restrict__ tpos, u64 a0, u32 q, const u32 *__restrict__ pdir = nullptr, int psh = 0)
{
    u64 lo = 0, hi = a0;
    if (pdir) { const u32 k = q >> psh; lo = pdir[k]; hi = pdir[k + 1]; }
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (tpos[mid] < q) lo = mid + 1; else hi = mid;
    }
    return (lo < a0 && tpos[lo] == q) ? lo : ~0ull;
}

// cyclic successor inside the factor [s, s + L): position of the h-th symbol after p.  h < L is the common case (one factor
// holds most of a natural text), and then no division is needed: (p - s) + h < 2 L.
__device__ __forceinline__ u64 cyclic_successor(u64 p, u64 s, u64 L, u64 h)
{
    const u64 hm = h < L ? h : h % L;
    u64 off = (p - s) + hm;
    if (off >= L) off -= L;
    return s + off;
}

// Rank of a key in the sorted round-0 keys.  A plain binary search over n = 2^30 keys is 30 dependent probes, the last
// ~14 of them cache misses.  A directory over the keys' top dlog bits (dir[k] = first slot whose key's top bits are >= k,
// dir[2^dlog] = n) narrows the range to ~n / 2^dlog slots; the keys are close to uniform inside a bucket (entropy-coded
// symbols), so interpolation lands within a few dozen slots and a gallop from there stays inside two or three cache lines.
#define K0_DIR_LOG2_MAX 20
__global__ __launch_bounds__(256) void tpos_directory_kernel(const u32 *__restrict__ tpos, u64 a0, int psh, u64 buckets, u32 *__restrict__ pdir)
{
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k > buckets) return;
    if (k == buckets) { pdir[k] = (u32)a0; return; }
    const u64 want = k << psh;
    u64 lo = 0, hi = a0;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if ((u64)tpos[mid] < want) lo = mid + 1; else hi = mid;
    }
    pdir[k] = (u32)lo;
}
// The sorted round-0 keys: u64 each, or split as the packed passes leave them (SortPlan::keys_split) -- u32 low words, and for keys
// of more than 32 bits their bits 32..39 in a byte array of their own (hi; null for keys of <= 32 bits).
struct K0Keys {
    const u64 *wide; const u32 *lo; const u8 *hi;
    __device__ __forceinline__ u64 at(u64 i) const { return wide ? wide[i] : ((u64)lo[i] | (hi ? (u64)hi[i] << 32 : 0ull)); }
    __device__ __forceinline__ u32 low(u64 i) const { return wide ? (u32)wide[i] : lo[i]; }
};
__global__ __launch_bounds__(256) void k0_directory_kernel(const K0Keys K0, u64 n, int key_bits, int dlog, u64 *__restrict__ dir)
{
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k > (1ull << dlog)) return;
    if (k == (1ull << dlog)) { dir[k] = n; return; }
    const u64 want = k << (key_bits - dlog);
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (K0.at(mid) < want) lo = mid + 1; else hi = mid;
    }
    dir[k] = lo;
}
// Inside a directory bucket every key has want's top dlog bits; when those include all bits above 32 (key_bits - dlog <= 32) the
// low words alone decide, and a probe of split keys stays one random read.
__device__ __forceinline__ u64 k0_lower_bound(const K0Keys &K0, u64 n, u64 want, const u64 *__restrict__ dir, int dlog, int key_bits)
{
    u64 lo = 0, hi = n;
    bool low_only = false;
    auto below = [&](u64 p) { return low_only ? K0.low(p) < (u32)want : K0.at(p) < want; };
    if (dir) {
        const int sh = key_bits - dlog;
        low_only = !K0.wide && sh <= 32;
        const u64 k = want >> sh;
        lo = dir[k]; hi = dir[k + 1];
        if (lo == hi) return lo;
        u64 g = lo;
        if (sh > 0) {
            const double frac = (double)(want & ((1ull << sh) - 1ull)) / (double)(1ull << sh);
            g = lo + (u64)(frac * (double)(hi - lo));
        }
        if (g >= hi) g = hi - 1;
        if (below(g)) {                         // the answer lies in (g, hi]
            lo = g + 1;
            for (u64 st = 1; lo < hi; st <<= 1) {
                const u64 p = g + st;
                if (p >= hi) break;
                if (below(p)) lo = p + 1; else { hi = p; break; }
            }
        } else {                                // the answer lies in [lo, g]
            hi = g;
            for (u64 st = 1; lo < hi; st <<= 1) {
                if (st > g - lo) break;
                const u64 p = g - st;
                if (below(p)) { lo = p + 1; break; }
                hi = p;
            }
        }
    }
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (below(mid)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <bool CYCLIC>
__global__ __launch_bounds__(256) void keybuild_sparse_kernel(const u32 *__restrict__ a_idx, const u32 *__restrict__ a_head, u64 a,
                                                              const u8 *__restrict__ T, u64 n, const u8 *__restrict__ codes,
                                                              int bits, int msym, int pad_add, u64 h, const K0Keys K0, int rb,
                                                              const u32 *__restrict__ fstart, u64 k, u64 *__restrict__ keys,
                                                              const u64 *__restrict__ vtab /* variable-length codes, or null */, int key_bits,
                                                              const u32 *__restrict__ tpos, const u32 *__restrict__ trank, u64 a0,
                                                              const u64 *__restrict__ dir, int dlog,
                                                              const u32 *__restrict__ pdir, int psh)
{
    __shared__ u64 svtab[256];
    if (vtab) svtab[threadIdx.x] = vtab[threadIdx.x];
    __syncthreads();
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= a) return;
    const u64 p = a_idx[i];
    u64 q, s = 0, e = 0;
    bool past_end = false;
    if (CYCLIC) {
        const u64 f = factor_of(fstart, k, p);
        s = fstart[f]; e = factor_end(fstart, k, n, f);
        const u64 L = e - s;
        q = cyclic_successor(p, s, L, h);
    } else {
        q = p + h;
        past_end = q >= n;
    }
    u64 r = 0;
    if (!past_end) {
        const u64 j = tied_find(tpos, a0, (u32)q, pdir, psh);
        if (j != ~0ull) {
            r = trank[j];
        } else {
            u64 want;
            if (CYCLIC) {
                want = vtab ? vl_key_cyclic_fast(T, svtab, vtab, key_bits, q, s, e) : cyclic_key(T, codes, bits, msym, q, s, e);
            } else {
                want = 0;
                for (int jj = 0; jj < msym; jj++) {
                    const u64 rr = q + jj;
                    want = (want << bits) | (rr < n ? (u64)codes[T[rr]] + (u64)pad_add : 0ull);
                }
            }
            r = k0_lower_bound(K0, n, want, dir, dlog, key_bits);
        }
    }
    const u64 r2 = CYCLIC ? r : (past_end ? 0ull : r + 1ull);
    keys[i] = ((u64)a_head[i] << rb) | r2;
}

// tied map construction: keys = positions (sorted by the radix sort), values = round-0 group heads
__global__ __launch_bounds__(256) void tied_map_keys_kernel(const u32 *__restrict__ idx, u64 a, u64 *__restrict__ keys)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < a) keys[i] = idx[i];
}
__global__ __launch_bounds__(256) void tied_map_finish_kernel(const u64 *__restrict__ keys, u64 a, u32 *__restrict__ tpos)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < a) tpos[i] = (u32)keys[i];
}

// ------------------------------------------------------------------------------------
// re-rank: ONE scan over the sorted keys gives group heads and compacts the still-tied elements
// ------------------------------------------------------------------------------------
// scan element: high word = slot of a group's first element (max-scan), low word = 1 for an
// element of a group with more than one member (sum-scan)
struct OpHeadCount {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const
    {
        const u32 ha = (u32)(a >> 32), hb = (u32)(b >> 32);
        return ((u64)(ha > hb ? ha : hb) << 32) | (u64)(u32)((u32)a + (u32)b);
    }
};

// The scan kernels visit element i = tile_base + j * 256 + tid, so the neighbouring keys K[i-1], K[i+1]
// sit in the neighbouring lanes: one global load per element; the wave's two edge lanes fetch the key across
// the wave boundary with a second, predicated load.  Loads are split from their use (load()/make()) so that a
// thread's eight loads are all in flight before the first flag is computed.
struct GroupRaw { u64 k, edge; u32 slot; };

struct GroupIn {
    const u64 *K; const u32 *S; u64 a; int rb;
    __device__ __forceinline__ GroupRaw load(u64 i) const
    {
        GroupRaw r;
        r.k = K[i];
        const int lane = lane_id();
        const u64 act = __ballot(true);                       // lanes that hold an element (the tail tile is ragged)
        const bool next_here = lane < 63 && ((act >> ((lane + 1) & 63)) & 1ull);
        r.edge = 0;
        if (lane == 0 && i > 0) r.edge = K[i - 1];
        if (lane != 0 && !next_here && i + 1 < a) r.edge = K[i + 1];
        r.slot = S[i];
        return r;
    }
    __device__ __forceinline__ u64 make(u64 i, const GroupRaw &r, u32 *note) const
    {
        const u64 ki = r.k;
        const int lane = lane_id();
        const u64 act = __ballot(true);
        const bool next_here = lane < 63 && ((act >> ((lane + 1) & 63)) & 1ull);
        u64 kp = shfl_up_t(ki, 1), kn = shfl_down_t(ki, 1);
        if (lane == 0) kp = r.edge;                           // lane 0 is never also the last holder unless alone; see below
        if (!next_here) kn = r.edge;
        // a lane that is both first and last (single active lane) has only one edge slot: its successor is out of range
        // or in the next wave; that only happens in the ragged tail, where lane 0's successor is loaded here
        if (lane == 0 && !next_here && i + 1 < a) kn = K[i + 1];
        const bool f0 = i == 0 || ki != kp;
        const bool f1 = i + 1 == a || kn != ki;
        const bool so = i > 0 && (ki >> rb) == (kp >> rb);
        *note = (f0 ? 1u : 0u) | (f1 ? 2u : 0u) | (so ? 4u : 0u);
        return ((u64)(f0 ? r.slot : 0u) << 32) | (u64)((f0 && f1) ? 0u : 1u);
    }
    __device__ __forceinline__ u64 operator()(u64 i, u32 *note) const { return make(i, load(i), note); }
    __device__ __forceinline__ u64 operator()(u64 i) const { u32 note; return make(i, load(i), &note); }
};

struct GroupOut {
    const u32 *S; const u32 *V; u64 a; int rb;
    const u64 *K;                                   // the sorted keys (old head = K[i] >> rb)
    const u32 *tpos; u32 *trank; u64 a0;            // sparse rank map (tied positions -> rank), or nullptr
    u32 *SA;
    u32 *n_idx, *n_slot, *n_head;
    u64 *cnt_active, *cnt_splits;
    // note: the flags GroupIn computed for this element (same lane), so the keys are not read again
    __device__ __forceinline__ void operator()(u64 i, u64 v, u32 note) const
    {
        const bool f0 = note & 1u, f1 = note & 2u, same_old = note & 4u;
        const bool keep = !(f0 && f1);
        const u32 head = (u32)(v >> 32);
        const u32 val = V[i];
        const u32 slot = S[i];
        // an element whose group keeps its first slot keeps its rank: no map search for it
        const bool moved = (u32)(K[i] >> rb) != head;
        if (tpos && moved) { const u64 j = tied_find(tpos, a0, val); if (j != ~0ull) trank[j] = head; }
        SA[slot] = val;
        if (keep) {
            const u32 dst = (u32)v - 1u;
            n_idx[dst] = val; n_slot[dst] = slot; n_head[dst] = head;
        }
        // number of still-tied elements = inclusive count at the last element (no atomics on the n-sized round);
        // a count of exactly 2^32 wraps to 0 with the last element tied
        if (i + 1 == a) *cnt_active = ((u32)v == 0u && keep) ? 0x100000000ull : (u64)(u32)v;
        // "did any group split this round?" is all the driver needs: one plain store per wave, and none once the
        // flag is visibly set (counting with atomics serialised millions of waves on one address in deep rounds)
        const u64 ms = __ballot(f0 && same_old);
        if (ms && lane_id() == __ffsll((unsigned long long)__ballot(true)) - 1 &&
            __hip_atomic_load(cnt_splits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
            __hip_atomic_store(cnt_splits, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// ---- round 0 at word granularity ---------------------------------------------------------------------------------------
// The n-sized round needs the sorted keys only to know where groups start (f0) and which elements sit in a group of more
// than one (keep).  group_flags_kernel reads the keys once and leaves both as bitmaps (one u64 per 64 slots, straight
// from __ballot); the scan then runs over n/64 words instead of n elements, and tied_from_flags_kernel turns the set
// bits into the tied list: a third of the time of an element-wise scan over the keys, as the later rounds run (GroupIn/GroupOut).
#define GF_WORDS 8      // words (of 64 slots) a wave handles per step: eight key loads in flight per lane
// A slot starts a group when its key differs from the slot before; it is the last of its group when the NEXT slot starts one: so only
// the left neighbour's key is fetched (DPP wave_shr:1 on the two halves; lane 0 takes the word before's lane 63 from a scalar), and
// "last of its group" is the start mask shifted by one, as scalar arithmetic on the ballot words.  (The first version brought both
// neighbours through the LDS crossbar, eight ds_bpermute per element: 2.45 ms at 2^30 where the keys stream in 1.7.)
// The keys come through a loader: GfWide (u64 keys; mask = the key bits that count -- the 64-bit path parks position bits above
// them) or GfSplit (the split form of the packed round-0 sort, K0Keys: 5 or 4 bytes per slot instead of 8).
struct GfWide {
    const u64 *k; u64 mask;
    __device__ __forceinline__ u64 operator()(u64 i) const { return k[i] & mask; }
};
template <bool HI>
struct GfSplit {
    const u32 *lo; const u8 *hi;
    __device__ __forceinline__ u64 operator()(u64 i) const { return (u64)lo[i] | (HI ? (u64)hi[i] << 32 : 0ull); }
};
template <class KL>
__global__ __launch_bounds__(256) void group_flags_kernel(const KL K, u64 n, u64 *__restrict__ headw, u64 *__restrict__ keepw)
{
    const int lane = lane_id();
    const u64 words = (n + 63) / 64;
    const u64 wave = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6, waves = ((u64)gridDim.x * 256) >> 6;
    for (u64 w0 = wave * GF_WORDS; w0 < words; w0 += waves * GF_WORDS) {
        // (unconditional loads from clamped indices: a load under `i < n ? ... : 0` becomes a branch with a wait for the data behind it,
        // ONE load in flight per wave -- which is how this kernel ran at 3.5 TB/s for three rounds; what a slot past the end holds is
        // never looked at)
        u64 k[GF_WORDS];
#pragma unroll
        for (int q = 0; q < GF_WORDS; q++) {
            const u64 i = (w0 + q) * 64 + lane;
            k[q] = K(i < n ? i : n - 1);
        }
        const u64 first = w0 * 64, after = (w0 + GF_WORDS) * 64;          // the chunk's outer neighbours: slots first - 1 and after
        const u64 before_key = K(first > 0 ? first - 1 : 0);                 // (uniform addresses: scalar loads)
        const u64 after_key = K(after < n ? after : n - 1);
        u64 hm[GF_WORDS], vm[GF_WORDS];        // per word: slots that start a group (slots past the end count as starts), valid slots
        u64 prev63 = before_key;
#pragma unroll
        for (int q = 0; q < GF_WORDS; q++) {
            const u64 i = (w0 + q) * 64 + lane;
            const u32 lo = (u32)k[q], hi = (u32)(k[q] >> 32);
            const u32 plo = (u32)__builtin_amdgcn_update_dpp((int)lo, (int)lo, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
            const u32 phi = (u32)__builtin_amdgcn_update_dpp((int)hi, (int)hi, 0x138, 0xf, 0xf, false);
            const bool valid = i < n;
            const bool diff = lane == 0 ? (i == 0 || k[q] != prev63) : (lo != plo || hi != phi);
            vm[q] = __ballot(valid);
            hm[q] = __ballot(!valid || diff);
            prev63 = ((u64)(u32)__builtin_amdgcn_readlane((int)hi, 63) << 32) | (u64)(u32)__builtin_amdgcn_readlane((int)lo, 63);
        }
        const bool after_starts = after >= n || after_key != prev63;          // does slot `after` start a group (or lie past the end)?
        u64 mine_h = 0, mine_k = 0;
#pragma unroll
        for (int q = 0; q < GF_WORDS; q++) {
            const u64 nextbit = q + 1 < GF_WORDS ? (hm[q + 1 < GF_WORDS ? q + 1 : q] & 1ull) : (after_starts ? 1ull : 0ull);
            const u64 lastm = (hm[q] >> 1) | (nextbit << 63);                   // slots whose successor starts a group
            const u64 h = hm[q] & vm[q];
            if (lane == q) { mine_h = h; mine_k = vm[q] & ~(h & lastm); }
        }
        if (lane < GF_WORDS && w0 + lane < words) { headw[w0 + lane] = mine_h; keepw[w0 + lane] = mine_k; }
    }
}

// scan element of a word: (slot of its last group start, 0 if none) : (number of tied slots)
struct WordIn {
    const u64 *headw, *keepw;
    __device__ __forceinline__ u64 operator()(u64 w) const
    {
        const u64 hm = headw[w], km = keepw[w];
        const u64 pos = hm ? w * 64 + (u64)(63 - __clzll((long long)hm)) : 0ull;
        return (pos << 32) | (u64)__popcll(km);
    }
};

__global__ __launch_bounds__(256) void tied_from_flags_kernel(const u64 *__restrict__ headw, const u64 *__restrict__ keepw,
                                                              const u64 *__restrict__ pre, u64 n, const u32 *__restrict__ V,
                                                              u32 *__restrict__ n_idx, u32 *__restrict__ n_slot, u32 *__restrict__ n_head,
                                                              u64 *__restrict__ cnt_active)
{
    const int lane = lane_id();
    const u64 words = (n + 63) / 64;
    const u64 wave = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6, waves = ((u64)gridDim.x * 256) >> 6;
    for (u64 wb = wave * 64; wb < words; wb += waves * 64) {
        // lane l holds word wb + l; words with tied slots are then expanded one at a time by the whole wave
        const u64 w = wb + lane;
        u64 hm = 0, km = 0, pr = 0;
        if (w < words) { hm = headw[w]; km = keepw[w]; pr = pre[w]; }
        if (w + 1 == words) *cnt_active = (u64)(u32)pr + (u64)__popcll(km);
        u64 todo = __ballot(km != 0);
        // four words per step, their positions fetched together (whole words, from indices clamped into the array): a word's stores wait
        // for its load, so taken one at a time the words went by at one load latency each
        while (todo) {
            int q[4];
            u32 v[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                q[t] = todo ? __ffsll((unsigned long long)todo) - 1 : -1;
                todo &= todo - 1;                                   // (0 stays 0)
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const u64 i = (wb + (u64)(q[t] < 0 ? 0 : q[t])) * 64 + lane;
                v[t] = V[i < n ? i : n - 1];
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (q[t] < 0) continue;
                const u64 h = shfl_t(hm, q[t]), kk = shfl_t(km, q[t]), pq = shfl_t(pr, q[t]);
                if ((kk >> lane) & 1ull) {
                    const u64 i = (wb + q[t]) * 64 + lane;
                    const u64 below = lane == 63 ? h : h & ((2ull << lane) - 1ull);        // group starts at or before this slot
                    const u32 head = below ? (u32)((wb + q[t]) * 64 + (u64)(63 - __clzll((long long)below))) : (u32)(pq >> 32);
                    const u32 dst = (u32)pq + (u32)__popcll(kk & lanemask_lt());
                    n_idx[dst] = v[t]; n_slot[dst] = (u32)i; n_head[dst] = head;
                }
            }
        }
    }
}

// rank[sa[i]] = i for every slot, then rank[idx] = head for the still-tied elements
__global__ __launch_bounds__(256) void rank_from_sa_kernel(const u32 *__restrict__ SA, u64 n, u32 *__restrict__ rank)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) rank[SA[i]] = (u32)i;
}
__global__ __launch_bounds__(256) void rank_from_list_kernel(const u32 *__restrict__ idx, const u32 *__restrict__ head, u64 a,
                                                             u32 *__restrict__ rank)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < a) rank[idx[i]] = head[i];
}

// ------------------------------------------------------------------------------------
// the doubling sort
// ------------------------------------------------------------------------------------
// What a doubling sort works in and what its stages tell each other: three kinds of field, each with one writer
struct SortSpace : SortBufs {               // 1. buffers: keys, vals (n each), tile_hist, scan_temp, placed by the arena's layout (FwdArena)
    u32 *rank = nullptr;                    //    rank (n): ensure_rank()
    // 2. inputs of the cyclic sort, set by forward_run before it.  Emission riding on round 0: P[p] = T[cprev(p)] travels with the
    // pairs and the last pass writes it straight into the output; carry_out null = gather after the sort instead
    const u8 *carry_src = nullptr;
    u8 *carry_buf[2] = {nullptr, nullptr};
    u8 *carry_out = nullptr;
    bool want_split = false;                // the sort will carry the byte stream (=> the packed passes may apply, the keys may be split)
    // 3. handed on by one stage to those after it.  round0_keys(): keys[0] holds split keys; first_hist (split keys only, may be null):
    // the first packed pass's table as the key builder counted it (SortPlan::first_hist).  It lives in vals[0]: round 0's values are
    // the identity, which the first pass does not read, and nothing else uses vals[0] before that pass has scanned the table.
    bool split_keys = false;
    u32 *first_hist = nullptr;
    const u32 *tie_slots = nullptr;         // tied_list(): the round-0 tie list (slots), for patching the carried bytes of elements
    u64 tie_count = 0;                      // that later rounds reorder
    bool ties_emitted = false;              // doubling_sort(): the later rounds wrote the bytes of the tied elements themselves (direct, dense)
};

// the dense rank array (4 n bytes) exists only for inputs that need it: many ties after round 0, a suffix array with ranks, or a
// sort without the carried-byte buffers (whose space the round-0 flag words otherwise use)
static int ensure_rank(bwts_ctx *ctx, SortSpace &sp, u64 n)
{
    if (sp.rank) return BWTS_OK;
    char *p = nullptr;
    BWTS_TRY(aux_reserve_slot(ctx, 4, align_up((size_t)n * 4, 256), &p));
    sp.rank = (u32 *)p;
    return BWTS_OK;
}

// ---- dense rank array after round 0, binned -------------------------------------------------------------------------
// rank[SA[i]] = head(i) is n random 4-byte writes: 24 G/s on this chip, 73-85 G/s when the writes in flight fall into a
// window of <= 1 MB (tools/micro/window_scatter.hip).  So: one u64 per slot, (head << 32) | position, with head(i) straight from
// the round-0 flag words (the tied elements need no second scatter), sorted on the position's top 16 bits by two keys-only radix
// passes (ballot-ranked like every other pass: a partition by LDS atomics cost 30 ms at n = 2^30), then rank[position] = head
// with all writes of a workgroup inside a window of n / 2^16 positions.
__global__ __launch_bounds__(256) void rank_keys_kernel(const u32 *__restrict__ SA, u64 n, const u64 *__restrict__ headw,
                                                        const u64 *__restrict__ pre, u64 *__restrict__ keys)
{
    const int lane = lane_id();
    // four 64-slot words per wave and step, their loads issued together (from clamped indices: see DESIGN.md section 10 on loads
    // behind a bounds test): one at a time this kernel ran at 3.3 TB/s
    const u64 words = (n + 63) >> 6;
    const u64 wave = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6, waves = ((u64)gridDim.x * 256) >> 6;
    for (u64 w0 = wave * 4; w0 < words; w0 += waves * 4) {
        u64 hm[4], pr[4];
        u32 sa[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const u64 w = w0 + q < words ? w0 + q : words - 1;
            const u64 i = (w << 6) + lane;
            hm[q] = headw[w]; pr[q] = pre[w];
            sa[q] = SA[i < n ? i : n - 1];
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const u64 w = w0 + q, i = (w << 6) + lane;
            if (w >= words || i >= n) continue;
            const u64 below = lane == 63 ? hm[q] : hm[q] & ((2ull << lane) - 1ull);
            const u32 h = below ? (u32)((w << 6) + (u64)(63 - __clzll((long long)below))) : (u32)(pr[q] >> 32);
            keys[i] = ((u64)h << 32) | (u64)sa[q];
        }
    }
}
// The positions are a permutation, so after the sort window w (positions [w << wlog, (w + 1) << wlog)) occupies exactly the
// keys [w << wlog, ...): one workgroup takes one window, scatters the heads into an LDS image of the window's ranks and
// writes the image out whole -- a streaming kernel (20 ms -> 3.5 ms at n = 2^30 against scattering to memory, where the four
// workgroups sharing a window sat on different XCDs and every rank line left their L2s in pieces).
#define RA_WLOG_MAX 14
__global__ __launch_bounds__(1024) void rank_apply_kernel(const u64 *__restrict__ keys, u64 n, int wlog, u32 *__restrict__ rank)
{
    extern __shared__ __attribute__((aligned(16))) u32 ra_img[];
    const u64 lo = (u64)blockIdx.x << wlog;
    const u64 hi = lo + (1ull << wlog) < n ? lo + (1ull << wlog) : n;
    for (u64 i = lo + threadIdx.x; i < hi; i += 1024) { const u64 kv = keys[i]; ra_img[(u32)kv - (u32)lo] = (u32)(kv >> 32); }
    __syncthreads();
    for (u64 i = lo + threadIdx.x; i < hi; i += 1024) rank[i] = ra_img[i - lo];
}
__global__ void count_tied_kernel(const u64 *__restrict__ keepw, const u64 *__restrict__ pre, u64 words, u64 *__restrict__ cnt_active)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *cnt_active = (u64)(u32)pre[words - 1] + (u64)__popcll(keepw[words - 1]);
}

// ---- later rounds: sorting inside groups ------------------------------------------------------------------------------
// The tied list is ordered by group (heads increase along it), so a round's sort by (head, successor rank) only has to
// order each group by the rank.  On real text most tied elements sit in small groups (53 MiB of source text: 62 % of all
// element-rounds in groups of <= 8, the late rounds almost entirely pairs), yet a radix sort of the whole list costs 7 passes.
// seg_small_sort_kernel finds every element's group extent from the list's head array; the members of a group of at most
// SEG_CAP sort themselves in place (each counts the members ordering before it); elements of larger groups are flagged and counted.  If they are the majority
// the whole list goes through the radix sort as before; otherwise only they are compacted (scan), radix-sorted
// and written back to the slots they came from -- the compaction keeps list order, and a sort by (head, rank) keeps groups
// in list order, so the j-th sorted element belongs to the j-th flagged slot.
#define SEG_CAP 8
#define SEG_HALO 8                      // list elements a wave looks at in front of the ones it owns
#define SEG_OWN  (64 - SEG_HALO - SEG_CAP - 1)      // elements a wave decides: their group's start and end lie inside its 64-lane window
// A wave looks at 64 consecutive list elements (one coalesced load of their group heads), finds group starts with one
// __ballot, and decides the SEG_OWN elements in the middle of its window: an element's group start is the highest start
// bit at or below its lane, the group's end the next start bit above that.  Elements of groups larger than SEG_CAP get
// big[i] = 1 and are counted (one atomic per wave, spread over 256 counters).  A group of 2 .. SEG_CAP whose first element
// the wave owns is sorted by its own lanes: each loads its (key, value), counts with SEG_CAP shuffles how many members order
// before it (ties by list order: stable), and stores itself to that slot of the group -- coalesced loads, near-coalesced stores.
__global__ __launch_bounds__(256) void seg_small_sort_kernel(const u32 *__restrict__ head, u64 *__restrict__ K, u32 *__restrict__ V, u64 a,
                                                             u8 *__restrict__ big, u64 *__restrict__ big_count)
{
    const int lane = lane_id();
    const u64 wave = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6;
    const u64 own0 = wave * SEG_OWN;                 // first element this wave decides
    if (own0 >= a) return;
    const long long e = (long long)own0 - SEG_HALO + lane;        // list element of this lane (may lie outside [0, a))
    const bool inside = e >= 0 && (u64)e < a;
    const u32 h = inside ? head[e] : 0u;
    u32 hp = (u32)__shfl_up((int)h, 1, 64);
    if (lane == 0) hp = (e > 0 && (u64)(e - 1) < a) ? head[e - 1] : 0u;
    // a start: first element of the list, or head differs from the predecessor's; elements outside the list count as
    // starts so that a group never extends over them
    const bool start = !inside || e == 0 || h != hp;
    const u64 starts = __ballot(start);
    // every lane: where does my group start and end inside the window?  (-1 / size 0 = cannot tell from here)
    const u64 below = lane == 63 ? starts : starts & ((2ull << lane) - 1ull);
    const int s_lane = below ? 63 - __clzll((long long)below) : -1;
    u32 sz = 0;
    bool too_big = s_lane < 0 || lane - s_lane >= SEG_CAP;         // start further back than SEG_CAP - 1 elements
    if (!too_big) {
        const u64 above = s_lane == 63 ? 0ull : starts >> (s_lane + 1);
        const int e_lane = above ? s_lane + 1 + (__ffsll((unsigned long long)above) - 1) : 64;
        sz = (u32)(e_lane - s_lane);
        if (sz > SEG_CAP) too_big = true;
    }
    const bool owned = inside && lane >= SEG_HALO && lane < SEG_HALO + SEG_OWN;
    if (owned) big[e] = too_big ? 1 : 0;
    const u64 bm = __ballot(owned && too_big);
    if (bm && lane == 0) atomicAdd((unsigned long long *)&big_count[wave & 255], (unsigned long long)__popcll(bm));
    // members of a small group whose first element this wave owns sort themselves
    const bool member = inside && !too_big && sz >= 2 && s_lane >= SEG_HALO && s_lane < SEG_HALO + SEG_OWN;
    if (__ballot(member) == 0) return;
    u64 k = 0;
    u32 v = 0;
    if (member) { k = K[e]; v = V[e]; }
    const u32 o = member ? (u32)(lane - s_lane) : 0u;
    u32 rank = 0;
#pragma unroll
    for (int j = 0; j < SEG_CAP; j++) {
        const int src = (s_lane < 0 ? 0 : s_lane) + j;
        const u64 ko = shfl_t(k, src & 63);
        if (member && (u32)j < sz && (ko < k || (ko == k && (u32)j < o))) rank++;
    }
    if (member) { const u64 dst = (u64)e - o + rank; K[dst] = k; V[dst] = v; }
}
// compaction of the larger groups' elements.  Scan value: low word = flagged elements, high word = flagged groups (their
// first elements) before the position.  The compacted key carries the group's ordinal among the flagged groups instead of
// its head slot -- at most m/(SEG_CAP+1) groups, so the radix sort of the compacted list needs fewer key bits (usually a
// whole pass less); seg_writeback_kernel puts the head back.
struct SegFlagIn {
    const u8 *big; const u32 *head;
    __device__ __forceinline__ u64 operator()(u64 i) const
    {
        const u32 f = big[i];
        const u32 st = f && (i == 0 || head[i] != head[i - 1]) ? 1u : 0u;
        return ((u64)st << 32) | f;
    }
};
struct SegBigOut {
    const u8 *big; const u32 *head; const u64 *K; const u32 *V; u64 a; int rb; u64 *bk; u32 *bv; u32 *bpos; u64 *count;
    __device__ __forceinline__ void operator()(u64 i, u64 before) const
    {
        const u32 f = big[i];
        if (f) {
            const u32 st = (i == 0 || head[i] != head[i - 1]) ? 1u : 0u;
            const u64 ord = (before >> 32) + st - 1;                     // groups flagged up to and including this element's, minus one
            const u32 at = (u32)before;
            bk[at] = (ord << rb) | (K[i] & ((1ull << rb) - 1ull));
            bv[at] = V[i];
            bpos[at] = (u32)i;
        }
        if (i + 1 == a) *count = (u64)(u32)before + f;
    }
};
__global__ __launch_bounds__(256) void seg_writeback_kernel(const u64 *__restrict__ sk, const u32 *__restrict__ sv, const u32 *__restrict__ bpos,
                                                            u64 m, const u32 *__restrict__ head, int rb, u64 *__restrict__ K, u32 *__restrict__ V)
{
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j < m) {
        const u32 p = bpos[j];
        K[p] = ((u64)head[p] << rb) | (sk[j] & ((1ull << rb) - 1ull));       // the slot's group (sorting keeps groups in place)
        V[p] = sv[j];
    }
}

// The record of one doubling sort (ctx->fwd_report, read by bwts_debug_forward_report; include/bwts_test.h names the words): values the
// stages hold on the host anyway.
enum FwdReportWord { FR_CYCLIC, FR_N, FR_K, FR_SIGMA, FR_BITS, FR_MSYM, FR_KEY_BITS, FR_VARLEN, FR_HSTEP, FR_KEYS, FR_FLAGS_OUTSIDE_RANK,
                     FR_TIED0, FR_RANK_EARLY, FR_FORM, FR_NO_CHUNKS, FR_NEED_SA, FR_END, FR_REST_CHUNKS, FR_REST_BIG, FR_REST_TILES,
                     FR_ROUNDS, FR_DIRECTORY, FR_ORDER_SORT, FR_LEFT,
                     FC_S = 24, FC_MAXCHUNKS, FC_A_SMALL, FC_BIG0, FC_M_EXIT, FC_M_STAY, FC_GROUPS, FC_WIDE_POSSIBLE, FC_FSL, FC_COMPACTIONS,
                     FC_COMPACTIONS_SKIPPED, FC_ENQUEUED_BEHIND_LAST,
                     FR_DIRECT = 36 /* FwdDirect: what became of the direct form */,
                     FR_LEAN = 37 /* FwdLean: what became of the lean last pass of round 0 */,
                     FC_S_RECUT = 38 /* chunks: the nominal size after the last compaction, 0 without one */ };
enum FwdRoundWord { FRR_FORM, FRR_H, FRR_IN, FRR_OUT, FRR_SPLITS, FRR_PROBE = 5, FRR_MBIG, FRR_WHOLE, FRR_SKIP_NEXT,
                    FRR_CHUNKS_IN = 5, FRR_CHUNKS_OUT, FRR_BIG_IN, FRR_BIG_STAYS, FRR_BIG_LEAVES, FRR_NCHUNKS, FRR_CHUNK_S, FRR_TILE_MBIG = 5 };
enum FwdForm { FR_FORM_NONE, FR_FORM_SPARSE, FR_FORM_CHUNKS, FR_FORM_TILES, FR_FORM_DIRECT };
enum FwdNoChunks { FR_NC_NA, FR_NC_SHORT, FR_NC_KNOB, FR_NC_STORE, FR_NC_ORDER, FR_NC_BIGLIST };
enum FwdEnd { FR_END_NONE, FR_END_EMPTY, FR_END_STABLE };
enum FwdLean { FR_LEAN_NONE, FR_LEAN_HELD, FR_LEAN_SEAM, FR_LEAN_COUNT, FR_LEAN_DIRECT };
static_assert(FR_LEAN == BWTS_FWD_LEAN_WORD, "include/bwts_test.h names the word");
static_assert(FC_ENQUEUED_BEHIND_LAST < FR_DIRECT && FC_S_RECUT < FWD_HEADER_WORDS && FRR_CHUNK_S < FWD_ROUND_WORDS && FR_LEFT < FC_S, "the forward report's layout");
static u64 *fwd_report_open(bwts_ctx *ctx)
{
    u64 *w = ctx->fwd_report[ctx->fwd_sorts_made < FWD_REPORT_SORTS ? ctx->fwd_sorts_made : FWD_REPORT_SORTS - 1];
    memset(w, 0, FWD_SORT_WORDS * sizeof(u64));
    ctx->fwd_sorts_made++;
    return w;
}
// the record of the sort that is running: fwd_report_open() has run (only the stages under doubling_sort may ask)
static inline u64 *fwd_report_of(bwts_ctx *ctx) { assert(ctx->fwd_sorts_made > 0); return ctx->fwd_report[ctx->fwd_sorts_made < FWD_REPORT_SORTS ? ctx->fwd_sorts_made - 1 : FWD_REPORT_SORTS - 1]; }
// the record of the round that made the round counter `rounds` (round 0 made it 1); null past the records there are
static inline u64 *fwd_report_round(bwts_ctx *ctx, u32 rounds)
{
    return rounds >= 2 && rounds - 2 < BWTS_MAX_ROUND_STATS ? fwd_report_of(ctx) + FWD_HEADER_WORDS + (size_t)(rounds - 2) * FWD_ROUND_WORDS : nullptr;
}

#include "dense_rounds.h"
#include "chunk_rounds.h"

// What round 0 leaves for the stages after it
struct Round0 {
    int res;                        // which of sp.keys[] / sp.vals[] holds the sorted keys and the suffix array
    K0Keys k0v;                     // the sorted keys: u64 each, or split as the packed passes leave them
    u32 *SA;
    u64 *headw, *keepw, *pre;       // group flags (64 slots per word) and the word scan
    bool flags_outside_rank;        // the flag words lie in the carried-byte buffers, not in sp.rank
    u64 a;                          // tied elements
    // the last pass ran lean (SortPlan::lean_last): the flags are its own, SA holds the tied slots' positions only, the sorted keys
    // were not written; seam: it raised its give-up flag, and flags and count mean nothing
    bool lean, seam;
};
#define CNT_SEAM (SM_COUNTERS + 3)      // the lean pass's give-up flag: read back with the tied count
// the bits of headw's last word past n: no slots, no group starts.  (One launch of 5 us per forward.  Done inside the lean pass, one
// atomic AND by its first tile, it changed that kernel's code enough to cost 0.65 ms per forward at 2^30, measured; a copy of the
// word from the host or two 32-bit fills are launches too.)
__global__ void flag_tail_kernel(u64 *headw, u64 n)
{
    if (threadIdx.x == 0 && blockIdx.x == 0 && (n & 63)) headw[n >> 6] = (1ull << (n & 63)) - 1ull;
}

// Where round 0's group flags and their word scan go (3 * n/8 bytes): the carried-byte ping-pong buffers when there are any (the
// packed passes never use them, the others are done with them when the flags are made), else sp.rank, which is not needed before the
// rounds that follow.  Every sort decides this, takes sp.rank where it needs it and clears the counters BEFORE its radix passes, not
// behind them: the lean last pass writes flags and give-up word while it sorts, and one order serves all (no pass touches either)
static int round0_flag_words(bwts_ctx *ctx, u64 n, SortSpace &sp, Round0 *r0)
{
    const u64 words = (n + 63) / 64;
    r0->flags_outside_rank = sp.carry_buf[0] && sp.carry_buf[1] && n >= 4096;
    if (r0->flags_outside_rank) {
        r0->headw = (u64 *)sp.carry_buf[0]; r0->keepw = r0->headw + words; r0->pre = (u64 *)sp.carry_buf[1];
    } else {
        BWTS_TRY(ensure_rank(ctx, sp, n));
        r0->headw = (u64 *)sp.rank; r0->keepw = r0->headw + words; r0->pre = r0->keepw + words;
    }
    return BWTS_OK;
}

// The group flags of the sorted keys (unless the lean last pass left them already), their word scan and the tied count, read back
// together with the lean pass's give-up flag
static int round0_flags(bwts_ctx *ctx, u64 n, SortSpace &sp, Round0 *r0)
{
    u64 *cnt = ctx->d_small + SM_COUNTERS;
    const u64 words = (n + 63) / 64;
    const K0Keys &k0v = r0->k0v;
    u64 *K0 = sp.keys[r0->res];
    {
        SpanGuard g(ctx, BWTS_K_RERANK, n, r0->lean ? 16 * words : (k0v.wide ? 8 : k0v.hi ? 5 : 4) * n);
        if (!r0->lean) {
            u64 waves = (words + GF_WORDS - 1) / GF_WORDS;
            unsigned blocks = (unsigned)((waves + 3) / 4 < 16384 ? (waves + 3) / 4 : 16384);
            if (k0v.wide) group_flags_kernel<GfWide><<<dim3(blocks), dim3(256), 0, ctx->stream>>>(GfWide{K0, ~0ull}, n, r0->headw, r0->keepw);
            else if (k0v.hi) group_flags_kernel<GfSplit<true>><<<dim3(blocks), dim3(256), 0, ctx->stream>>>(GfSplit<true>{k0v.lo, k0v.hi}, n, r0->headw, r0->keepw);
            else group_flags_kernel<GfSplit<false>><<<dim3(blocks), dim3(256), 0, ctx->stream>>>(GfSplit<false>{k0v.lo, nullptr}, n, r0->headw, r0->keepw);
        }
        WordIn in{r0->headw, r0->keepw};
        ScanStoreArr<u64> out{r0->pre};
        BWTS_TRY((device_scan<false, u64>(ctx, words, in, out, OpHeadCount(), (u64)0, sp.scan_temp)));
        count_tied_kernel<<<dim3(1), dim3(64), 0, ctx->stream>>>(r0->keepw, r0->pre, words, cnt + 0);
        HIPC(hipGetLastError());
        STAGE("group flags + word scan + count");
    }
    BWTS_TRY(read_small(ctx, SM_COUNTERS, 4));
    r0->a = ctx->h_small[CNT_ACTIVE];
    r0->seam = r0->lean && ctx->h_small[CNT_SEAM] != 0;
    return BWTS_OK;
}

static SortPlan round0_plan(const SortSpace &sp, bool cyclic)
{
    SortPlan plan = sp.plan();
    plan.sym_src = sp.carry_src; plan.sym_buf[0] = sp.carry_buf[0]; plan.sym_buf[1] = sp.carry_buf[1]; plan.sym_final = sp.carry_out;
    plan.vals_identity = true;     // keybuild0 writes no value array
    plan.keys_split = cyclic && sp.split_keys && plan.sym_final;
    plan.first_hist = plan.keys_split ? sp.first_hist : nullptr;
    return plan;
}

// Round 0: the radix sort of the keys that keybuild0 left in sp.keys[0] (values: the identity), group flags, their word scan, the tied count.
// lean_ok: nobody behind this sort reads the sorted keys or the whole suffix array unless many positions stay tied, and few are
// expected to: five packed passes then end in the lean one, which leaves the flags itself
template <bool CYCLIC>
static int round0_sort(bwts_ctx *ctx, u64 n, const Alphabet &al, SortSpace &sp, bool lean_ok, Round0 *r0)
{
    u64 *cnt = ctx->d_small + SM_COUNTERS;
    SortPlan plan = round0_plan(sp, CYCLIC);
    if (CYCLIC && sp.split_keys && !plan.keys_split) return BWTS_E_INTERNAL;      // keybuild split the keys for a sort that cannot take them
    BWTS_TRY(round0_flag_words(ctx, n, sp, r0));
    r0->lean = lean_ok && plan.keys_split && al.key_bits > 32 && al.key_bits <= 40;
    HIPC(hipMemsetAsync(cnt, 0, 4 * sizeof(u64), ctx->stream));
    if (r0->lean) {
        const u64 words = (n + 63) / 64;
        HIPC(hipMemsetAsync(r0->headw, 0xff, words * sizeof(u64), ctx->stream));
        HIPC(hipMemsetAsync(r0->keepw, 0, words * sizeof(u64), ctx->stream));
        flag_tail_kernel<<<dim3(1), dim3(64), 0, ctx->stream>>>(r0->headw, n);
        HIPC(hipGetLastError());
        plan.lean_last = true; plan.headw = r0->headw; plan.keepw = r0->keepw; plan.seam_giveup = ctx->d_small + CNT_SEAM;
    }
    int res = 0;
    STAGE("cyclic patch (before round 0)");
    BWTS_TRY(radix_sort_pairs(ctx, plan, n, al.key_bits, &res));
    STAGE("round-0 sort");
    u64 *K0 = sp.keys[res];
    r0->res = res;
    r0->k0v = K0Keys{K0, nullptr, nullptr};
    if (plan.keys_split) r0->k0v = K0Keys{nullptr, (const u32 *)K0, al.key_bits > 32 ? (const u8 *)K0 + align_up((size_t)n * 4, 256) : nullptr};
    r0->SA = sp.vals[res];
    return round0_flags(ctx, n, sp, r0);
}

// Behind a lean last pass that did not stand (a seam it could not decide, more ties than the tied list has room for beside the
// untouched streams, a list the direct form gave back): the classic last pass from the same input, and the flags from its keys
static int round0_redo_classic(bwts_ctx *ctx, u64 n, SortSpace &sp, Round0 *r0)
{
    HIPC(hipMemsetAsync(ctx->d_small + SM_COUNTERS, 0, 4 * sizeof(u64), ctx->stream));
    BWTS_TRY(radix_packed_last_pass(ctx, round0_plan(sp, true), n));
    STAGE("round-0 sort: classic last pass");
    r0->lean = false;
    return round0_flags(ctx, n, sp, r0);
}

// Many ties: the dense rank array.  It is built BEFORE the tied list, while the list's future home (the other key
// buffer) is still free: the build sorts one u64 per slot between that buffer and the sorted keys' (not needed any
// more without the sparse rank map).
static int early_ranks(bwts_ctx *ctx, u64 n, SortSpace &sp, const Round0 &r0)
{
    BWTS_TRY(ensure_rank(ctx, sp, n));
    SpanGuard g(ctx, BWTS_K_RERANK, n, 28 * n);
    u64 *rk[2] = {sp.keys[r0.res ^ 1], sp.keys[r0.res]};
    u64 blocks = (n + 255) / 256; if (blocks > 16384) blocks = 16384;
    rank_keys_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(r0.SA, n, r0.headw, r0.pre, rk[0]);
    HIPC(hipGetLastError());
    // sorted on the position's top 16 bits (24 beyond n = 2^30): windows of at most 2^RA_WLOG_MAX positions
    const int pb = bitlen_u64(n - 1);
    const int sbits = pb - 16 <= RA_WLOG_MAX ? 16 : 24;
    int rres = 0;
    BWTS_TRY(radix_sort_keys(ctx, rk, sp.tile_hist, sp.scan_temp, n, pb - sbits, sbits, &rres));
    const int wlog = RA_WLOG_MAX;                   // sorted on at least the bits above 2^14: every 2^14 keys are 2^14 consecutive positions
    BWTS_TRY(ensure_dyn_lds(ctx, (const void *)rank_apply_kernel, (size_t)4 << RA_WLOG_MAX));
    rank_apply_kernel<<<dim3((unsigned)((n + (1ull << wlog) - 1) >> wlog)), dim3(1024), (size_t)4 << wlog, ctx->stream>>>(rk[rres], n, wlog, sp.rank);
    HIPC(hipGetLastError());
    return BWTS_OK;
}

// The tied list, in the key and value buffers that round 0 left free (8n + 4n bytes)
// (behind a lean last pass those still hold the pass's input, which a fallback sorts again: the list, of at most n / 32 elements
// then, goes where the sorted keys would have gone)
static int tied_list(bwts_ctx *ctx, u64 n, SortSpace &sp, const Round0 &r0, ActiveList *cur)
{
    u64 *cnt = ctx->d_small + SM_COUNTERS;
    if (r0.lean) {
        if (r0.a > n / 32) return BWTS_E_INTERNAL;
        const u64 cap = n / 32 + 1;                 // 3 * cap * 4 <= 8 n: the packed sort runs from 65 536 elements
        cur->idx = (u32 *)sp.keys[r0.res];
        cur->slot = cur->idx + cap;
        cur->head = cur->slot + cap;
    } else {
        cur->idx = (u32 *)sp.keys[r0.res ^ 1];
        cur->slot = cur->idx + n;
        cur->head = sp.vals[r0.res ^ 1];
    }
    SpanGuard g(ctx, BWTS_K_RERANK, r0.a, 12 * r0.a);
    const u64 waves = ((n + 63) / 64 + 63) / 64;
    const unsigned blocks = (unsigned)((waves + 3) / 4 < 16384 ? (waves + 3) / 4 : 16384);
    tied_from_flags_kernel<<<dim3(blocks), dim3(256), 0, ctx->stream>>>(r0.headw, r0.keepw, r0.pre, n, r0.SA, cur->idx, cur->slot, cur->head, cnt + 0);
    HIPC(hipGetLastError());
    STAGE("tied list");
    sp.tie_slots = cur->slot;        // stays untouched by the later rounds
    sp.tie_count = r0.a;
    return BWTS_OK;
}

// ---- few ties, shallow: every tied group ordered by comparing its members' rotations --------------------------------------
// After round 0 on an i.i.d.-like input the tied positions are a fraction of a percent of n, nearly all in pairs, and two tied
// rotations differ a few symbols behind what the key covered.  Ordering them needs no rank of any other position: the thread at a
// group's first list element (the list is in slot order, so a group is a run of equal heads) sorts the members by insertion,
// comparing their rotations inside their own Lyndon factors from symbol `skip` (al.hstep: what every key covers) on, sixteen bytes
// at a time away from the factors' wraps, and writes the members' carried bytes T[cprev(p)] into the group's slots.  SA, the list
// and the sorted keys stay as they are, so when any group does not fit -- more than DIRECT_GROUP members, or two rotations still
// equal after DIRECT_DEPTH symbols whose periods sum to more than that (below it, Fine and Wilf: equal for ever, the same byte
// either way) -- the flag is raised, every thread leaves at its next look at it, and the sparse rounds run as if nothing had been.
#define DIRECT_GROUP 8          // SEG_CAP: the groups the sparse rounds sort in place
#define DIRECT_DEPTH 640u       // symbols compared before a pair is given up: every thread resident with the first to get there has read
                                // as many by then, which is what a fallback costs (0.1 ms at 2^28 positions with 2^20 tied)
#define DIRECT_POLL  64u        // compared symbols between two looks at the flag
#define CNT_DIRECT   (SM_COUNTERS + 28)
enum FwdDirect { FR_DIRECT_NONE, FR_DIRECT_SETTLED, FR_DIRECT_GROUP, FR_DIRECT_DEEP };
static_assert(DIRECT_GROUP >= SEG_CAP, "the direct form takes every group the small-groups sort takes");

enum RotCmp { ROT_LESS, ROT_NOT_LESS, ROT_DEEP, ROT_STOP };
// the rotation at offset op of factor [ps, ps + pl) against the one at offset oq of [qs, qs + ql)
__device__ __forceinline__ RotCmp rotation_less(const u8 *__restrict__ T, u64 ps, u64 pl, u64 op, u64 qs, u64 ql, u64 oq, const u64 *flag)
{
    const u64 lim = pl + ql < DIRECT_DEPTH ? pl + ql : DIRECT_DEPTH;
    u64 next_poll = DIRECT_POLL;
    for (u64 d = 0; d < lim;) {
        if (pl - op >= 16 && ql - oq >= 16) {
            u64 x[2], y[2];
            __builtin_memcpy(x, T + ps + op, 16);
            __builtin_memcpy(y, T + qs + oq, 16);
            const int w = x[0] != y[0] ? 0 : 1;
            if (x[w] != y[w]) {
                const int sh = (__ffsll((unsigned long long)(x[w] ^ y[w])) - 1) & ~7;
                return ((x[w] >> sh) & 255u) < ((y[w] >> sh) & 255u) ? ROT_LESS : ROT_NOT_LESS;
            }
            op += 16; oq += 16; d += 16;
        } else {
            const u8 cp = T[ps + op], cq = T[qs + oq];
            if (cp != cq) return cp < cq ? ROT_LESS : ROT_NOT_LESS;
            op++; oq++; d++;
        }
        if (op == pl) op = 0;
        if (oq == ql) oq = 0;
        if (d >= next_poll) {
            if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return ROT_STOP;
            next_poll += DIRECT_POLL;
        }
    }
    return pl + ql > DIRECT_DEPTH ? ROT_DEEP : ROT_NOT_LESS;
}

__global__ __launch_bounds__(256) void direct_ties_kernel(const u32 *__restrict__ idx, const u32 *__restrict__ head, u64 a,
                                                          const u8 *__restrict__ T, u64 n, const u32 *__restrict__ fstart, u64 k, u64 skip,
                                                          u8 *__restrict__ out, u64 *flag)
{
    // a member: its position, its factor's first and last position (the length itself may be 2^32)
    __shared__ u32 s_pos[DIRECT_GROUP][256], s_first[DIRECT_GROUP][256], s_last[DIRECT_GROUP][256];
    const int t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * 256 + t;
    if (i >= a) return;
    const u32 h0 = head[i];
    if (i > 0 && head[i - 1] == h0) return;
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    u32 cnt = 1;
    while (cnt <= DIRECT_GROUP && i + cnt < a && head[i + cnt] == h0) cnt++;
    if (cnt > DIRECT_GROUP) { atomicCAS((unsigned long long *)flag, 0ull, (unsigned long long)FR_DIRECT_GROUP); return; }
    for (u32 j = 0; j < cnt; j++) {
        const u32 p = idx[i + j];
        const u64 f = factor_of(fstart, k, p);
        s_pos[j][t] = p; s_first[j][t] = fstart[f]; s_last[j][t] = (u32)(factor_end(fstart, k, n, f) - 1);
    }
    for (u32 m = 1; m < cnt; m++) {
        const u32 p = s_pos[m][t], pf = s_first[m][t], pe = s_last[m][t];
        const u64 ps = pf, pl = (u64)pe - pf + 1, op = ((u64)p - pf + skip) % pl;
        u32 j = m;
        while (j > 0) {
            const u32 q = s_pos[j - 1][t], qf = s_first[j - 1][t], qe = s_last[j - 1][t];
            const u64 ql = (u64)qe - qf + 1;
            const RotCmp c = rotation_less(T, ps, pl, op, qf, ql, ((u64)q - qf + skip) % ql, flag);
            if (c == ROT_STOP) return;
            if (c == ROT_DEEP) { atomicCAS((unsigned long long *)flag, 0ull, (unsigned long long)FR_DIRECT_DEEP); return; }
            if (c != ROT_LESS) break;
            s_pos[j][t] = q; s_first[j][t] = qf; s_last[j][t] = qe;
            j--;
        }
        s_pos[j][t] = p; s_first[j][t] = pf; s_last[j][t] = pe;
    }
    // the carried byte, as patch_ties_kernel finds it: a factor's first position takes the factor's last byte
    for (u32 j = 0; j < cnt; j++) {
        const u32 p = s_pos[j][t];
        out[(u64)h0 + j] = T[p == s_first[j][t] ? s_last[j][t] : p - 1];
    }
}

// Runs the kernel and reads its flag: FR_DIRECT_SETTLED when every tied slot now holds its byte, else why the list goes to the sparse rounds
static int direct_ties(bwts_ctx *ctx, const u8 *d_T, u64 n, const Alphabet &al, const u32 *d_fstart, u64 k, const SortSpace &sp,
                       const ActiveList &cur, u64 a, u64 *outcome)
{
    u64 *flag = ctx->d_small + CNT_DIRECT;
    HIPC(hipMemsetAsync(flag, 0, sizeof(u64), ctx->stream));
    {
        SpanGuard g(ctx, BWTS_K_RERANK, a, 24 * a);
        direct_ties_kernel<<<dim3((unsigned)((a + 255) / 256)), dim3(256), 0, ctx->stream>>>(cur.idx, cur.head, a, d_T, n, d_fstart, k, (u64)al.hstep,
                                                                                             sp.carry_out, flag);
        HIPC(hipGetLastError());
        STAGE("direct ties");
    }
    BWTS_TRY(read_small(ctx, CNT_DIRECT, 1));
    const u64 f = ctx->h_small[CNT_DIRECT];
    if (f != 0 && f != FR_DIRECT_GROUP && f != FR_DIRECT_DEEP) return BWTS_E_INTERNAL;
    *outcome = f ? f : (u64)FR_DIRECT_SETTLED;
    return BWTS_OK;
}
// positions from which the direct form is the default (BWTS_DIRECT_MIN_LOG2, a test switch, moves the line; 64: never)
static bool direct_ties_allowed(const bwts_ctx *ctx, u64 n)
{
    int lg = 24;
    if (const char *e = bwts_knob(ctx, "BWTS_DIRECT_MIN_LOG2")) lg = atoi(e);
    if (lg < 0) lg = 0;
    return lg < 64 && n >= (1ull << lg);
}

// the buffers of the sparse rounds' small-groups path: flags, compacted keys x2, values x2, slots of the larger groups
struct SegBufs { u8 *big; u64 *bk[2]; u32 *bv[2], *bpos; };

// Groups of <= SEG_CAP sort in place, the rest go through the radix sort (see seg_small_sort_kernel).  *whole = true: the larger
// groups hold nearly all of the list and nothing more was done -- the caller sorts everything; else K, V hold the sorted round.
static int seg_sort_round(bwts_ctx *ctx, SortSpace &sp, const SegBufs &sb, const u32 *head, u64 *K, u32 *V, u64 a, int rb, int round_key_bits,
                          bool *whole, bool *skip_next, u64 *m_big_out)
{
    u64 *cnt = ctx->d_small + SM_COUNTERS;
    u64 m_big = 0;
    {
        SpanGuard g(ctx, BWTS_K_RERANK, a, 20 * a);
        u64 *segcnt = ctx->d_small + SM_SEGCNT;
        HIPC(hipMemsetAsync(segcnt, 0, 256 * sizeof(u64), ctx->stream));
        const u64 waves = (a + SEG_OWN - 1) / SEG_OWN;
        seg_small_sort_kernel<<<dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, ctx->stream>>>(head, K, V, a, sb.big, segcnt);
        HIPC(hipGetLastError());
    }
    BWTS_TRY(read_small(ctx, SM_SEGCNT, 256));
    for (int c = 0; c < 256; c++) m_big += ctx->h_small[SM_SEGCNT + c];
    if (m_big > a) return BWTS_E_INTERNAL;
    *m_big_out = m_big;
    *skip_next = m_big * 10 > a * 9;
    // larger groups hold nearly all of the list: sorting everything costs less than compacting them
    // (by bytes moved the break-even is near 85 %)
    *whole = m_big * 5 > a * 4;
    if (*whole || !m_big) return BWTS_OK;
    {
        SpanGuard g(ctx, BWTS_K_RERANK, a, 20 * a);
        SegFlagIn fin{sb.big, head};
        SegBigOut fout{sb.big, head, K, V, a, rb, sb.bk[0], sb.bv[0], sb.bpos, cnt + 3};
        BWTS_TRY((device_scan<false, u64>(ctx, a, fin, fout, OpAdd(), (u64)0, sp.scan_temp)));
    }
    const SortPlan bp = sort_plan(sb.bk[0], sb.bk[1], sb.bv[0], sb.bv[1], sp.tile_hist, sp.scan_temp);
    int rbig = 0;
    const int big_bits = bitlen_u64(m_big / (SEG_CAP + 1)) + rb;       // ordinals < m_big / (SEG_CAP + 1)
    BWTS_TRY(radix_sort_pairs(ctx, bp, m_big, big_bits < round_key_bits ? big_bits : round_key_bits, &rbig));
    SpanGuard g(ctx, BWTS_K_RERANK, m_big, 28 * m_big);
    seg_writeback_kernel<<<dim3((unsigned)((m_big + 255) / 256)), dim3(256), 0, ctx->stream>>>(sb.bk[rbig], sb.bv[rbig], sb.bpos, m_big, head, rb, K, V);
    HIPC(hipGetLastError());
    return BWTS_OK;
}

// The rounds after round 0 when few elements are tied: sparse ranks (a map from the tied positions to their heads, everything else
// ranked by a search in the sorted round-0 keys), the list in SA order, a sort per round.
struct SparseRun {
    // side block 0: two key buffers, one value scratch, two list sets, the tied map, the two directories, the small-groups path's buffers
    u64 *akeys[2], *dir_at;
    u32 *scratch, *tpos, *trank, *pdir_at;
    ActiveList sets[2];
    SegBufs sb;
    void declare(BlockLayout &L, u64 a)
    {
        L.arrays(a, &akeys[0], &akeys[1]); L.array(&scratch, a);
        for (int s = 0; s < 2; s++) L.arrays(a, &sets[s].idx, &sets[s].slot, &sets[s].head);
        L.arrays(a, &tpos, &trank);
        L.array(&dir_at, ((u64)1 << K0_DIR_LOG2_MAX) + 1); L.array(&pdir_at, ((u64)1 << K0_DIR_LOG2_MAX) + 2);
        L.array(&sb.big, a); L.arrays(a, &sb.bk[0], &sb.bk[1]); L.arrays(a, &sb.bv[0], &sb.bv[1], &sb.bpos);
    }
    u64 a0;                         // tied after round 0: the map's size
    int rb, round_key_bits;
    u64 *dir = nullptr;             // sparse_map(): the directories over the sorted keys and the map's positions (null: plain
    u32 *pdir = nullptr;            // binary searches)
    int dlog = 0, psh = 0;
    ActiveList cur;                 // sparse_round(): the tied list and its size, the groups the round split, the set the next
    u64 a, splits = 0;              // round writes, the round counter
    int nxt = 0;
    u32 rounds;                     // (of the whole sort: round 0 counted)
    bool seg_skip_next = false;
};

// the tied map (tpos = the tied positions, sorted; trank = their ranks) and the two directories
static int sparse_map(bwts_ctx *ctx, SparseRun &r, u64 n, const Alphabet &al, SortSpace &sp, const K0Keys &k0v)
{
    const u64 a = r.a0;
    SpanGuard g(ctx, BWTS_K_RERANK, a, 24 * a);
    // directory over the sorted keys' top bits for the rank searches of keybuild_sparse_kernel
    const int kb = al.key_bits;
    r.dlog = kb < K0_DIR_LOG2_MAX ? kb : K0_DIR_LOG2_MAX;
    if (r.dlog > bitlen_u64(n)) r.dlog = bitlen_u64(n);
    if (r.dlog >= 8) {
        r.dir = r.dir_at;
        k0_directory_kernel<<<dim3((unsigned)(((1ull << r.dlog) + 1 + 255) / 256)), dim3(256), 0, ctx->stream>>>(k0v, n, kb, r.dlog, r.dir);
    }
    // split keys with a high byte: the rank searches compare low words alone (k0_lower_bound)
    if (k0v.hi && (!r.dir || kb - r.dlog > 32)) return BWTS_E_INTERNAL;
    tied_map_keys_kernel<<<dim3((unsigned)((a + 255) / 256)), dim3(256), 0, ctx->stream>>>(r.cur.idx, a, r.akeys[0]);
    HIPC(hipMemcpyAsync(r.scratch, r.cur.head, a * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
    const SortPlan mp = sort_plan(r.akeys[0], r.akeys[1], r.scratch, r.trank, sp.tile_hist, sp.scan_temp);
    int mr = 0;
    BWTS_TRY(radix_sort_pairs(ctx, mp, a, bitlen_u64(n - 1) > 0 ? bitlen_u64(n - 1) : 1, &mr));
    tied_map_finish_kernel<<<dim3((unsigned)((a + 255) / 256)), dim3(256), 0, ctx->stream>>>(r.akeys[mr], a, r.tpos);
    if (mr == 0) HIPC(hipMemcpyAsync(r.trank, r.scratch, a * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
    fwd_report_of(ctx)[FR_DIRECTORY] = r.dir ? (u64)r.dlog : 0;
    if (r.dir) {          // same switch as the key directory: a directory over the map's positions
        const int pb = bitlen_u64(n - 1);
        r.psh = pb > K0_DIR_LOG2_MAX ? pb - K0_DIR_LOG2_MAX : 0;
        const u64 buckets = ((n - 1) >> r.psh) + 1;
        r.pdir = r.pdir_at;
        tpos_directory_kernel<<<dim3((unsigned)((buckets + 1 + 255) / 256)), dim3(256), 0, ctx->stream>>>(r.tpos, a, r.psh, buckets, r.pdir);
    }
    HIPC(hipGetLastError());
    return BWTS_OK;
}

// one round at step h: keys (head, rank of the h-th successor), the sort, the re-rank scan; leaves the new list in r.cur / r.a
template <bool CYCLIC>
static int sparse_round(bwts_ctx *ctx, SparseRun &r, const u8 *d_T, u64 n, const Alphabet &al, const u32 *d_fstart, u64 k, SortSpace &sp, const Round0 &r0, u64 h)
{
    u64 *cnt = ctx->d_small + SM_COUNTERS;
    const u64 a = r.a;
    ActiveList &cur = r.cur;
    r.rounds++;
    {
        SpanGuard g(ctx, BWTS_K_KEYBUILD, a, 20 * a);
        const unsigned blocks = (unsigned)((a + 255) / 256);
        keybuild_sparse_kernel<CYCLIC><<<dim3(blocks), dim3(256), 0, ctx->stream>>>(
            cur.idx, cur.head, a, d_T, n, (const u8 *)(ctx->d_small + SM_CODES), al.bits, al.msym, al.pad_add, h, r0.k0v, r.rb, d_fstart, k, r.akeys[0],
            al.varlen ? ctx->d_small + SM_VTAB : nullptr, al.key_bits, r.tpos, r.trank, r.a0, r.dir, r.dlog, r.pdir, r.psh);
        HIPC(hipGetLastError());
    }
    const u64 *AK = r.akeys[0];
    const u32 *AV = cur.idx;
    // (large groups dominating one round dominate the next one too: then the classification is skipped every other round)
    const bool seg_probe = !r.seg_skip_next;
    r.seg_skip_next = false;
    bool whole = true;
    u64 m_big = 0;
    if (a > 4096 && seg_probe) BWTS_TRY(seg_sort_round(ctx, sp, r.sb, cur.head, r.akeys[0], cur.idx, a, r.rb, r.round_key_bits, &whole, &r.seg_skip_next, &m_big));
    u64 *rr = fwd_report_round(ctx, r.rounds);
    if (rr) {
        rr[FRR_FORM] = FR_FORM_SPARSE; rr[FRR_H] = h; rr[FRR_IN] = a;
        rr[FRR_PROBE] = a <= 4096 ? 0 : seg_probe ? 1 : 2; rr[FRR_MBIG] = m_big; rr[FRR_WHOLE] = whole; rr[FRR_SKIP_NEXT] = r.seg_skip_next;
    }
    if (whole) {
        const SortPlan ap = sort_plan(r.akeys[0], r.akeys[1], cur.idx, r.scratch, sp.tile_hist, sp.scan_temp);
        int r2 = 0;
        BWTS_TRY(radix_sort_pairs(ctx, ap, a, r.round_key_bits, &r2));
        AK = r.akeys[r2];
        AV = r2 ? r.scratch : cur.idx;
    }
    HIPC(hipMemsetAsync(cnt, 0, 4 * sizeof(u64), ctx->stream));
    {
        SpanGuard g(ctx, BWTS_K_RERANK, a, 24 * a);
        const ActiveList &to = r.sets[r.nxt];
        GroupIn in{AK, cur.slot, a, r.rb};
        GroupOut out{cur.slot, AV, a, r.rb, AK, r.tpos, r.trank, r.a0, r0.SA, to.idx, to.slot, to.head, cnt + 0, cnt + 1};
        BWTS_TRY((device_scan<true, u64>(ctx, a, in, out, OpHeadCount(), (u64)0, sp.scan_temp)));
    }
    BWTS_TRY(read_small(ctx, SM_COUNTERS, 4));
    r.a = ctx->h_small[CNT_ACTIVE]; r.splits = ctx->h_small[CNT_SPLITS];
    cur = r.sets[r.nxt]; r.nxt ^= 1;
    if (CYCLIC && r.rounds - 1 < BWTS_MAX_ROUND_STATS) ctx->tm.round_active[r.rounds - 1] = r.a;
    if (rr) { rr[FRR_OUT] = r.a; rr[FRR_SPLITS] = r.splits; }
    return BWTS_OK;
}

// cur, *a_io: the tied list; on return what is still tied (groups of equal infinite words).
template <bool CYCLIC>
static int sparse_rounds(bwts_ctx *ctx, const u8 *d_T, u64 n, const Alphabet &al, const u32 *d_fstart, u64 k, SortSpace &sp,
                         const Round0 &r0, ActiveList *cur_io, u64 *a_io, u32 *rounds_io)
{
    SparseRun r;
    BlockLayout L;
    r.cur = *cur_io; r.a = r.a0 = *a_io; r.rounds = *rounds_io; r.declare(L, r.a0);
    char *base = nullptr;
    BWTS_TRY(aux_reserve(ctx, L.bytes(), &base));
    L.place(base);
    r.rb = CYCLIC ? bitlen_u64(n - 1) : bitlen_u64(n);
    if (2 * r.rb > 64) return BWTS_E_RANGE;
    r.round_key_bits = 2 * r.rb > 1 ? 2 * r.rb : 1;
    BWTS_TRY(sparse_map(ctx, r, n, al, sp, r0.k0v));
    for (u64 h = (u64)al.hstep;; h <<= 1) {
        BWTS_TRY((sparse_round<CYCLIC>(ctx, r, d_T, n, al, d_fstart, k, sp, r0, h)));
        fwd_report_of(ctx)[FR_END] = r.a == 0 ? FR_END_EMPTY : CYCLIC && r.splits == 0 ? FR_END_STABLE : FR_END_NONE;
        if (r.a == 0) break;
        if (CYCLIC && r.splits == 0) break;             // partition stable under doubling: equal infinite words
        if (!CYCLIC && h >= n) return BWTS_E_INTERNAL;  // suffixes are distinct; cannot happen
        if (r.rounds > 80) return BWTS_E_INTERNAL;
    }
    *cur_io = r.cur; *a_io = r.a; *rounds_io = r.rounds;
    return BWTS_OK;
}

// Sorts all positions by their (cyclic | suffix) word.  sp.keys[0]/sp.vals[0] hold the round-0
// keys and the identity on entry.  want_ranks: leave final ranks in sp.rank (ISA for the suffix sort).
// Round 0, the dense ranks when many elements are tied, the tied list, then the later rounds in one of four forms: direct_ties (few
// ties, the byte rode round 0; a list it cannot settle goes on to the next), sparse_rounds, chunk_rounds, dense_rounds (tiles).
template <bool CYCLIC>
static int doubling_sort(bwts_ctx *ctx, const u8 *d_T, u64 n, const Alphabet &al, const u32 *d_fstart, u64 k,
                         SortSpace &sp, bool want_ranks, u32 **sa_out, u32 *rounds_out, u64 *active0_out)
{
    // the lean last pass: behind a cyclic sort whose byte rode round 0 only the ranks and the sparse and dense forms read the sorted
    // keys or the whole suffix array.  (A call that works on a segment table is no such sort: its partition reads the suffix array,
    // so no byte rides and carry_out is null.  The context's own table says nothing here: it stays set between calls, and a
    // segmented call transforms its large segments alone, byte riding.)  BWTS_RX_LEAN=0 (a test switch): never
    const bool direct_ok = CYCLIC && sp.carry_out && !want_ranks && direct_ties_allowed(ctx, n);
    const bool lean_off = [ctx] { const char *e = bwts_knob(ctx, "BWTS_RX_LEAN"); return e && atoi(e) == 0; }();
    const bool lean_ok = direct_ok && al.few_ties && !lean_off;
    Round0 r0;
    BWTS_TRY((round0_sort<CYCLIC>(ctx, n, al, sp, lean_ok, &r0)));
    // lean is all or nothing: it stands when the direct form settles every tied group from the list alone
    u64 lean = FR_LEAN_NONE, direct = FR_DIRECT_NONE;
    ActiveList cur, none{nullptr, nullptr, nullptr};
    bool listed = false;
    if (r0.lean) {
        lean = r0.seam ? FR_LEAN_SEAM : r0.a > n / 32 ? FR_LEAN_COUNT : FR_LEAN_HELD;
        if (lean == FR_LEAN_HELD) {
            BWTS_TRY(tied_list(ctx, n, sp, r0, &cur));
            listed = true;
            if (r0.a > 0) BWTS_TRY(direct_ties(ctx, d_T, n, al, d_fstart, k, sp, cur, r0.a, &direct));
            if (r0.a > 0 && direct != FR_DIRECT_SETTLED) lean = FR_LEAN_DIRECT;
        }
        if (lean != FR_LEAN_HELD) { BWTS_TRY(round0_redo_classic(ctx, n, sp, &r0)); listed = false; }
    }
    u64 a = r0.a;
    u32 *SA = r0.SA;
    *active0_out = a;
    if (CYCLIC) ctx->tm.round_active[0] = a;
    const bool rank_early = a > n / 32 && r0.flags_outside_rank && n >= (1ull << 22);
    u64 *rep = fwd_report_open(ctx);
    rep[FR_CYCLIC] = CYCLIC; rep[FR_N] = n; rep[FR_K] = k; rep[FR_SIGMA] = (u64)al.sigma; rep[FR_BITS] = (u64)al.bits; rep[FR_MSYM] = (u64)al.msym;
    rep[FR_KEY_BITS] = (u64)al.key_bits; rep[FR_VARLEN] = al.varlen; rep[FR_HSTEP] = (u64)al.hstep;
    rep[FR_KEYS] = r0.k0v.wide ? 0 : r0.k0v.hi ? 2 : 1; rep[FR_FLAGS_OUTSIDE_RANK] = r0.flags_outside_rank; rep[FR_TIED0] = a;
    rep[FR_RANK_EARLY] = rank_early; rep[FR_ROUNDS] = 1; rep[FR_LEAN] = lean;
    if (rank_early) BWTS_TRY(early_ranks(ctx, n, sp, r0));
    if (!listed) BWTS_TRY(tied_list(ctx, n, sp, r0, &cur));
    u32 rounds = 1;

    // every position tied at n = 2^32 (a constant or a two-symbol periodic input of exactly 4 GiB): the side buffers of the
    // later rounds are sized by the tied count and do not fit next to the 36 n bytes of round 0
    if (a > 0xffffffffull) return BWTS_E_NOMEM;
    // few tied elements: sparse rank map; many (real text ties most m-grams): the dense rank array
    if (a > 0 && a <= n / 32) {
        // the cyclic sort whose bytes rode round 0 (only the tied slots are left to write) first tries to settle every group by
        // comparing rotations; all or nothing: a list it cannot settle goes to the sparse rounds untouched
        // (a lean round 0 has asked already; what made the direct form give up is still what it is)
        if (direct_ok && direct == FR_DIRECT_NONE) BWTS_TRY(direct_ties(ctx, d_T, n, al, d_fstart, k, sp, cur, a, &direct));
        rep[FR_DIRECT] = direct;
        if (direct == FR_DIRECT_SETTLED) {
            rounds++;
            if (u64 *rr = fwd_report_round(ctx, rounds)) { rr[FRR_FORM] = FR_FORM_DIRECT; rr[FRR_H] = (u64)al.hstep; rr[FRR_IN] = a; rr[FRR_OUT] = 0; rr[FRR_SPLITS] = 1; }
            if (rounds - 1 < BWTS_MAX_ROUND_STATS) ctx->tm.round_active[rounds - 1] = 0;
            rep[FR_FORM] = FR_FORM_DIRECT; rep[FR_END] = FR_END_EMPTY;
            sp.ties_emitted = true;
            a = 0;
        } else {
            rep[FR_FORM] = FR_FORM_SPARSE;
            BWTS_TRY((sparse_rounds<CYCLIC>(ctx, d_T, n, al, d_fstart, k, sp, r0, &cur, &a, &rounds)));
        }
        rep[FR_ROUNDS] = rounds; rep[FR_LEFT] = a;
    } else if (a > 0) {
        BWTS_TRY(ensure_rank(ctx, sp, n));
        if (!rank_early) BWTS_TRY(build_ranks(ctx, SA, n, cur, a, sp.rank));      // (else built before the tied list, see above)
        // group-local rounds; SA is only rebuilt when someone reads it afterwards (suffix array requested, or the
        // gather form of the emission)
        const bool need_sa = !CYCLIC || !sp.carry_out;
        // chunks (chunk_rounds.h) unless BWTS_DENSE=tiles asks for the tile form (dense_rounds.h), the list is short or memory is
        const bool tiles_only = [ctx] { const char *e = bwts_knob(ctx, "BWTS_DENSE"); return e && !strcmp(e, "tiles"); }();
        bool handled = false;
        rep[FR_NEED_SA] = need_sa;
        if (tiles_only) rep[FR_NO_CHUNKS] = FR_NC_KNOB;
        if (!tiles_only) BWTS_TRY((chunk_rounds<CYCLIC>(ctx, d_T, n, al, d_fstart, k, sp, cur, a, SA, need_sa, &rounds, &handled)));
        rep[FR_FORM] = handled ? FR_FORM_CHUNKS : FR_FORM_TILES;
        if (!handled) BWTS_TRY((dense_rounds<CYCLIC>(ctx, d_T, n, al, d_fstart, k, sp, cur, a, SA, need_sa, &rounds)));
        rep[FR_ROUNDS] = rounds;
        sp.ties_emitted = CYCLIC && sp.carry_out;
        *sa_out = SA;
        *rounds_out = rounds;
        return BWTS_OK;
    }
    if (want_ranks && !rank_early) { BWTS_TRY(ensure_rank(ctx, sp, n)); BWTS_TRY(build_ranks(ctx, SA, n, a ? cur : none, a, sp.rank)); }
    *sa_out = SA;
    *rounds_out = rounds;
    return BWTS_OK;
}

static_assert(KB_TILE == SCAN_TILE, "keybuild0's tile minima feed the scan's final sweep");

// keys of positions [pos0, pos0 + count) into keys0 (index q - pos0), tile minima into tile_min[0 ..)
// hist0 (may be null; pos0 = 0 only): the first packed radix pass's table (SortPlan::first_hist)
static int launch_keybuild0_seg(bwts_ctx *ctx, const u8 *d_T, u64 n, const Alphabet &al, u64 *keys0, u64 *tile_min, bool split, u64 pos0, u64 count,
                                u8 *wprev = nullptr /* wide keys only: T[q - 1] of every position beside its key */, u32 *hist0 = nullptr)
{
    if (hist0 && (pos0 != 0 || !split)) return BWTS_E_INTERNAL;
    SpanGuard g(ctx, BWTS_K_KEYBUILD, count, count + (split ? 5 : 8) * count);
    const u64 blocks = (count + KB_RX_TILE - 1) / KB_RX_TILE;
    KeyStore ks = key_store_of(keys0, count, split, al.key_bits);
    ks.wprev = split ? nullptr : wprev;
    if (al.varlen) {
        keybuild0v_kernel<<<dim3((unsigned)blocks), dim3(KB_THREADS), 0, ctx->stream>>>(d_T, n, ctx->d_small + SM_VTAB, al.key_bits,
                                                                                        ks, tile_min, pos0, pos0 + count, hist0);
        HIPC(hipGetLastError());
        return BWTS_OK;
    }
    keybuild0_kernel<<<dim3((unsigned)blocks), dim3(KB_THREADS), 0, ctx->stream>>>(
        d_T, n, (const u8 *)(ctx->d_small + SM_CODES), al.bits, al.msym, al.pad_add, ks, tile_min, pos0, pos0 + count, hist0);
    HIPC(hipGetLastError());
    return BWTS_OK;
}

// ------------------------------------------------------------------------------------
// Lyndon factors, general path: strict prefix minima of the suffix ranks (mk_bwts_sa.c:126-129)
// ------------------------------------------------------------------------------------
struct RankIn { const u32 *r; __device__ __forceinline__ u32 operator()(u64 i) const { return r[i]; } };
struct MinFlagOut {
    const u32 *r; u8 *flag;
    __device__ __forceinline__ void operator()(u64 i, u32 min_before) const { flag[i] = (i == 0 || r[i] < min_before) ? 1 : 0; }
};
struct FlagIn { const u8 *flag; __device__ __forceinline__ u32 operator()(u64 i) const { return flag[i]; } };
struct StartOut {
    const u8 *flag; u32 *starts; u64 n; u64 *total;
    __device__ __forceinline__ void operator()(u64 i, u32 dst) const
    {
        if (flag[i]) starts[dst] = (u32)i;
        if (i + 1 == n) *total = (u64)dst + flag[i];
    }
};

// suffix sort on the padded alphabet; SA in *d_sa, ISA in sp.rank when want_ranks
static int suffix_sort_in(bwts_ctx *ctx, const u8 *d_T, u64 n, SortSpace &sp, bool want_ranks, u32 **d_sa, u32 *rounds)
{
    if (n > 0xffffffffull) return BWTS_E_RANGE;
    Alphabet al;
    BWTS_TRY(set_alphabet(ctx, true, n, &al));
    BWTS_TRY(launch_keybuild0_seg(ctx, d_T, n, al, sp.keys[0], nullptr, false, 0, n));
    u64 active0 = 0;
    return doubling_sort<false>(ctx, d_T, n, al, nullptr, 0, sp, want_ranks, d_sa, rounds, &active0);
}

// The shared tail of the general and the segment path, after their compaction scan left the sorted factor starts in keys[1] (free at
// both) and their number in CNT_TOTAL: read k, refuse one outside [k_min, n], move the list to side slot 2.
static int take_factor_list(bwts_ctx *ctx, u64 n, u64 k_min, SortSpace &sp, u32 **d_fstart, u64 *k_out)
{
    BWTS_TRY(read_small(ctx, CNT_TOTAL, 1));
    const u64 k = ctx->h_small[CNT_TOTAL];
    if (k < k_min || k > n) return BWTS_E_INTERNAL;
    char *fl = nullptr;
    BWTS_TRY(aux_reserve_slot(ctx, 2, (size_t)k * 4, &fl));
    HIPC(hipMemcpyAsync(fl, sp.keys[1], k * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
    *d_fstart = (u32 *)fl; *k_out = k;
    return BWTS_OK;
}

static int lyndon_general(bwts_ctx *ctx, const u8 *d_T, u64 n, SortSpace &sp, u32 **d_fstart, u64 *k_out, u32 *rounds)
{
    u32 *sa = nullptr;
    BWTS_TRY(suffix_sort_in(ctx, d_T, n, sp, true, &sa, rounds));
    // the sort's key buffers are free again: flags and the compacted starts live there
    u8 *flag = (u8 *)sp.keys[0];
    {
        SpanGuard g(ctx, BWTS_K_LYNDON, n, 8 * n);
        RankIn in{sp.rank};
        MinFlagOut out{sp.rank, flag};
        BWTS_TRY((device_scan<false, u32>(ctx, n, in, out, OpMin(), 0xffffffffu, sp.scan_temp)));
        FlagIn fin{flag};
        StartOut sout{flag, (u32 *)sp.keys[1], n, ctx->d_small + CNT_TOTAL};
        BWTS_TRY((device_scan<false, u32>(ctx, n, fin, sout, OpAdd(), 0u, sp.scan_temp)));
    }
    return take_factor_list(ctx, n, 1, sp, d_fstart, k_out);
}

// ------------------------------------------------------------------------------------
// Lyndon factors, fast path
// ------------------------------------------------------------------------------------
// p starts a factor iff its suffix is smaller than every earlier suffix.  With K(p) the packed
// first msym symbols: K(p) > min_{q<p} K(q) rules p out; K(p) < that minimum (and no zero fill
// in K(p)) proves it; equality -- or fill -- is settled by an exact comparison with the latest
// factor start.  Prefix-min scan over the round-0 keys -> candidate list -> one workgroup.
#define LYN_CAND_CAP   65536ull
#define LYN_WORK_CAP   (64ull << 20)      // bytes compared inside the resolver workgroup before it gives up

struct KeyIn { KeyStore K; __device__ __forceinline__ u64 operator()(u64 i) const { return ks_load(K, i); } };
struct CandOut {
    KeyStore K; u64 n; int msym; u64 *cand; u64 cap; u64 *counter;
    u64 pos0 = 0;          // element j of this launch is position pos0 + j (wide path: one segment at a time)
    __device__ __forceinline__ void operator()(u64 j, u64 min_before) const
    {
        const u64 ki = ks_load(K, j);
        const u64 i = pos0 + j;
        const bool c = i == 0 || ki <= min_before;
        const u64 m = __ballot(c);
        if (m == 0) return;
        const int leader = __ffsll((unsigned long long)m) - 1;
        unsigned long long base = 0;
        if (lane_id() == leader) base = atomicAdd((unsigned long long *)counter, (unsigned long long)__popcll(m));
        base = shfl_t((u64)base, leader);
        if (c) {
            const u64 at = base + (u64)__popcll(m & lanemask_lt());
            const bool definite = i == 0 || (ki < min_before && i + (u64)msym <= n);     // msym: symbols a key may reach over
            if (at < cap) cand[at] = (i << 1) | (definite ? 1ull : 0ull);
        }
    }
};

struct TileMayHoldCandidate {
    const u64 *tile_min;
    __device__ __forceinline__ bool operator()(u64 t, u64 min_before) const { return tile_min[t] <= min_before; }
};

// one workgroup walks the position-sorted candidates; exact suffix comparison is block-wide.  A comparison
// that is still undecided after LYN_LOCAL_LCE bytes is handed to the host, which runs it on the whole chip
// (suffix_less_grid_kernel) and restarts the walk behind that candidate.
#define LYN_LOCAL_LCE  (64u << 10)
struct LynState {         // in d_small: resumable state of the resolver
    u64 next;             // next candidate to look at
    u64 cur;              // latest factor start
    u64 k;                // factor starts found so far
    u64 status;           // 0 = finished, 1 = long comparison wanted (candidate `next`), 2 = work cap exceeded
    u64 forced;           // 1: the host has decided candidate `next`: forced_less says whether it starts a factor
    u64 forced_less;
    u64 work;
};

template <typename POS>
__global__ __launch_bounds__(256) void lyndon_resolve_kernel(const u8 *__restrict__ T, u64 n, const u64 *__restrict__ cand, u64 cnt,
                                                             POS *__restrict__ fstart, LynState *__restrict__ st, u64 work_cap)
{
    __shared__ int s_mis[4];      // per wave: first mismatching lane of the chunk, or -1
    __shared__ int s_less[4];     // per wave: candidate byte < current-start byte at that lane
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    u64 cur = st->cur, k = st->k, work = st->work;
    const u64 first = st->next;
    const bool forced = st->forced != 0, forced_less = st->forced_less != 0;
    __syncthreads();
    for (u64 c = first; c < cnt; c++) {
        const u64 e = cand[c];
        const u64 p = e >> 1;
        bool is_start;
        if (p == 0 || (e & 1)) {
            is_start = true;
        } else if (forced && c == first) {
            is_start = forced_less;
        } else {
            is_start = false;
            for (u64 off = 0;; off += 256) {
                const u64 i = off + tid;
                const int a = p + i < n ? (int)T[p + i] : -1;       // the shorter suffix is the smaller one
                const int b = cur + i < n ? (int)T[cur + i] : -1;
                const u64 mm = __ballot(a != b);
                if (lane == 0) s_mis[w] = mm ? __ffsll((unsigned long long)mm) - 1 : -1;
                if (mm && lane == __ffsll((unsigned long long)mm) - 1) s_less[w] = a < b;
                __syncthreads();
                int found = -1;
#pragma unroll
                for (int ww = 3; ww >= 0; ww--) if (s_mis[ww] >= 0) found = ww;
                const int less = found >= 0 ? s_less[found] : 0;
                __syncthreads();
                work += 256;
                if (found >= 0) { is_start = less != 0; break; }
                if (off + 256 >= LYN_LOCAL_LCE || work > work_cap) {
                    if (tid == 0) { st->next = c; st->cur = cur; st->k = k; st->work = work; st->forced = 0; st->status = work > work_cap ? 2 : 1; }
                    return;
                }
            }
        }
        if (is_start) {
            if (tid == 0) fstart[k] = (POS)p;
            k++;
            cur = p;
        }
    }
    if (tid == 0) { st->next = cnt; st->cur = cur; st->k = k; st->work = work; st->forced = 0; st->status = 0; }
}

// first position where T[p..] and T[q..] differ (q < p), over the whole chip: result[0] = min mismatch offset
__global__ __launch_bounds__(256) void suffix_mismatch_grid_kernel(const u8 *__restrict__ T, u64 n, u64 p, u64 q,
                                                                   unsigned long long *__restrict__ result)
{
    const u64 len = n - p;                  // p's suffix is the shorter one; offset len is a mismatch by definition
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < len; i += (u64)gridDim.x * 256) {
        if (i >= __hip_atomic_load(result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;     // someone found an earlier one
        if (T[p + i] != T[q + i]) { atomicMin(result, (unsigned long long)i); break; }
    }
}

// The cnt_c candidates in cand[0] become the factor starts fstart[0 .. *k): sorted by position, then walked by the resolver.
// BWTS_OK with *settled = false: too much sequential work, and the caller takes its other route to the factors.
template <typename IDX>
static int lyndon_resolve_candidates(bwts_ctx *ctx, const u8 *d_T, u64 n, u64 *const cand[2], u32 *const cvals[2], u32 *tile_hist, void *scan_temp, u64 cnt_c,
                                     IDX *fstart, u64 *k, bool *settled)
{
    *settled = false;
    // candidates arrive in arbitrary order: sort by position
    SortPlan cp = sort_plan(cand[0], cand[1], cvals[0], cvals[1], tile_hist, scan_temp);
    int res = 0;
    BWTS_TRY(radix_sort_pairs(ctx, cp, cnt_c, bitlen_u64(n) + 1, &res));
    // resumable resolver: long comparisons are decided by a grid-wide kernel between two of its launches
    LynState *d_st = (LynState *)(ctx->d_small + CNT_LYN_K);
    LynState *h_st = (LynState *)(ctx->h_small + CNT_LYN_K);
    unsigned long long *d_mis = (unsigned long long *)(ctx->d_small + CNT_LYN_K + 8);
    HIPC(hipMemsetAsync(d_st, 0, sizeof(LynState), ctx->stream));
    for (int iter = 0;; iter++) {
        {
            SpanGuard g(ctx, BWTS_K_LYNDON, cnt_c, 0);
            lyndon_resolve_kernel<IDX><<<dim3(1), dim3(256), 0, ctx->stream>>>(d_T, n, cand[res], cnt_c, fstart, d_st, LYN_WORK_CAP);
            HIPC(hipGetLastError());
        }
        BWTS_TRY(read_small(ctx, CNT_LYN_K, 8));
        if (h_st->status == 0) break;
        if (h_st->status == 2 || iter > 4096) return BWTS_OK;       // too much sequential work
        // status 1: compare suffix(p) with suffix(cur) on the whole chip
        u64 e = 0;
        HIPC(hipMemcpyAsync(&e, cand[res] + h_st->next, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
        HIPC(hipStreamSynchronize(ctx->stream));
        const u64 pp = e >> 1, qq = h_st->cur;
        const u64 len = n - pp;
        HIPC(hipMemcpyAsync(d_mis, &len, sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
        {
            SpanGuard g(ctx, BWTS_K_LYNDON, len, 2 * len);
            u64 blocks = (len + 255) / 256; if (blocks > 4096) blocks = 4096;
            suffix_mismatch_grid_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(d_T, n, pp, qq, d_mis);
            HIPC(hipGetLastError());
        }
        BWTS_TRY(read_small(ctx, CNT_LYN_K + 8, 1));
        const u64 at = ctx->h_small[CNT_LYN_K + 8];
        bool less;
        if (at >= len) less = true;                                 // suffix(p) is a proper prefix of suffix(cur): the shorter is smaller
        else {
            u8 ab[2];
            HIPC(hipMemcpyAsync(&ab[0], d_T + pp + at, 1, hipMemcpyDeviceToHost, ctx->stream));
            HIPC(hipMemcpyAsync(&ab[1], d_T + qq + at, 1, hipMemcpyDeviceToHost, ctx->stream));
            HIPC(hipStreamSynchronize(ctx->stream));
            less = ab[0] < ab[1];
        }
        h_st->forced = 1; h_st->forced_less = less ? 1 : 0; h_st->status = 0;
        HIPC(hipMemcpyAsync(d_st, h_st, sizeof(LynState), hipMemcpyHostToDevice, ctx->stream));
        HIPC(hipStreamSynchronize(ctx->stream));
    }
    *k = h_st->k;
    if (*k == 0) return BWTS_E_INTERNAL;
    *settled = true;
    return BWTS_OK;
}

// returns BWTS_OK with *done = false when the input needs the general path
static int lyndon_fast(bwts_ctx *ctx, const u8 *d_T, u64 n, const Alphabet &al, SortSpace &sp, const u64 *tile_min, u64 *cand[2],
                       u32 *cvals[2], u32 *fstart, u64 *k_out, bool *done)
{
    *done = false;
    u64 *cnt = ctx->d_small + SM_COUNTERS;
    HIPC(hipMemsetAsync(cnt + 4, 0, 4 * sizeof(u64), ctx->stream));
    {
        // keybuild0 left every tile's smallest key in tile_min; after the exclusive min-scan of those, a tile can
        // hold a candidate only if its own minimum does not exceed the minimum of everything before it
        SpanGuard g(ctx, BWTS_K_LYNDON, n, 0);
        const u64 tiles = scan_tiles(n);
        HIPC(hipMemcpyAsync(sp.scan_temp, tile_min, tiles * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream));
        BWTS_TRY((device_scan_partials<u64, OpMin>(ctx, tiles, OpMin(), ~0ull, sp.scan_temp)));
        const KeyStore ks = key_store_of(sp.keys[0], n, sp.split_keys, al.key_bits);
        KeyIn in{ks};
        CandOut out{ks, n, al.varlen ? 64 : al.msym, cand[0], LYN_CAND_CAP, ctx->d_small + CNT_CAND};
        TileMayHoldCandidate filter{tile_min};
        BWTS_TRY((device_scan_final<false, u64>(ctx, n, in, out, OpMin(), ~0ull, sp.scan_temp, filter)));
    }
    BWTS_TRY(read_small(ctx, CNT_CAND, 1));
    const u64 cnt_c = ctx->h_small[CNT_CAND];
    if (cnt_c == 0) return BWTS_E_INTERNAL;
    if (cnt_c > LYN_CAND_CAP) return BWTS_OK;
    return lyndon_resolve_candidates<u32>(ctx, d_T, n, cand, cvals, sp.tile_hist, sp.scan_temp, cnt_c, fstart, k_out, done);
}

// ------------------------------------------------------------------------------------
// Lyndon factors of many independent segments (bwts_forward_segments)
// ------------------------------------------------------------------------------------
// One wave per segment runs Duval's algorithm on the segment alone, so a suffix ends at its segment's end (the shorter one is the
// smaller) whatever the next segment holds.  The scalar state (i, j, k) is the same in every lane; the lanes look at 64 positions at
// once: while k == i the scan skips every j with T[j] > T[i] (each only resets k to i), otherwise it skips the run of positions where
// T[k + l] == T[j + l].  A factor start gets flag[p] = 1; the compaction scan of the general path turns the flags into the sorted list.
// Its work is the segment's length in sequential steps: segments of SEG_FWD_BIG bytes or more never get here (forward_segments_impl).
__global__ __launch_bounds__(256) void seg_duval_kernel(const u8 *__restrict__ T, const u64 *__restrict__ seg_off, u64 count, u8 *__restrict__ flag)
{
    const u64 s = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= count) return;
    const int lane = lane_id();
    const u64 base = seg_off[s], L = seg_off[s + 1] - base;
    const u8 *S = T + base;
    u64 i = 0;
    while (i < L) {
        u64 j = i + 1, k = i;
        for (;;) {
            if (k == i) {
                const u32 si = S[i];
                for (;;) {
                    const u64 q = j + (u64)lane;
                    const bool stop = q >= L || (u32)S[q] <= si;
                    const u64 m = __ballot(stop);
                    if (m) { j += (u64)(__ffsll((unsigned long long)m) - 1); break; }
                    j += 64;
                }
                if (j >= L || S[j] < S[k]) break;
                k++; j++;
                continue;
            }
            for (;;) {
                const u64 q = j + (u64)lane;
                const bool stop = q >= L || S[k + lane] != S[q];
                const u64 m = __ballot(stop);
                if (m) { const u64 l = (u64)(__ffsll((unsigned long long)m) - 1); k += l; j += l; break; }
                k += 64; j += 64;
            }
            if (j >= L || S[j] < S[k]) break;
            k = i; j++;                                   // T[k] < T[j]
        }
        // factors of length j - k start at i, i + (j - k), ... while <= k
        const u64 p = j - k, cnt = (k - i) / p + 1;
        for (u64 t = (u64)lane; t < cnt; t += 64) flag[base + i + t * p] = 1;
        i += cnt * p;
    }
}

static int segment_factors(bwts_ctx *ctx, const u8 *d_T, u64 n, const SegTable &seg, SortSpace &sp, u32 **d_fstart, u64 *k_out)
{
    {
        SpanGuard g(ctx, BWTS_K_LYNDON, n, 2 * n);
        HIPC(hipMemsetAsync(seg.flag, 0, n, ctx->stream));
        seg_duval_kernel<<<dim3((unsigned)((seg.count + 3) / 4)), dim3(256), 0, ctx->stream>>>(d_T, seg.d_off, seg.count, seg.flag);
        HIPC(hipGetLastError());
        FlagIn fin{seg.flag};
        StartOut sout{seg.flag, (u32 *)sp.keys[1], n, ctx->d_small + CNT_TOTAL};
        BWTS_TRY((device_scan<false, u32>(ctx, n, fin, sout, OpAdd(), 0u, sp.scan_temp)));
    }
    return take_factor_list(ctx, n, seg.count, sp, d_fstart, k_out);
}

static int lyndon_mode(const bwts_ctx *ctx)
{
    const char *env = bwts_knob(ctx, "BWTS_LYNDON");     // auto (default) | fast | general
    if (env && !strcmp(env, "general")) return 2;
    if (env && !strcmp(env, "fast")) return 1;
    return 0;
}

// The arena of a narrow forward call: every array it holds, declared once, on every call -- which path runs (fast or general factors,
// split or wide keys) is known only after the arena is reserved.  Side slots 2 (factor list of the general path), 3 (previous symbols +
// carried bytes of a sort on wide keys) and 4 (dense rank array) stay on demand: the headline path does not pay for them.
struct FwdArena {
    SortSpace sp;                           // the sort buffers (SortBufs): keys x2, vals x2, tile_hist, scan_temp
    u64 *cand[2];                           // Lyndon candidates, LYN_CAND_CAP each: the set, its sort's values, the factor starts found
    u32 *cvals[2], *fast_starts;
    u64 *tile_min;                          // smallest round-0 key of every scan tile
    u8  *flag_words[2];                     // round 0's group flags (2 x n/8 bytes) and their word scan (n/8) beside split keys
    void declare(BlockLayout &L, u64 n)
    {
        sp.declare(L, n);
        L.arrays(LYN_CAND_CAP, &cand[0], &cand[1]); L.arrays(LYN_CAND_CAP, &cvals[0], &cvals[1], &fast_starts);
        L.array(&tile_min, scan_tiles(n) + 1);
        L.array(&flag_words[0], n / 4 + 64); L.array(&flag_words[1], n / 8 + 64);
    }
};
size_t forward_arena_bytes(u64 n) { FwdArena A; BlockLayout L; A.declare(L, n); return L.bytes(); }
// points A's arrays into the arena, which the caller has reserved with forward_arena_bytes(n)
static int fwd_arena_place(bwts_ctx *ctx, u64 n, FwdArena &A)
{
    BlockLayout L;
    A.declare(L, n);
    char *base = (char *)arena_alloc(ctx, L.bytes());
    if (base) L.place(base);
    return base ? BWTS_OK : BWTS_E_NOMEM;
}

// Alphabet, split decision, round-0 keys in sp.keys[0] (values: the identity, unwritten).  tile_min (may be null): for the tiles' smallest
// keys.  count_first: the key builder may count the first packed pass's table into vals[0] -- only where no sort comes before the cyclic one.
static int round0_keys(bwts_ctx *ctx, const u8 *d_T, u64 n, SortSpace &sp, Alphabet *al, u64 *tile_min, bool count_first)
{
    BWTS_TRY(set_alphabet(ctx, false, n, al, d_T, &sp));
    sp.split_keys = sp.want_split && radix_packed_applicable(ctx, n, al->key_bits);
    STAGE("histogram + alphabet");
    sp.first_hist = count_first && sp.split_keys && radix_tile_hist_bytes(n) <= (size_t)n * 4 ? sp.vals[0] : nullptr;
    BWTS_TRY(launch_keybuild0_seg(ctx, d_T, n, *al, sp.keys[0], tile_min, sp.split_keys, 0, n, nullptr, sp.first_hist));
    STAGE("keybuild0");
    return BWTS_OK;
}

// wrap the keys of positions near their factor's end
static int cyclic_patch(bwts_ctx *ctx, const u8 *d_T, u64 n, const Alphabet &al, const KeyStore &ks, u32 *first_hist, const u32 *d_fstart, u64 k)
{
    const u64 threads = k * (u64)(al.varlen ? 64 : al.msym - 1);
    if (!threads) return BWTS_OK;
    SpanGuard g(ctx, BWTS_K_KEYBUILD, threads, 0);
    if (al.varlen)
        cyclic_patch_vl_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream>>>(
            d_T, n, ctx->d_small + SM_VTAB, al.key_bits, d_fstart, k, ks, first_hist);
    else
        cyclic_patch_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream>>>(
            d_T, n, (const u8 *)(ctx->d_small + SM_CODES), al.bits, al.msym, d_fstart, k, ks, first_hist);
    HIPC(hipGetLastError());
    return BWTS_OK;
}

// Finds the factors and leaves the cyclic round-0 keys in sp.keys[0] / identity in sp.vals[0]:
// factors (segments | fast | general), keys, head fix, patch.
static int factors_and_keys(bwts_ctx *ctx, const u8 *d_T, u64 n, FwdArena &A, Alphabet *al, u32 **d_fstart, u64 *k_out,
                            u32 *lyndon_rounds, bool hist_ready = false, const SegTable *seg = nullptr)
{
    SortSpace &sp = A.sp;
    if (!hist_ready) BWTS_TRY(read_histogram(ctx, d_T, n));
    const int mode = seg ? 3 : lyndon_mode(ctx);
    bool done = false;
    *lyndon_rounds = 0;
    if (seg) {                  // independent segments: each one's own factors (every segment end is a factor end)
        BWTS_TRY(segment_factors(ctx, d_T, n, *seg, sp, d_fstart, k_out));
        STAGE("segment factors");
    } else if (mode != 2) {     // the fast path reads the keys (and their tile minima): they come first
        BWTS_TRY(round0_keys(ctx, d_T, n, sp, al, A.tile_min, true));
        BWTS_TRY(lyndon_fast(ctx, d_T, n, *al, sp, A.tile_min, A.cand, A.cvals, A.fast_starts, k_out, &done));
        STAGE("lyndon_fast");
        if (done) *d_fstart = A.fast_starts;
        else if (mode == 1) return BWTS_E_INTERNAL;
    }
    // (the general path's suffix sort uses vals[0] and keys[0]: the keys are built after it, and count nothing.  After a fast path that
    // gave up, split_keys and first_hist stay set through that sort: only a cyclic sort reads them, and round0_keys() then sets both anew)
    if (!seg && !done) BWTS_TRY(lyndon_general(ctx, d_T, n, sp, d_fstart, k_out, lyndon_rounds));
    if (!done) BWTS_TRY(round0_keys(ctx, d_T, n, sp, al, nullptr, false));
    const KeyStore ks = key_store_of(sp.keys[0], n, sp.split_keys, al->key_bits);
    if (sp.split_keys) {
        carried_head_fix_kernel<<<dim3((unsigned)((*k_out + 255) / 256)), dim3(256), 0, ctx->stream>>>(d_T, n, *d_fstart, *k_out, ks);
        HIPC(hipGetLastError());
        STAGE("carried_head_fix");
    }
    return cyclic_patch(ctx, d_T, n, *al, ks, sp.first_hist, *d_fstart, *k_out);
}

// the test hooks' entries: their caller has reserved forward_arena_bytes(n)
int suffix_sort_device(bwts_ctx *ctx, const u8 *d_T, u64 n, u32 **d_sa, u32 **d_rank, u32 *rounds)
{
    ctx->fwd_sorts_made = 0;
    BWTS_TRY(read_histogram(ctx, d_T, n));
    FwdArena A;
    BWTS_TRY(fwd_arena_place(ctx, n, A));
    BWTS_TRY(suffix_sort_in(ctx, d_T, n, A.sp, true, d_sa, rounds));
    *d_rank = A.sp.rank;
    return BWTS_OK;
}
int lyndon_factors_device(bwts_ctx *ctx, const u8 *d_T, u64 n, u32 **d_fstart, u64 *k_out, u32 *rounds)
{
    ctx->fwd_sorts_made = 0;
    FwdArena A;
    BWTS_TRY(fwd_arena_place(ctx, n, A));
    Alphabet al;
    return factors_and_keys(ctx, d_T, n, A, &al, d_fstart, k_out, rounds);
}

// ------------------------------------------------------------------------------------
// emission (mk_bwts_sa.c:172-188): P[p] = T[cprev(p)], bwts[r] = P[sa[r]]
// ------------------------------------------------------------------------------------
// P[i] = T[i-1] (P[0] = T[n-1]); 16 bytes per thread: one 16-byte load, the byte in front of it, one 16-byte store
__global__ __launch_bounds__(256) void prevsym_kernel(const u8 *__restrict__ T, u64 n, u8 *__restrict__ P)
{
    const bool vec_ok = (((uintptr_t)T | (uintptr_t)P) & 15) == 0;
    for (u64 c = (u64)blockIdx.x * 256 + threadIdx.x; c * 16 < n; c += (u64)gridDim.x * 256) {
        const u64 i = c * 16;
        if (vec_ok && i + 16 <= n) {
            const uint4 v = *(const uint4 *)(T + i);
            const u32 before = i ? (u32)T[i - 1] : (u32)T[n - 1];
            uint4 o;
            o.x = (v.x << 8) | before;
            o.y = (v.y << 8) | (v.x >> 24);
            o.z = (v.z << 8) | (v.y >> 24);
            o.w = (v.w << 8) | (v.z >> 24);
            *(uint4 *)(P + i) = o;
        } else {
            for (u64 j = i; j < n && j < i + 16; j++) P[j] = j ? T[j - 1] : T[n - 1];
        }
    }
}
__global__ __launch_bounds__(256) void prevsym_fix_kernel(const u8 *__restrict__ T, u64 n, const u32 *__restrict__ fstart, u64 k,
                                                          u8 *__restrict__ P)
{
    const u64 f = (u64)blockIdx.x * 256 + threadIdx.x;
    if (f < k) P[fstart[f]] = T[factor_end(fstart, k, n, f) - 1];
}
__global__ __launch_bounds__(256) void carried_head_fix_kernel(const u8 *__restrict__ T, u64 n, const u32 *__restrict__ fstart, u64 k, KeyStore ks)
{
    const u64 f = (u64)blockIdx.x * 256 + threadIdx.x;
    if (f >= k) return;
    const u64 p = fstart[f];
    const u8 last = T[factor_end(fstart, k, n, f) - 1];
    if (ks.c16) ks.c[2 * p + 1] = last; else ks.c[p] = last;
}
__global__ __launch_bounds__(256) void emit_kernel(const u32 *__restrict__ SA, const u8 *__restrict__ P, u64 n, u8 *__restrict__ out)
{
    // 8 slots per thread: two 16-byte index loads, eight independent gathers in flight, one packed 8-byte store
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 i = q * 8;
    if (i + 8 <= n && ((uintptr_t)out & 7) == 0) {
        const uint4 s0 = *(const uint4 *)(SA + i), s1 = *(const uint4 *)(SA + i + 4);
        const u32 b0 = P[s0.x], b1 = P[s0.y], b2 = P[s0.z], b3 = P[s0.w], b4 = P[s1.x], b5 = P[s1.y], b6 = P[s1.z], b7 = P[s1.w];
        const u32 lo = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24), hi = b4 | (b5 << 8) | (b6 << 16) | (b7 << 24);
        *(uint2 *)(out + i) = make_uint2(lo, hi);
    } else {
        for (u64 j = i; j < n && j < i + 8; j++) out[j] = P[SA[j]];
    }
}

// bytes of elements that the later rounds moved: out[slot] = P[sa[slot]]
// P == nullptr (split keys: no previous-symbol array was built): T[cprev(p)] is looked up through the factor list
__global__ __launch_bounds__(256) void patch_ties_kernel(const u32 *__restrict__ slots, u64 a, const u32 *__restrict__ SA,
                                                         const u8 *__restrict__ P, const u8 *__restrict__ T, u64 n,
                                                         const u32 *__restrict__ fstart, u64 k, u8 *__restrict__ out)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= a) return;
    const u32 r = slots[i];
    const u64 p = SA[r];
    if (P) { out[r] = P[p]; return; }
    const u64 f = factor_of(fstart, k, p);
    out[r] = fstart[f] == p ? T[factor_end(fstart, k, n, f) - 1] : T[p - 1];
}

#include "wide_path.h"

// ------------------------------------------------------------------------------------
// independent segments: the cyclic sort emitted every byte in global rank order; segment s's bytes go to [off_s, off_s + len_s)
// in that order (a stable partition by the segment of SA[r]).  Key = segment << 8 | byte, LSD passes on the segment bits only.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_fill_kernel(const u64 *__restrict__ seg_off, u64 count, u32 *__restrict__ segid)
{
    const u64 s = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= count) return;
    const u64 end = seg_off[s + 1];
    for (u64 p = seg_off[s] + (u64)lane_id(); p < end; p += 64) segid[p] = (u32)s;
}
__global__ __launch_bounds__(256) void seg_keys_kernel(const u32 *__restrict__ SA, const u32 *__restrict__ segid, const u8 *__restrict__ bytes, u64 n,
                                                       u64 *__restrict__ keys)
{
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r < n) keys[r] = ((u64)segid[SA[r]] << 8) | bytes[r];
}
__global__ __launch_bounds__(256) void seg_bytes_kernel(const u64 *__restrict__ keys, u64 n, u8 *__restrict__ out)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (u8)keys[i];
}

static int partition_by_segment(bwts_ctx *ctx, u64 n, const SegTable &seg, SortSpace &sp, const u32 *SA, u8 *d_out)
{
    // after the sort only SA (one of the value buffers) and the output are live: the other value buffer takes the segment ids, the
    // two key buffers the sort
    u32 *segid = SA == sp.vals[0] ? sp.vals[1] : sp.vals[0];
    int sbits = bitlen_u64(seg.count - 1);
    if (sbits < 1) sbits = 1;
    {
        SpanGuard g(ctx, BWTS_K_OTHER, n, 4 * n);
        seg_fill_kernel<<<dim3((unsigned)((seg.count + 3) / 4)), dim3(256), 0, ctx->stream>>>(seg.d_off, seg.count, segid);
        seg_keys_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(SA, segid, d_out, n, sp.keys[0]);
        HIPC(hipGetLastError());
    }
    int res = 0;
    u64 *keys[2] = {sp.keys[0], sp.keys[1]};
    BWTS_TRY(radix_sort_keys(ctx, keys, sp.tile_hist, sp.scan_temp, n, 8, sbits, &res));
    {
        SpanGuard g(ctx, BWTS_K_OTHER, n, 9 * n);
        seg_bytes_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(keys[res], n, d_out);
        HIPC(hipGetLastError());
    }
    return BWTS_OK;
}

// is the input one byte value repeated?  Eight probes, then -- only if they agree -- the byte histogram.
int constant_input_probe(bwts_ctx *ctx, const u8 *d_in, u64 n, bool *constant)
{
    *constant = false;
    u8 probe[8];
    for (int i = 0; i < 8; i++) HIPC(hipMemcpyAsync(&probe[i], d_in + (n - 1) / 7 * (u64)i, 1, hipMemcpyDefault, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    for (int i = 1; i < 8; i++) if (probe[i] != probe[0]) return BWTS_OK;
    BWTS_TRY(byte_histogram_device(ctx, d_in, n, ctx->d_small));
    BWTS_TRY(read_small(ctx, 0, 256));
    int present = 0;
    for (int c = 0; c < 256; c++) present += ctx->h_small[c] ? 1 : 0;
    *constant = present == 1;
    return BWTS_OK;
}

// One byte value only: n factors of one symbol, every rotation equal -- the transform is the identity (mk_bwts_sa.c:172-188 emits
// each factor's own last byte).
static int emit_identity(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, hipMemcpyKind kind)
{
    HIPC(hipMemcpyAsync(d_out, d_in, n, kind, ctx->stream));
    ctx->tm.factors = n; ctx->tm.rounds = 1; ctx->tm.lyndon_rounds = 0; ctx->tm.active_after_round0 = 0;
    ctx->tm.key_symbols = 1; ctx->tm.key_bits = 1;
    return BWTS_OK;
}

// The sort's inputs (SortSpace, section 2).  P[p] = T[cprev(p)] (mk_bwts_sa.c:172-188): a factor's head takes the factor's last byte.
// With split keys the byte already travels in the keys' c stream and no array is built: P stays null, and the carried-byte
// buffers only hold the round-0 flag words.  Else side slot 3 holds P and, when the bytes ride on the sort, the two buffers.
static int carry_setup(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, FwdArena &A, bool carry, const u32 *d_fstart, u64 k, u8 *&P)
{
    SortSpace &sp = A.sp;
    const size_t n1 = align_up((size_t)n, 256);
    if (!sp.split_keys) {
        char *pc = nullptr;
        BWTS_TRY(aux_reserve_slot(ctx, 3, carry ? 3 * n1 : n1, &pc));
        P = (u8 *)pc;
        SpanGuard g(ctx, BWTS_K_OTHER, n, 2 * n);
        u64 blocks = (n / 16 + 255) / 256 + 1; if (blocks > 8192) blocks = 8192;
        prevsym_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(d_in, n, P);
        prevsym_fix_kernel<<<dim3((unsigned)((k + 255) / 256)), dim3(256), 0, ctx->stream>>>(d_in, n, d_fstart, k, P);
        HIPC(hipGetLastError());
    }
    if (carry) {
        sp.carry_src = P;
        sp.carry_buf[0] = sp.split_keys ? A.flag_words[0] : P + n1;
        sp.carry_buf[1] = sp.split_keys ? A.flag_words[1] : P + 2 * n1;
        sp.carry_out = d_out;
    }
    return BWTS_OK;
}

// emission: either it rode on the sort (only the tied elements are patched), or a gather
static int emit(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, const SortSpace &sp, const u32 *SA, const u8 *P, const u32 *d_fstart, u64 k)
{
    if (sp.carry_out && sp.tie_count && !sp.ties_emitted) {
        SpanGuard g(ctx, BWTS_K_EMIT, sp.tie_count, 6 * sp.tie_count);
        patch_ties_kernel<<<dim3((unsigned)((sp.tie_count + 255) / 256)), dim3(256), 0, ctx->stream>>>(sp.tie_slots, sp.tie_count, SA, P, d_in, n, d_fstart, k, d_out);
    } else if (!sp.carry_out) {
        SpanGuard g(ctx, BWTS_K_EMIT, n, 6 * n);
        emit_kernel<<<dim3((unsigned)(((n + 7) / 8 + 255) / 256)), dim3(256), 0, ctx->stream>>>(SA, P, n, d_out);
    }
    HIPC(hipGetLastError());
    return BWTS_OK;
}

static int forward_run(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, const SegTable *seg)
{
    ctx->fwd_sorts_made = 0;
    // beyond 32-bit indices: the blocked path with 64-bit positions and ranks (wide_path.h).  BWTS_FORCE_WIDE=1 sends every
    // input there, falling back when the wide form cannot take it; =2 does not fall back (tests)
    const int force_wide = [ctx] { const char *e = bwts_knob(ctx, "BWTS_FORCE_WIDE"); return e ? atoi(e) : 0; }();
    if (!seg && n > 0x100000000ull) {
        // one byte value only, beyond 2^32 (every position is a factor and a candidate: the wide path's factor search would refuse it
        // with BWTS_E_RANGE): the identity, as below -- eight probes first, the histogram only if they agree
        bool constant = false;
        BWTS_TRY(constant_input_probe(ctx, d_in, n, &constant));
        if (constant) return emit_identity(ctx, d_in, n, d_out, hipMemcpyDefault);
    }
    if (!seg && (n > 0x100000000ull || force_wide)) {
        const int rc = forward_wide_impl(ctx, d_in, n, d_out);
        if (n > 0x100000000ull || force_wide == 2 || rc != BWTS_E_RANGE) return rc;
    }
    // One byte value only.  Taken before anything is allocated: at n = 2^32 this is the input on which every position stays
    // tied, which the tied-list buffers (32-bit slots) cannot hold.
    BWTS_TRY(read_histogram(ctx, d_in, n));
    int present = 0;
    for (int c = 0; c < 256; c++) present += ctx->h_small[SM_HIST + c] ? 1 : 0;
    if (present == 1) return emit_identity(ctx, d_in, n, d_out, hipMemcpyDeviceToDevice);
    BWTS_TRY(arena_reserve(ctx, forward_arena_bytes(n)));
    FwdArena A;
    BWTS_TRY(fwd_arena_place(ctx, n, A));
    SortSpace &sp = A.sp;

    // 1. Lyndon factors + round-0 keys
    Alphabet al;
    u32 *d_fstart = nullptr, lrounds = 0;
    u64 k = 0;
    const char *emit_env = bwts_knob(ctx, "BWTS_EMIT");      // carry (default) | gather
    // (segments: the partition below needs the whole suffix array, which the sort rebuilds for its tied elements only when no byte
    // rides on it -- the gather emission)
    const bool carry = !seg && !(emit_env && !strcmp(emit_env, "gather"));
    sp.want_split = carry;                           // the byte stream rides round 0 => the packed passes may take split keys
    BWTS_TRY(factors_and_keys(ctx, d_in, n, A, &al, &d_fstart, &k, &lrounds, true, seg));
    ctx->tm.factors = k; ctx->tm.lyndon_rounds = lrounds; ctx->tm.key_symbols = (u32)al.msym; ctx->tm.key_bits = (u32)al.key_bits;
    u8 *P = nullptr;
    BWTS_TRY(carry_setup(ctx, d_in, n, d_out, A, carry, d_fstart, k, P));

    // 2. cyclic sort
    u32 *SA = nullptr, rounds = 0;
    u64 active0 = 0;
    BWTS_TRY((doubling_sort<true>(ctx, d_in, n, al, d_fstart, k, sp, false, &SA, &rounds, &active0)));
    ctx->tm.rounds = rounds; ctx->tm.active_after_round0 = active0;

    // 3. emission, and the segments' bytes to their places
    BWTS_TRY(emit(ctx, d_in, n, d_out, sp, SA, P, d_fstart, k));
    if (seg) BWTS_TRY(partition_by_segment(ctx, n, *seg, sp, SA, d_out));
    return BWTS_OK;
}

int forward_device_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out) { return forward_run(ctx, d_in, n, d_out, nullptr); }

// one wave per segment moves its bytes between the caller's layout (at src_off[s]) and the packed block of the short segments (at off[s])
__global__ __launch_bounds__(256) void seg_move_kernel(const u8 *__restrict__ from, u8 *__restrict__ to, const u64 *__restrict__ off,
                                                       const u64 *__restrict__ src_off, u64 count, int gather)
{
    const u64 s = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= count) return;
    const u64 a = off[s], len = off[s + 1] - a, b = src_off[s];
    const u64 fb = gather ? b : a, tb = gather ? a : b;
    for (u64 i = (u64)lane_id(); i < len; i += 64) to[tb + i] = from[fb + i];
}

int forward_segments_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out)
{
    const std::vector<u64> &off = ctx->seg_off;
    const u64 count = (u64)off.size() - 1;
    if (count == 1) return forward_run(ctx, d_in, n, d_out, nullptr);
    // A segment of `big` bytes or more gains nothing from the shared pass and would cost its length in sequential Duval steps there:
    // it is transformed alone, straight into its place.  BWTS_SEG_FWD_BIG (test switch) moves the line: 1 = every segment alone.
    u64 big = SEG_FWD_BIG;
    if (const char *e = bwts_knob(ctx, "BWTS_SEG_FWD_BIG")) { const long long v = atoll(e); if (v >= 1) big = (u64)v; }
    u64 nshort = 0, m = 0, factors = 0;
    u32 rounds = 0;
    for (u64 s = 0; s < count; s++) {
        const u64 len = off[s + 1] - off[s];
        if (len < big) { nshort++; m += len; }
    }
    if (nshort == count) {
        SegTable seg{d_seg_off(ctx), count, nullptr};
        BWTS_TRY(seg_scratch_reserve(ctx, n, &seg.flag));
        return forward_run(ctx, d_in, n, d_out, &seg);
    }
    for (u64 s = 0; s < count; s++) {
        const u64 len = off[s + 1] - off[s];
        if (len < big) continue;
        BWTS_TRY(forward_run(ctx, d_in + off[s], len, d_out + off[s], nullptr));
        factors += ctx->tm.factors;
        if (ctx->tm.rounds > rounds) rounds = ctx->tm.rounds;
    }
    if (nshort) {
        // the short segments, packed into one block: table (nshort + 1 words) and their places in the caller's buffers (nshort words)
        std::vector<u64> tab(2 * nshort + 1);
        u64 j = 0;
        tab[0] = 0;
        for (u64 s = 0; s < count; s++) {
            const u64 len = off[s + 1] - off[s];
            if (len >= big) continue;
            tab[nshort + 1 + j] = off[s];
            tab[j + 1] = tab[j] + len;
            j++;
        }
        u64 *d_tab = nullptr;
        BWTS_TRY(seg_upload_extra(ctx, tab.data(), tab.size(), &d_tab));
        u8 *scr = nullptr;
        const size_t m1 = align_up((size_t)m, 256);
        BWTS_TRY(seg_scratch_reserve(ctx, 3 * m1, &scr));
        u8 *pin = scr, *pout = scr + m1;
        const unsigned blocks = (unsigned)((nshort + 3) / 4);
        seg_move_kernel<<<dim3(blocks), dim3(256), 0, ctx->stream>>>(d_in, pin, d_tab, d_tab + nshort + 1, nshort, 1);
        HIPC(hipGetLastError());
        if (nshort == 1) BWTS_TRY(forward_run(ctx, pin, m, pout, nullptr));
        else {
            SegTable seg{d_tab, nshort, scr + 2 * m1};
            BWTS_TRY(forward_run(ctx, pin, m, pout, &seg));
        }
        seg_move_kernel<<<dim3(blocks), dim3(256), 0, ctx->stream>>>(pout, d_out, d_tab, d_tab + nshort + 1, nshort, 0);
        HIPC(hipGetLastError());
        factors += ctx->tm.factors;
        if (ctx->tm.rounds > rounds) rounds = ctx->tm.rounds;
    }
    ctx->tm.n = n;
    ctx->tm.factors = factors;
    ctx->tm.rounds = rounds;
    return BWTS_OK;
}
