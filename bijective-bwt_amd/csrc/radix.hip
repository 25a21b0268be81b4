// radix.hip -- stable 8-bit LSD radix sort of (u64 key, u32 value) pairs, with an optional byte stream riding along.
//
// This replaces the inside of divsufsort() (call site /root/reference/mk_bwts_sa.c:48):
// the engine sorts suffixes / rotations by prefix doubling, and every doubling round is
// an LSD radix sort of packed keys.  One pass = three launches:
//   histogram kernel      per-tile 256-bin digit histogram (LDS, per-wave private bins)
//   column scan           exclusive scan of the [tile][digit] table in digit-major order
//   scatter kernel        per-wave ballot ranking, LDS-staged tile sort, coalesced scatter
// Two families of pass kernels:
//   radix_scatter2_kernel         wide streams: u64 key, u32 value (+ u8 byte); 2*(8+4[+1]) bytes per element and pass.
//                                 Later rounds, keys wider than 40 bits.
//   radix_scatter_packed_kernel   round 0 of the forward transform with keys of <= 40 bits: packed streams, 2*(4+4+2) bytes
//                                 (see "packed streams" below).
//   radix_scatter_lean_last_kernel  the last of five packed passes when few positions are expected to stay tied: the byte out,
//                                 and the group flags of its own output instead of sorted keys and values; 7 bytes per element.
// All are built from the same blocks: RxTile (the tile's place and its LDS), wave_rank_step and digit_bases / digit_bases_folded (device_utils.h),
// Pos16; radix_hist_kernel<T> counts the digits of whichever stream holds them.  The packed and the lean kernels rank part of a
// thread's items with one returning LDS add each instead of the ballots (rank_split, wave_rank_atomic_step).
#include "internal.h"
#include "device_utils.h"
#include "scan_templ.h"

#include <stdlib.h>

#define RX_CHUNK   128          // tiles per column-scan chunk
#define RX_XCDS    8
// the one tile shape: 512 threads x 16 items, at least 4 waves per SIMD -- two 8192-element tiles resident per CU
constexpr int RX_THREADS = 512, RX_ITEMS = 16, RX_MINW = 4, RX_WAVES = RX_THREADS / 64, RX_TILE = RX_THREADS * RX_ITEMS;
constexpr u64 RX_HIST_TILE = 3072;      // radix_tile_hist_bytes() sizes the table for tiles of this many elements

// Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share one), and each XCD has its own
// non-coherent L2.  Tile t's run for digit d is followed in memory by tile t+1's run, so the two share a
// cache line at the seam: give every XCD a CONTIGUOUS range of tiles, walked in dispatch order, so that
// both halves of a seam line are written through the same L2 close in time and leave it as one full line.
// Placement only changes speed, never results.
__device__ __forceinline__ u64 rx_tile_of_block(u64 tiles)
{
    const u64 per = (tiles + RX_XCDS - 1) / RX_XCDS;
    return (u64)(blockIdx.x % RX_XCDS) * per + (u64)(blockIdx.x / RX_XCDS);
}
static inline u64 rx_grid(u64 tiles) { return (tiles + RX_XCDS - 1) / RX_XCDS * RX_XCDS; }

static inline u64 rx_tiles(u64 m) { return (m + RX_TILE - 1) / RX_TILE; }
static inline u64 radix_chunks(u64 tiles) { return (tiles + RX_CHUNK - 1) / RX_CHUNK; }

size_t radix_tile_hist_bytes(u64 m)
{
    // sized for tiles of RX_HIST_TILE elements, so one size serves every user: the radix passes' 8192-element tiles and the inverse's
    // 4096-element LF tiles (inverse.hip, wide_inverse.h).  Every arena reservation that holds the table depends on this value.
    const u64 tiles = (m + RX_HIST_TILE - 1) / RX_HIST_TILE + 1;
    return align_up((size_t)tiles * 256 * sizeof(u32), 256) +
           align_up((size_t)radix_chunks(tiles) * 256 * sizeof(u32), 256);
}

// ------------------------------------------------------------------------------------
// generic in-place exclusive sum (used for the chunk table and elsewhere)
// ------------------------------------------------------------------------------------
struct LoadU32  { const u32 *p; __device__ __forceinline__ u32 operator()(u64 i) const { return p[i]; } };
struct StoreU32 { u32 *p; __device__ __forceinline__ void operator()(u64 i, u32 v) const { p[i] = v; } };

size_t scan_temp_bytes(u64 n) { return scan_temp_bytes_t(n, sizeof(u64)); }

int exclusive_sum_u32(bwts_ctx *ctx, u32 *data, u64 n, void *temp)
{
    LoadU32 in{data};
    StoreU32 out{data};
    return device_scan<false, u32>(ctx, n, in, out, OpAdd(), (u32)0, temp);
}

// ------------------------------------------------------------------------------------
// pass kernels
// ------------------------------------------------------------------------------------
// per-tile digit counts of one stream: the u64 keys, or the packed passes' lo (u32) / c (u16) streams
template <typename T>
__global__ __launch_bounds__(RX_THREADS) void radix_hist_kernel(const T *__restrict__ src, u64 m, int shift, u32 *__restrict__ tile_hist)
{
    __shared__ u32 bins[RX_WAVES][256];
    const int tid = threadIdx.x, w = tid >> 6;
    for (int i = tid; i < RX_WAVES * 256; i += RX_THREADS) ((u32 *)bins)[i] = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * RX_TILE;
    // all loads first (one register (pair) each), then the LDS atomics: keeps 16 loads in flight per lane
    T k[RX_ITEMS];
#pragma unroll
    for (int j = 0; j < RX_ITEMS; j++) {
        const u64 i = base + (u64)j * RX_THREADS + tid;
        k[j] = i < m ? src[i] : (T)0;
    }
#pragma unroll
    for (int j = 0; j < RX_ITEMS; j++) {
        const u64 i = base + (u64)j * RX_THREADS + tid;
        hist_add_runs(bins[w], (u32)(k[j] >> shift) & 255u, i < m);
    }
    __syncthreads();
    if (tid < 256) {
        u32 s = 0;
#pragma unroll
        for (int ww = 0; ww < RX_WAVES; ww++) s += bins[ww][tid];
        tile_hist[(u64)blockIdx.x * 256 + tid] = s;
    }
}

// column sums of a chunk of tiles: chunk_sum[d * chunks + c]
__global__ __launch_bounds__(256) void radix_chunk_sum_kernel(const u32 *__restrict__ tile_hist, u64 tiles, u64 chunks,
                                                              u32 *__restrict__ chunk_sum)
{
    const u64 c = blockIdx.x;
    const u64 t0 = c * RX_CHUNK;
    const u64 t1 = t0 + RX_CHUNK < tiles ? t0 + RX_CHUNK : tiles;
    u32 s = 0;
    for (u64 t = t0; t < t1; t++) s += tile_hist[t * 256 + threadIdx.x];
    chunk_sum[(u64)threadIdx.x * chunks + c] = s;
}

// turns per-tile counts into global exclusive offsets, in place
__global__ __launch_bounds__(256) void radix_chunk_apply_kernel(u32 *__restrict__ tile_hist, u64 tiles, u64 chunks,
                                                                const u32 *__restrict__ chunk_off)
{
    const u64 c = blockIdx.x;
    const u64 t0 = c * RX_CHUNK;
    const u64 t1 = t0 + RX_CHUNK < tiles ? t0 + RX_CHUNK : tiles;
    u32 run = chunk_off[(u64)threadIdx.x * chunks + c];
    for (u64 t = t0; t < t1; t++) {
        const u32 v = tile_hist[t * 256 + threadIdx.x];
        tile_hist[t * 256 + threadIdx.x] = run;
        run += v;
    }
}

// The scatter kernels' dynamic LDS: the six arrays, each at its byte offset from the dynamic base, and their total.  Kernels take
// the pointers from here and launches the byte count, so the two cannot drift apart.  (The pointers are handed out one by one and
// kept in locals: held in an object, or with the tile's place computed in a shared function, the same arithmetic cost some
// instantiations a VGPR more or less.)  The LDS tile holds the keys first and is then
// reused for the values (and, optionally, a third one-byte stream), the per-wave digit counters are 16-bit and each slot's digit is
// kept in a byte table, so the destination of a slot is re-derived instead of living in a register: 9 B of LDS per element instead
// of 12, two 8192-element tiles fit a CU and one tile's loads overlap the other's ranking.  That is the wide kernel
// (radix_scatter2_kernel), whose registers are full.  The packed kernels have sixteen to spare: both their write-outs give a thread
// the same slots, so it keeps each slot's destination base from the first to the second and has no byte table (bytes_no_sdig).
template <int THREADS, int ITEMS>
struct RxTile {
    static constexpr int WAVES = THREADS / 64, TILE = THREADS * ITEMS;
    static constexpr size_t off_dbase = (size_t)TILE * sizeof(u64), off_gbase = off_dbase + 256 * sizeof(u32),
                            off_scan = off_gbase + 256 * sizeof(u32), off_whist = off_scan + 16 * sizeof(u32),
                            off_sdig = off_whist + (size_t)WAVES * 256 * sizeof(u16), bytes = off_sdig + TILE;
    // what a kernel without the byte table asks for (the packed passes, the lean last pass): everything in front of it
    static constexpr size_t bytes_no_sdig = off_sdig;
    // TILE slots: the first stream (keys; the packed passes' u32 digit stream), then the others (values; uint2 pairs)
    static __device__ __forceinline__ u64 *stage(char *smem) { return (u64 *)smem; }
    // WAVES x 256 u32 in the front of the stage area, which is idle until the first staging trip: the counters of a ranking that
    // takes the atomic step (rank_split); digit_bases_folded reads them for the last time before the barriers of its scan
    static_assert((size_t)WAVES * 256 * sizeof(u32) <= off_dbase, "the counters fit the stage area");
    static __device__ __forceinline__ u32 (*cnt(char *smem))[256] { return (u32 (*)[256])smem; }
    // 256 each: the digit's first slot in the tile (not used where digit_bases_folded has put it into the waves' starts); its run's
    // global start minus that slot
    static __device__ __forceinline__ u32 *dbase(char *smem) { return (u32 *)(smem + off_dbase); }
    static __device__ __forceinline__ u32 *gbase(char *smem) { return (u32 *)(smem + off_gbase); }
    // WAVES words (padded to 16) for block_scan_exclusive
    static __device__ __forceinline__ u32 *scan_sm(char *smem) { return (u32 *)(smem + off_scan); }
    // WAVES x 256: the waves' digit counters, then each wave's start inside the digit
    static __device__ __forceinline__ u16 (*whist(char *smem))[256] { return (u16 (*)[256])(smem + off_whist); }
    // TILE: digit of the element in slot s
    static __device__ __forceinline__ u8 *sdig(char *smem) { return (u8 *)(smem + off_sdig); }
};
static_assert(RxTile<RX_THREADS, RX_ITEMS>::bytes == 79936, "9 B per element + 6208: two tiles per CU");
static_assert(RxTile<RX_THREADS, RX_ITEMS>::bytes_no_sdig == 71744, "8 B per element + 6208");

// one byte per item, four to a register (the key bytes that the last pass over 40-bit keys holds back for the second write-out)
template <int ITEMS>
struct Dig8 {
    static_assert(ITEMS % 4 == 0, "packed as bytes");
    u32 p[ITEMS / 4];
    __device__ __forceinline__ u32 get(int j) const { return (p[j >> 2] >> (8 * (j & 3))) & 255u; }
    // the first write of a quad: its first item sets the register, the others join it (d < 256)
    __device__ __forceinline__ void init(int j, u32 d) { if (j & 3) p[j >> 2] |= d << (8 * (j & 3)); else p[j >> 2] = d; }
};

// the items' 16-bit tile positions, two per register
template <int ITEMS>
struct Pos16 {
    static_assert(ITEMS % 2 == 0, "positions are packed as 16-bit pairs");
    u32 p[ITEMS / 2];
    __device__ __forceinline__ u32 get(int j) const { return (j & 1) ? p[j >> 1] >> 16 : p[j >> 1] & 0xffffu; }
    __device__ __forceinline__ void set(int j, u32 v)
    {
        if (j & 1) p[j >> 1] = (p[j >> 1] & 0xffffu) | (v << 16); else p[j >> 1] = (p[j >> 1] & 0xffff0000u) | v;
    }
    // the first write of a pair: the even item sets the register, the odd one joins it
    __device__ __forceinline__ void init(int j, u32 v) { if (j & 1) p[j >> 1] |= v << 16; else p[j >> 1] = v; }
};

// The ranking of a packed tile, split between two units (device_utils.h): the wave's first K items take wave_rank_atomic_step, the
// others wave_rank_step, in the order of j and on the same u32 counters, so the ranks are those of sixteen ballot steps.  The
// atomics go out back to back -- their returns wait in ra[] -- and the LDS unit serves them while the VALU works on the
// ballots of the items behind them.  digit(j), valid(j): item j's.  K is even: positions are packed in pairs.
// K = 12 in every pass: measured over K = 0 .. 16 (profiles/history/rank_split.md).  All sixteen atomic is
// faster still on random digits and loses 5 % of a middle pass on text, whose sorted keys put runs of one digit into a wave:
// a same-address atomic serves its lanes one by one, the ballot step does not care.
constexpr int RX_ATOMIC_FIRST = 12, RX_ATOMIC_MIDDLE = 12, RX_ATOMIC_LAST = 12, RX_ATOMIC_LEAN = 12;
template <int K, typename D, typename V>
__device__ __forceinline__ void rank_split(u32 *wave_cnt, Pos16<RX_ITEMS> &pos, D digit, V valid)
{
    static_assert(K >= 0 && K <= RX_ITEMS && K % 2 == 0, "whole pairs of items");
    u32 ra[K ? K : 1];
#pragma unroll
    for (int j = 0; j < K; j++) {
        ra[j] = 0;
        wave_rank_atomic_step(wave_cnt, digit(j), valid(j), [&](u32 r) { ra[j] = r; });
    }
#pragma unroll
    for (int j = K; j < RX_ITEMS; j++) wave_rank_step(wave_cnt, digit(j), valid(j), [&](u32 r) { pos.init(j, r); });
#pragma unroll
    for (int j = 0; j < K; j++) pos.init(j, ra[j]);
}

template <int TH, int IT, int MINW, bool HAS_SYM, bool IDENT, bool KEYS_ONLY = false>
__global__ __launch_bounds__(TH, MINW) void radix_scatter2_kernel(const u64 *__restrict__ kin, const u32 *__restrict__ vin,
                                                                     u64 *__restrict__ kout, u32 *__restrict__ vout,
                                                                     const u32 *__restrict__ tile_off, u64 m, int shift,
                                                                     const u8 *__restrict__ sin, u8 *__restrict__ sout)
{
    using L = RxTile<TH, IT>;
    constexpr int WAVES = L::WAVES, TILE = L::TILE;
    static_assert(TILE <= 65536, "positions are 16-bit");
    extern __shared__ __attribute__((aligned(16))) char rx_smem[];
    u64 *stage = L::stage(rx_smem);
    u32 *dbase = L::dbase(rx_smem), *gbase = L::gbase(rx_smem), *scan_sm = L::scan_sm(rx_smem);
    u16 (*whist)[256] = L::whist(rx_smem);
    u8 *sdig = L::sdig(rx_smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const u64 tile = rx_tile_of_block((m + TILE - 1) / TILE);
    const u64 tile_base = tile * TILE;
    if (tile_base >= m) return;                                   // padding block of the XCD-aligned grid
    const u64 wave_base = tile_base + (u64)w * (64 * IT);
    const u64 remain = m - tile_base;
    const u32 tile_count = remain < TILE ? (u32)remain : (u32)TILE;

    for (int i = tid; i < WAVES * 128; i += TH) ((u32 *)whist)[i] = 0;

    u64 key[IT];
    Pos16<IT> pos;
#pragma unroll
    for (int j = 0; j < IT; j++) {
        const u64 i = wave_base + (u64)j * 64 + lane;
        key[j] = i < m ? kin[i] : ~0ull;
    }
    __syncthreads();

#pragma unroll
    for (int j = 0; j < IT; j++) {
        const bool valid = wave_base + (u64)j * 64 + lane < m;
        const u32 d = (u32)(key[j] >> shift) & 255u;
        wave_rank_step(whist[w], d, valid, [&](u32 r) { pos.init(j, r); });
    }
    __syncthreads();
    {
        const u32 exc = digit_bases<WAVES>(whist, scan_sm);
        if (tid < 256) {
            dbase[tid] = exc;
            gbase[tid] = tile_off[tile * 256 + tid] - exc;
        }
    }
    __syncthreads();

    // From here on every loop is split into "all LDS reads", then "all dependent work": inside one loop body the
    // compiler keeps a read, its s_waitcnt and the dependent LDS/global operation together, which serialises sixteen
    // LDS round trips per phase (seen in the ISA); batched, a phase costs about one.
    constexpr int HB = IT % 8 == 0 ? 8 : 4;                  // LDS reads batched per phase step
#pragma unroll
    for (int j0 = 0; j0 < IT; j0 += HB) {
        u32 add[HB];
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const u32 d = (u32)(key[j0 + jj] >> shift) & 255u;
            add[jj] = dbase[d] + whist[w][d];
        }
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const int j = j0 + jj;
            const bool valid = wave_base + (u64)j * 64 + lane < m;
            const u32 p = pos.get(j) + add[jj];
            pos.set(j, p);
            if (valid) stage[p] = key[j];
        }
    }
    // the keys' registers are free: the value (and byte) loads overlap the key write-out
    u32 val[KEYS_ONLY ? 1 : IT];
    u32 sym[HAS_SYM ? IT : 1];
    if (!KEYS_ONLY) {
#pragma unroll
        for (int j = 0; j < IT; j++) {
            const u64 i = wave_base + (u64)j * 64 + lane;
            val[KEYS_ONLY ? 0 : j] = IDENT ? (u32)i : (i < m ? vin[i] : 0u);          // first pass of a sort over positions: value = index
        }
    }
    if (HAS_SYM) {
        // one register per byte and no arithmetic on them here: the 16 loads issue back to back (packing them
        // on arrival made the compiler wait for memory after every two or three loads)
#pragma unroll
        for (int j = 0; j < IT; j++) {
            const u64 i = wave_base + (u64)j * 64 + lane;
            sym[j] = i < m ? (u32)sin[i] : 0u;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j0 = 0; j0 < IT; j0 += HB) {
        u64 k[HB];
        u32 g[HB];
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const u32 s = (u32)(j0 + jj) * TH + tid;
            k[jj] = s < tile_count ? stage[s] : 0ull;
        }
#pragma unroll
        for (int jj = 0; jj < HB; jj++) g[jj] = gbase[(u32)(k[jj] >> shift) & 255u];
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const u32 s = (u32)(j0 + jj) * TH + tid;
            if (s < tile_count) {
                sdig[s] = (u8)((u32)(k[jj] >> shift) & 255u);
                kout[g[jj] + s] = k[jj];
            }
        }
    }
    if (KEYS_ONLY) return;                                          // a sort of bare keys (the payload sits in their upper bits)
    __syncthreads();
    // second trip through the same LDS: the value, with the travelling byte in the upper half of the slot
#pragma unroll
    for (int j = 0; j < IT; j++) {
        const bool valid = wave_base + (u64)j * 64 + lane < m;
        const u32 p = pos.get(j);
        if (valid) {
            if (HAS_SYM) stage[p] = (u64)val[KEYS_ONLY ? 0 : j] | ((u64)sym[j] << 32);
            else ((u32 *)stage)[p] = val[KEYS_ONLY ? 0 : j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j0 = 0; j0 < IT; j0 += HB) {
        u64 e[HAS_SYM ? HB : 1];
        u32 v32[HAS_SYM ? 1 : HB];
        u32 g[HB];
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const u32 s = (u32)(j0 + jj) * TH + tid;
            const u32 sc = s < tile_count ? s : 0u;
            if (HAS_SYM) e[jj] = stage[sc]; else v32[jj] = ((u32 *)stage)[sc];
            g[jj] = sdig[sc];
        }
#pragma unroll
        for (int jj = 0; jj < HB; jj++) g[jj] = gbase[g[jj]];
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const u32 s = (u32)(j0 + jj) * TH + tid;
            if (s < tile_count) {
                const u32 dst = g[jj] + s;
                if (HAS_SYM) { vout[dst] = (u32)e[jj]; sout[dst] = (u8)(e[jj] >> 32); }
                else vout[dst] = v32[jj];
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// packed streams (round 0 of the forward transform)
// ------------------------------------------------------------------------------------
// A round-0 key has at most 40 significant bits, yet a pass of the kernel above moves 8 + 4 + 1 bytes per element.
// Between the first and the last pass the element travels instead as
//     lo  u32   key bits 0..31
//     val u32   the position
//     c   u16   key bits 32..39 | carried byte << 8        (HI16)   -- or u8: the carried byte alone (keys <= 32 bits)
// = 10 (9) bytes, and a histogram sweep reads only the stream that holds its digit (4 or 2 bytes, not 8).
// keybuild leaves lo and c in exactly this form (forward.hip, KeyStore) and counts the first pass's digits while it writes them
// (SortPlan::first_hist), the first pass supplies value = index, and the last pass leaves the sorted keys split as well: lo, and
// for keys of more than 32 bits their bits 32..39 as one byte (5 bytes per key instead of a u64's 8; K0Split in forward.hip reads
// them).  Ranking, LDS staging and XCD mapping are those of radix_scatter2_kernel; the LDS tile carries the digit's stream on its
// first trip and the other two on its second.
struct PackedIO {
    const u32 *lo_in; const void *c_in;                    // c: u16 if HI16 else u8
    const u32 *val_in;                                     // not read by the first pass (value = index)
    u32 *lo_out;
    void *c_out;                                           // !LAST
    u8 *hi_out, *sym_out;                                  // LAST: key bits 32..39 (HI16), carried byte
    u32 *val_out;
};

template <bool FIRST, bool LAST, bool HI16>
__global__ __launch_bounds__(RX_THREADS, RX_MINW) void radix_scatter_packed_kernel(PackedIO io, const u32 *__restrict__ tile_off, u64 m, int shift)
{
    extern __shared__ __attribute__((aligned(16))) char rx_smem[];
    using L = RxTile<RX_THREADS, RX_ITEMS>;
    u64 *stage = L::stage(rx_smem);
    u32 *gbase = L::gbase(rx_smem), *scan_sm = L::scan_sm(rx_smem);
    u16 (*whist)[256] = L::whist(rx_smem);
    u32 (*cnt)[256] = L::cnt(rx_smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const u64 tile = rx_tile_of_block((m + RX_TILE - 1) / RX_TILE);
    const u64 tile_base = tile * RX_TILE;
    if (tile_base >= m) return;                                   // padding block of the grid
    const u64 wave_base = tile_base + (u64)w * (64 * RX_ITEMS);
    const u64 remain = m - tile_base;
    const u32 tile_count = remain < RX_TILE ? (u32)remain : (u32)RX_TILE;

    for (int i = tid; i < RX_WAVES * 256; i += RX_THREADS) ((u32 *)cnt)[i] = 0;

    // element j of this lane is i0 + 64 j; which of the sixteen exist is decided once (bit j of vmask), so that no
    // 64-bit index has to stay alive for the bounds checks further down
    const u64 i0 = wave_base + (u64)lane;
    u32 vmask = 0;
#pragma unroll
    for (int j = 0; j < RX_ITEMS; j++) vmask |= (i0 + (u64)j * 64 < m ? 1u : 0u) << j;
#define PK_VALID(j) ((vmask >> (j)) & 1u)

    // Only the stream that holds this pass's digit is loaded before the ranking and makes the first LDS trip alone;
    // the other two are loaded while the first trip is written out and share the second trip.
    // With 40-bit keys the fifth (= last) pass sorts by the byte that travels in c.
    constexpr bool DIG_C = HI16 && LAST;
    u32 dsrc[RX_ITEMS];
    Pos16<RX_ITEMS> pos;
    {
        const u16 *c16 = (const u16 *)io.c_in + i0;
        const u32 *lop = io.lo_in + i0;
#pragma unroll
        for (int j = 0; j < RX_ITEMS; j++) {
            if (DIG_C) dsrc[j] = PK_VALID(j) ? (u32)c16[j * 64] : 0xffffu;
            else dsrc[j] = PK_VALID(j) ? lop[j * 64] : ~0u;
        }
    }
#define PK_DIGIT(j) (DIG_C ? (dsrc[j] & 255u) : ((dsrc[j] >> shift) & 255u))
    __syncthreads();

    rank_split<FIRST ? RX_ATOMIC_FIRST : LAST ? RX_ATOMIC_LAST : RX_ATOMIC_MIDDLE>(
        cnt[w], pos, [&](int j) { return PK_DIGIT(j); }, [&](int j) { return (bool)PK_VALID(j); });
    __syncthreads();
    {
        const u32 exc = digit_bases_folded<RX_WAVES>(cnt, whist, scan_sm);   // whist[w][d]: the slot of wave w's first element with digit d
        if (tid < 256) gbase[tid] = tile_off[tile * 256 + tid] - exc;
    }
    __syncthreads();

    constexpr int HB = 8;
    u32 *stage32 = (u32 *)stage;
    // first trip: the digit's stream into its slot
#pragma unroll
    for (int j0 = 0; j0 < RX_ITEMS; j0 += HB) {
        u32 add[HB];
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            add[jj] = whist[w][PK_DIGIT(j0 + jj)];
        }
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const int j = j0 + jj;
            const bool valid = PK_VALID(j);
            const u32 p = pos.get(j) + add[jj];
            pos.set(j, p);
            if (valid) stage32[p] = dsrc[j];
        }
    }
    // the other two streams: (lo, val) on the pass that sorts by c, else (val, c); their loads overlap the write-out below
    u32 sa[RX_ITEMS], sb[RX_ITEMS];
    {
        const u32 *lop = io.lo_in + i0, *valp = io.val_in + i0;
        const u8 *c8 = (const u8 *)io.c_in + i0;
        const u16 *c16 = (const u16 *)io.c_in + i0;
#pragma unroll
        for (int j = 0; j < RX_ITEMS; j++) {
            if (FIRST) sa[j] = 0u;                                   // value = index, formed when it is staged
            else if (DIG_C) sa[j] = PK_VALID(j) ? lop[j * 64] : 0u;
            else sa[j] = PK_VALID(j) ? valp[j * 64] : 0u;
        }
#pragma unroll
        for (int j = 0; j < RX_ITEMS; j++) {
            if (DIG_C) sb[j] = PK_VALID(j) ? valp[j * 64] : 0u;
            else sb[j] = PK_VALID(j) ? (HI16 ? (u32)c16[j * 64] : (u32)c8[j * 64]) : 0u;
        }
    }
    __syncthreads();
    // Both write-outs hand slot (j0 + jj) * RX_THREADS + tid to this thread, and the slot's digit is a field of the word it reads in
    // the first: no table of the slots' digits, and the digit's base (gbase) is looked up once and waits in gs[] for the second
    // write-out.  On the last 40-bit pass the digit is also the key byte that waits for its lo (hi_s, four to a register).  A slot
    // past the tile's end reads slot 0 and is not written.  (The bases pass through g[] on their way into gs[] and out of it again:
    // written straight into gs[] and used from there, the same loops compiled to 100 VGPRs instead of 107 and to passes that ran
    // 0.15 ms per forward slower at 2^30 than the parent's, where this form runs faster: profiles/history/packed_lds_dropped.md.)
    Dig8<DIG_C ? RX_ITEMS : 4> hi_s;
    u32 gs[RX_ITEMS];
#pragma unroll
    for (int j0 = 0; j0 < RX_ITEMS; j0 += HB) {
        u32 x[HB], g[HB];
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const u32 s = (u32)(j0 + jj) * RX_THREADS + tid;
            const u32 sc = s < tile_count ? s : 0u;
            x[jj] = stage32[sc];
        }
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const u32 d = DIG_C ? x[jj] & 255u : (x[jj] >> shift) & 255u;
            if (DIG_C) hi_s.init(j0 + jj, d);
            g[jj] = gbase[d];
        }
#pragma unroll
        for (int jj = 0; jj < HB; jj++) gs[j0 + jj] = g[jj];
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const u32 s = (u32)(j0 + jj) * RX_THREADS + tid;
            if (s < tile_count) {
                const u32 dst = g[jj] + s;
                if (DIG_C) io.sym_out[dst] = (u8)(x[jj] >> 8);
                else io.lo_out[dst] = x[jj];
            }
        }
    }
    __syncthreads();
    // second trip: the pair.  (The index value is rebuilt from an opaque copy of the base: left to itself the compiler
    // keeps the sixteen indices of the load addresses alive from the top of the kernel and spills them.)
    u32 idx_base = (u32)wave_base + (u32)lane;
    asm volatile("" : "+v"(idx_base));
#pragma unroll
    for (int j = 0; j < RX_ITEMS; j++) {
        const bool valid = PK_VALID(j);
        const u32 second = sb[j];
        const u32 firstw = FIRST ? idx_base + (u32)j * 64u : sa[j];
        if (valid) ((uint2 *)stage)[pos.get(j)] = make_uint2(firstw, second);
    }
    __syncthreads();
#pragma unroll
    for (int j0 = 0; j0 < RX_ITEMS; j0 += HB) {
        uint2 e[HB];
        u32 g[HB];
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const u32 s = (u32)(j0 + jj) * RX_THREADS + tid;
            const u32 sc = s < tile_count ? s : 0u;
            e[jj] = ((const uint2 *)stage)[sc];
            g[jj] = gs[j0 + jj];
        }
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const u32 s = (u32)(j0 + jj) * RX_THREADS + tid;
            if (s < tile_count) {
                const u32 dst = g[jj] + s;
                if (DIG_C) {
                    io.lo_out[dst] = e[jj].x;
                    io.hi_out[dst] = (u8)hi_s.get(j0 + jj);
                    io.val_out[dst] = e[jj].y;
                } else {
                    io.val_out[dst] = e[jj].x;
                    if (LAST) io.sym_out[dst] = (u8)e[jj].y;
                    else if (HI16) ((u16 *)io.c_out)[dst] = (u16)e[jj].y;
                    else ((u8 *)io.c_out)[dst] = (u8)e[jj].y;
                }
            }
        }
    }
#undef PK_DIGIT
#undef PK_VALID
}

// The lean last pass of a five-pass sort (SortPlan::lean_last): the carried byte goes out as above, and of the keys only what the
// stages after round 0 ask of them when few positions stay tied: which output slots start a group of equal keys (headw) and which sit
// in a group of more than one (keepw) -- the two bitmaps group_flags_kernel (forward.hip) makes from the sorted keys -- and the
// positions of the tied slots.  Neither lo, the key byte nor the other positions are written: 7 bytes per element instead of 20.
//
// The pass's input is sorted by lo (passes 0..3 covered its 32 bits, stably), so the elements of one lo form a run of the input, and
// the pass is stable: the output neighbour of an element in front, inside its digit, is the nearest element with its digit before it
// in the input, and the two keys are equal iff that one lies in the same run.  Inside the tile that is the slot before it (same
// digit, same lo).  The first slot of a digit's run in the tile has its neighbour in an earlier tile: it can have the same lo only
// when this lo is that of the tile's first element and the run of that value reaches back over the tile's start; then the key is
// equal iff the digit occurs in the part of the run before the tile.  Mirrored for the last slot of a digit's run and the run that
// goes on behind the tile.  Wave 0 looks at LEAN_SEAM elements on either side and keeps, per side, the set of digits in the
// neighbouring run (2 x 256 bits, in its own row of the waves' digit counters, once it has read that for the last time); a run
// that fills them -- one tile in thousands on random keys -- is followed further, LEAN_SEAM elements at a time.  A run of
// LEAN_REACH elements that has not ended (nor the array there) is not decided from here: *giveup is raised, the flags are then
// worthless and the host sorts the classic way (radix_packed_last_pass).  Below that the flags are exact.  (The reach is what lets
// a phrase pasted a few hundred times -- a run of as many equal lo -- through to the stage whose business large groups are.)
// headw comes in all ones (its last word up to m: masking it in here cost the pass 0.6 ms at 2^30), keepw all zeros: a tied slot -- one in
// 250 on the inputs this is chosen for -- sets its keepw bit, clears its headw bit if it equals the slot before, and fetches and
// stores its position.
// With only the byte to write the tile makes one LDS trip where the other passes make two: c and lo are both loaded before the
// ranking and staged together (lo | c with the element's place in the tile, 8 B per slot as ever), and one sweep over the slots
// writes the bytes and looks for equal neighbours: two barriers and a write-out loop fewer (zipf 2^30: 4.10 -> 3.60 ms).  The
// slots' byte table, 8 KB of RxTile, is not used (the digit is c's low byte) and not asked for: bytes_no_sdig, as the packed passes.
#define LEAN_SEAM 64
#define LEAN_REACH 1024
static_assert(LEAN_REACH % LEAN_SEAM == 0 && LEAN_REACH <= RX_TILE, "the elements before a tile that is not the first are all there");
struct LeanIO {
    const u32 *lo_in; const u16 *c_in; const u32 *val_in;
    u8 *sym_out;
    u32 *val_out;                                          // written at tied slots only
    u64 *headw, *keepw, *giveup;
};

__global__ __launch_bounds__(RX_THREADS, RX_MINW) void radix_scatter_lean_last_kernel(LeanIO io, const u32 *__restrict__ tile_off, u64 m)
{
    extern __shared__ __attribute__((aligned(16))) char rx_smem[];
    using L = RxTile<RX_THREADS, RX_ITEMS>;
    u32 *stage32 = (u32 *)L::stage(rx_smem);
    u32 *gbase = L::gbase(rx_smem), *scan_sm = L::scan_sm(rx_smem);
    u16 (*whist)[256] = L::whist(rx_smem);
    u32 (*cnt)[256] = L::cnt(rx_smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const u64 tile = rx_tile_of_block((m + RX_TILE - 1) / RX_TILE);
    const u64 tile_base = tile * RX_TILE;
    if (tile_base >= m) return;                                   // padding block of the grid
    const u64 wave_base = tile_base + (u64)w * (64 * RX_ITEMS);
    const u64 remain = m - tile_base;
    const u32 tile_count = remain < RX_TILE ? (u32)remain : (u32)RX_TILE;

    for (int i = tid; i < RX_WAVES * 256; i += RX_THREADS) ((u32 *)cnt)[i] = 0;

    const u64 i0 = wave_base + (u64)lane;
    u32 vmask = 0;
#pragma unroll
    for (int j = 0; j < RX_ITEMS; j++) vmask |= (i0 + (u64)j * 64 < m ? 1u : 0u) << j;
#define PK_VALID(j) ((vmask >> (j)) & 1u)

    // Both streams are loaded before the ranking: with nothing but the byte to write there is one LDS trip, not two, and lo has to
    // be there for it.  In wave 0 also the LEAN_SEAM elements on either side of the tile.
    u32 dsrc[RX_ITEMS], lo[RX_ITEMS];
    Pos16<RX_ITEMS> pos;
    {
        const u16 *c16 = io.c_in + i0;
        const u32 *lop = io.lo_in + i0;
#pragma unroll
        for (int j = 0; j < RX_ITEMS; j++) dsrc[j] = PK_VALID(j) ? (u32)c16[j * 64] : 0xffffu;
#pragma unroll
        for (int j = 0; j < RX_ITEMS; j++) lo[j] = PK_VALID(j) ? lop[j * 64] : 0u;
    }
    // (a tile that does not start the array has 8192 elements before it; one that is not full has none behind it)
    const bool has_before = tile_base > 0, has_after = tile_base + RX_TILE + (u64)lane < m;
    u32 b_lo = 0, b_c = 0, a_lo = 0, a_c = 0;
    if (w == 0) {
        if (has_before) { const u64 i = tile_base - 1 - (u64)lane; b_lo = io.lo_in[i]; b_c = io.c_in[i]; }
        if (has_after) { const u64 i = tile_base + RX_TILE + (u64)lane; a_lo = io.lo_in[i]; a_c = io.c_in[i]; }
    }
    const u32 lo_first = io.lo_in[tile_base], lo_last = io.lo_in[tile_base + tile_count - 1];       // (uniform addresses: scalar loads)
    __syncthreads();
    rank_split<RX_ATOMIC_LEAN>(cnt[w], pos, [&](int j) { return dsrc[j] & 255u; }, [&](int j) { return (bool)PK_VALID(j); });
    __syncthreads();
    {
        const u32 exc = digit_bases_folded<RX_WAVES>(cnt, whist, scan_sm);
        if (tid < 256) gbase[tid] = tile_off[tile * 256 + tid] - exc;
    }
    __syncthreads();

    // the trip: a slot holds its lo in the stage's first half and, in the second, c | the element's place in the tile << 16 (the
    // digit is c's low byte: the byte table is not used)
    constexpr int HB = 8;
    u32 *lo_s = stage32, *cx_s = stage32 + RX_TILE;
#pragma unroll
    for (int j0 = 0; j0 < RX_ITEMS; j0 += HB) {
        u32 add[HB];
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            add[jj] = whist[w][dsrc[j0 + jj] & 255u];
        }
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const int j = j0 + jj;
            const u32 p = pos.get(j) + add[jj];
            if (PK_VALID(j)) {
                lo_s[p] = lo[j];
                cx_s[p] = dsrc[j] | ((u32)w * (64u * RX_ITEMS) + (u32)j * 64u + (u32)lane) << 16;
            }
        }
    }
    // the seams.  Wave 0 has read its row of the digit counters for the last time just above (nobody else reads that row): the row's
    // first 16 words hold the two sets
    u32 *seam = (u32 *)whist;
    if (w == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (lane < 16) seam[lane] = 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // lanes of a window that belong to the run: those in front of the first that does not match
        const auto in_run = [](u64 match) { return ~match ? (u32)__ffsll((unsigned long long)~match) - 1u : (u32)LEAN_SEAM; };
        u32 run_b = in_run(__ballot(has_before && b_lo == lo_first)), run_a = in_run(__ballot(has_after && a_lo == lo_last));
        if ((u32)lane < run_b) atomicOr(&seam[(b_c & 255u) >> 5], 1u << (b_c & 31u));
        if ((u32)lane < run_a) atomicOr(&seam[8 + ((a_c & 255u) >> 5)], 1u << (a_c & 31u));
        for (u32 off = LEAN_SEAM; run_b == off && off < LEAN_REACH; off += LEAN_SEAM) {
            const u64 i = tile_base - 1 - off - (u64)lane;
            const u32 l = io.lo_in[i], c = io.c_in[i];
            const u32 r = in_run(__ballot(l == lo_first));
            if ((u32)lane < r) atomicOr(&seam[(c & 255u) >> 5], 1u << (c & 31u));
            run_b += r;
        }
        for (u32 off = LEAN_SEAM; run_a == off && off < LEAN_REACH; off += LEAN_SEAM) {
            const u64 i = tile_base + RX_TILE + off + (u64)lane;
            const bool there = i < m;
            const u32 l = there ? io.lo_in[i] : 0u, c = there ? (u32)io.c_in[i] : 0u;
            const u32 r = in_run(__ballot(there && l == lo_last));
            if ((u32)lane < r) atomicOr(&seam[8 + ((c & 255u) >> 5)], 1u << (c & 31u));
            run_a += r;
        }
        const bool undecided = run_b == LEAN_REACH || (run_a == LEAN_REACH && tile_base + RX_TILE + LEAN_REACH < m);
        if (undecided && lane == 0) __hip_atomic_store(io.giveup, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    // every slot: the byte out; equal to a neighbour in the tile's order, or to the lo a seam run has?
#pragma unroll
    for (int j0 = 0; j0 < RX_ITEMS; j0 += HB) {
        u32 cx[HB], x[HB], xp[HB], xn[HB], g[HB];
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const u32 s = (u32)(j0 + jj) * RX_THREADS + tid;
            const u32 sc = s < tile_count ? s : 0u;
            cx[jj] = cx_s[sc];
            x[jj] = lo_s[sc];
            xp[jj] = lo_s[sc ? sc - 1u : 0u];
            xn[jj] = lo_s[sc + 1u < tile_count ? sc + 1u : sc];
        }
#pragma unroll
        for (int jj = 0; jj < HB; jj++) g[jj] = gbase[cx[jj] & 255u];
#pragma unroll
        for (int jj = 0; jj < HB; jj++) {
            const u32 s = (u32)(j0 + jj) * RX_THREADS + tid;
            if (s >= tile_count) continue;
            const u32 dst = g[jj] + s;
            io.sym_out[dst] = (u8)(cx[jj] >> 8);
            const bool eq_p = s > 0 && xp[jj] == x[jj], eq_n = s + 1u < tile_count && xn[jj] == x[jj];
            // (random keys: one slot in a few hundred gets past this line)
            if (!(eq_p || eq_n || x[jj] == lo_first || x[jj] == lo_last)) continue;
            const u32 d = cx[jj] & 255u;
            const bool run_first = s == 0 || (cx_s[s - 1u] & 255u) != d, run_last = s + 1u == tile_count || (cx_s[s + 1u] & 255u) != d;
            const bool same_p = run_first ? x[jj] == lo_first && ((seam[d >> 5] >> (d & 31u)) & 1u) : eq_p;
            const bool same_n = run_last ? x[jj] == lo_last && ((seam[8 + (d >> 5)] >> (d & 31u)) & 1u) : eq_n;
            if (!(same_p || same_n)) continue;
            io.val_out[dst] = io.val_in[tile_base + (cx[jj] >> 16)];
            __hip_atomic_fetch_or(&io.keepw[dst >> 6], 1ull << (dst & 63u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (same_p) __hip_atomic_fetch_and(&io.headw[dst >> 6], ~(1ull << (dst & 63u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#undef PK_VALID
}

// ------------------------------------------------------------------------------------
// host side of a pass
// ------------------------------------------------------------------------------------
static bool knob_off(const bwts_ctx *ctx, const char *name) { const char *e = bwts_knob(ctx, name); return e && atoi(e) == 0; }

// This pass's offsets: the per-tile digit counts of `src` (unless tile_hist holds them already), then their column scan.
template <typename T>
static int radix_pass_offsets(bwts_ctx *ctx, const T *src, u64 m, int shift, u32 *tile_hist, bool counted, void *scan_temp)
{
    const u64 tiles = rx_tiles(m);
    if (!counted) {
        SpanGuard g(ctx, BWTS_K_RADIX_HIST, m, sizeof(T) * m);
        radix_hist_kernel<T><<<dim3((unsigned)tiles), dim3(RX_THREADS), 0, ctx->stream>>>(src, m, shift, tile_hist);
    }
    SpanGuard g(ctx, BWTS_K_RADIX_SCAN, tiles * 256, tiles * 256 * 12);
    STAGE("radix pass: histogram");
    BWTS_TRY(radix_column_scan(ctx, tile_hist, tiles, scan_temp));
    STAGE("radix pass: column scan");
    return BWTS_OK;
}

// One scatter launch of either family; `kernel` is the instantiation its caller picked.  roofline: the launch is timed a second time
// under its own class -- the roofline kernel (one template variant, n-sized launches).  lds: RX_LDS, or RX_LDS_PACKED for the kernels without the slots' byte table.
constexpr size_t RX_LDS = RxTile<RX_THREADS, RX_ITEMS>::bytes, RX_LDS_PACKED = RxTile<RX_THREADS, RX_ITEMS>::bytes_no_sdig;
template <typename... P, typename... A>
static int launch_scatter(bwts_ctx *ctx, void (*kernel)(P...), size_t lds, u64 m, u64 alg_bytes, bool roofline, A... args)
{
    {
        SpanGuard g(ctx, BWTS_K_RADIX_SCATTER, m, alg_bytes);
        const int gm = roofline ? span_begin(ctx, BWTS_K_RADIX_SCATTER_MAIN, m, alg_bytes) : -1;
        const int rc = ensure_dyn_lds(ctx, (const void *)kernel, lds);
        if (rc == BWTS_OK) kernel<<<dim3((unsigned)rx_grid(rx_tiles(m))), dim3(RX_THREADS), lds, ctx->stream>>>(args...);
        span_end(ctx, gm);
        BWTS_TRY(rc);
    }
    HIPC(hipGetLastError());
    STAGE("radix pass: scatter");
    return BWTS_OK;
}

// pass p of `passes` over the packed streams, from keys[cur] / vals[cur] into the other pair.  lean: the last of five passes in its
// lean form (radix_scatter_lean_last_kernel), which writes neither of them
template <bool HI16>
static int radix_packed_pass(bwts_ctx *ctx, const SortPlan &plan, u64 m, int p, int passes, int cur, bool lean)
{
    const size_t lo_bytes = align_up((size_t)m * 4, 256);
    const u64 pass_bytes = HI16 ? 20 : 18;
    const int shift = 8 * p;
    const bool first = p == 0, last = p == passes - 1;
    char *src = (char *)plan.keys[cur], *dst = (char *)plan.keys[cur ^ 1];
    PackedIO io{};
    io.lo_in = (const u32 *)src; io.c_in = src + lo_bytes; io.val_in = plan.vals[cur];
    io.lo_out = (u32 *)dst; io.c_out = dst + lo_bytes; io.val_out = plan.vals[cur ^ 1];
    io.hi_out = (u8 *)dst + lo_bytes; io.sym_out = plan.sym_final;
    // the first pass's table may have been counted already (the key builder's)
    u32 *tile_hist = first && plan.first_hist ? plan.first_hist : plan.tile_hist;
    const bool counted = tile_hist != plan.tile_hist;
    if (HI16 && shift >= 32) BWTS_TRY(radix_pass_offsets(ctx, (const u16 *)io.c_in, m, 0, tile_hist, counted, plan.scan_temp));
    else BWTS_TRY(radix_pass_offsets(ctx, io.lo_in, m, shift, tile_hist, counted, plan.scan_temp));
    if (lean) {
        if (!HI16 || !last || !plan.headw || !plan.keepw || !plan.seam_giveup) return BWTS_E_INTERNAL;
        // c and lo in, the byte out; what the tied slots add is booked with the tied list
        const LeanIO lio{io.lo_in, (const u16 *)io.c_in, io.val_in, io.sym_out, io.val_out, plan.headw, plan.keepw, plan.seam_giveup};
        return launch_scatter(ctx, radix_scatter_lean_last_kernel, RX_LDS_PACKED, m, 7 * m, false, lio, tile_hist, m);
    }
    // the first pass reads no values; the last writes the keys split and the byte alone
    const u64 bytes = first ? pass_bytes - 4 : last ? pass_bytes / 2 + (HI16 ? 10 : 9) : pass_bytes;
    const auto kernel = first ? radix_scatter_packed_kernel<true, false, HI16>
                      : last  ? radix_scatter_packed_kernel<false, true, HI16> : radix_scatter_packed_kernel<false, false, HI16>;
    return launch_scatter(ctx, kernel, RX_LDS_PACKED, m, bytes * m, !first && !last, io, tile_hist, m, shift);
}

// round 0 with the byte stream and identity values, keys of 17..40 bits: split -> packed ... packed -> split
template <bool HI16>
static int radix_sort_packed(bwts_ctx *ctx, const SortPlan &plan, u64 m, int passes, int *result_buf)
{
    if (plan.lean_last && passes != 5) return BWTS_E_INTERNAL;
    int cur = 0;
    for (int p = 0; p < passes; p++) {
        BWTS_TRY(radix_packed_pass<HI16>(ctx, plan, m, p, passes, cur, plan.lean_last && p == passes - 1));
        cur ^= 1;
    }
    *result_buf = cur;
    return BWTS_OK;
}

// After a lean last pass that could not stand: the classic fifth pass, from the fourth pass's output, which the lean pass left as it was
int radix_packed_last_pass(bwts_ctx *ctx, const SortPlan &plan, u64 m)
{
    if (!plan.keys_split || !plan.sym_final) return BWTS_E_INTERNAL;
    return radix_packed_pass<true>(ctx, plan, m, 4, 5, 0, false);
}

// ------------------------------------------------------------------------------------
// small sorts: every pass inside one workgroup
// ------------------------------------------------------------------------------------
// The late rounds of the doubling sort often hold a few hundred stubborn ties; at 7 launches per pass and 7-8 passes per
// sort, launch latency is all they cost.  Up to RS_MAX pairs are sorted here in one launch: the pairs live in LDS
// (ping-pong), a pass ranks with the same ballot matching as the big kernels, a thread owns RS_ITEMS consecutive-by-wave
// elements, and the per-wave digit counts are scanned by the first 256 threads.
#define RS_THREADS 1024
#define RS_WAVES   (RS_THREADS / 64)
#define RS_ITEMS   4
#define RS_MAX     (RS_THREADS * RS_ITEMS)
__global__ __launch_bounds__(RS_THREADS) void radix_sort_small_kernel(const u64 *__restrict__ kin, const u32 *__restrict__ vin,
                                                                      u64 *__restrict__ kout, u32 *__restrict__ vout, u32 m, int passes)
{
    __shared__ u64 sk[2][RS_MAX];
    __shared__ u32 sv[2][RS_MAX];
    __shared__ u16 whist[RS_WAVES][256];
    __shared__ u32 dbase[256];
    __shared__ u32 scan_sm[RS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (u32 i = tid; i < m; i += RS_THREADS) { sk[0][i] = kin[i]; sv[0][i] = vin[i]; }
    int cur = 0;
    for (int p = 0; p < passes; p++) {
        const int shift = 8 * p;
        for (int i = tid; i < RS_WAVES * 128; i += RS_THREADS) ((u32 *)whist)[i] = 0;
        __syncthreads();
        // wave w owns elements [w * 64 * RS_ITEMS, ...), item j of a lane is element base + j * 64 + lane
        const u32 wbase = (u32)w * (64 * RS_ITEMS);
        u64 key[RS_ITEMS];
        u32 val[RS_ITEMS], pos[RS_ITEMS];
#pragma unroll
        for (int j = 0; j < RS_ITEMS; j++) {
            const u32 i = wbase + (u32)j * 64 + lane;
            key[j] = i < m ? sk[cur][i] : ~0ull;
            val[j] = i < m ? sv[cur][i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < RS_ITEMS; j++) {
            const bool valid = wbase + (u32)j * 64 + lane < m;
            const u32 d = (u32)(key[j] >> shift) & 255u;
            wave_rank_step(whist[w], d, valid, [&](u32 r) { pos[j] = r; });
        }
        __syncthreads();
        {
            const u32 exc = digit_bases<RS_WAVES>(whist, scan_sm);
            if (tid < 256) dbase[tid] = exc;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RS_ITEMS; j++) {
            const bool valid = wbase + (u32)j * 64 + lane < m;
            const u32 d = (u32)(key[j] >> shift) & 255u;
            if (valid) {
                const u32 dst = dbase[d] + whist[w][d] + pos[j];
                sk[cur ^ 1][dst] = key[j];
                sv[cur ^ 1][dst] = val[j];
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    for (u32 i = tid; i < m; i += RS_THREADS) { kout[i] = sk[cur][i]; vout[i] = sv[cur][i]; }
}

// ------------------------------------------------------------------------------------
// column scan and the sort drivers
// ------------------------------------------------------------------------------------
// [tile][digit] counts -> global exclusive offsets in digit-major order, in place.
// tile_hist must be followed by the chunk table (radix_tile_hist_bytes()).
// The three steps above in one launch, for tables of at most RX_FUSED_CHUNKS chunks (sorts of up to 2^28 elements): one workgroup
// per chunk, thread = digit.  Every workgroup publishes its chunk's column sums, waits until all have (at most 256 workgroups of
// 256 threads: always resident together, and the only wait in the kernel), then adds up what lies before its chunk -- the chunks
// before it in its own column, all of the smaller digits' columns -- and rewrites its chunk.  sync[0] counts arrivals, sync[1]
// departures; the last workgroup to leave puts both back to zero for the next launch.
// (The sort of a few million pairs spent as long in the five launches it replaces as in the histogram sweep itself.)
#define RX_FUSED_CHUNKS 256
__global__ __launch_bounds__(256) void radix_column_scan_fused_kernel(u32 *__restrict__ tile_hist, u64 tiles, u32 chunks, u32 *__restrict__ chunk_sum,
                                                                      unsigned int *__restrict__ sync)
{
    __shared__ u32 scan_sm[4];
    const u32 c = blockIdx.x, d = threadIdx.x;
    const u64 t0 = (u64)c * RX_CHUNK;
    const u64 t1 = t0 + RX_CHUNK < tiles ? t0 + RX_CHUNK : tiles;
    // (both sweeps over the chunk's tiles keep eight loads in flight: with one at a time a chunk of 128 tiles took 16 us)
    u32 s = 0;
    {
        u64 t = t0;
        for (; t + 8 <= t1; t += 8) {
            u32 v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = tile_hist[(t + j) * 256 + d];
#pragma unroll
            for (int j = 0; j < 8; j++) s += v[j];
        }
        for (; t < t1; t++) s += tile_hist[t * 256 + d];
    }
    u32 before = 0, total = s;
    if (chunks > 1) {            // (one chunk -- up to 2^20 elements: nobody to wait for)
        chunk_sum[(u64)c * 256 + d] = s;
        __threadfence();                         // every thread's sums are out before the workgroup reports in
        __syncthreads();
        if (d == 0) {
            __hip_atomic_fetch_add(&sync[0], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            while (__hip_atomic_load(&sync[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < chunks) __builtin_amdgcn_s_sleep(1);
        }
        __syncthreads();
        __threadfence();                         // acquire for the whole workgroup: the plain loads below see the other workgroups' sums
        total = 0;
        u32 cc = 0;
        for (; cc + 4 <= chunks; cc += 4) {      // independent loads, four in flight
            const u32 v0 = chunk_sum[(u64)cc * 256 + d], v1 = chunk_sum[(u64)(cc + 1) * 256 + d];
            const u32 v2 = chunk_sum[(u64)(cc + 2) * 256 + d], v3 = chunk_sum[(u64)(cc + 3) * 256 + d];
            total += v0 + v1 + v2 + v3;
            before += (cc < c ? v0 : 0u) + (cc + 1 < c ? v1 : 0u) + (cc + 2 < c ? v2 : 0u) + (cc + 3 < c ? v3 : 0u);
        }
        for (; cc < chunks; cc++) { const u32 v = chunk_sum[(u64)cc * 256 + d]; total += v; before += cc < c ? v : 0u; }
    }
    u32 all;
    const u32 base = block_scan_exclusive<u32, OpAdd, 4>(total, OpAdd(), 0u, scan_sm, &all);      // elements with a smaller digit
    u32 run = base + before;
    {
        u64 t = t0;
        for (; t + 8 <= t1; t += 8) {
            u32 v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = tile_hist[(t + j) * 256 + d];
#pragma unroll
            for (int j = 0; j < 8; j++) { tile_hist[(t + j) * 256 + d] = run; run += v[j]; }
        }
        for (; t < t1; t++) { const u32 v = tile_hist[t * 256 + d]; tile_hist[t * 256 + d] = run; run += v; }
    }
    if (chunks > 1) {
        __syncthreads();
        if (d == 0) {
            const u32 left = __hip_atomic_fetch_add(&sync[1], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (left + 1 == chunks) {          // everyone has read the sums and passed the wait
                __hip_atomic_store(&sync[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&sync[1], 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

int radix_column_scan(bwts_ctx *ctx, u32 *tile_hist, u64 tiles, void *scan_temp)
{
    const u64 chunks = radix_chunks(tiles);
    u32 *chunk_sum = (u32 *)((char *)tile_hist + align_up((size_t)tiles * 256 * sizeof(u32), 256));
    const bool fused_ok = !knob_off(ctx, "BWTS_RX_FUSED_SCAN");
    if (ctx->fused_scan_cap == 0) {
        // every workgroup of the fused kernel waits for all the others: it may only be used with as many workgroups as the device
        // is certain to hold at once (a whole MI355X: 256 CUs x 8; a partition of it, or a CU-masked queue, fewer)
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, radix_column_scan_fused_kernel, 256, 0) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
        ctx->fused_scan_cap = per_cu > 0 && cus > 0 ? per_cu * cus : -1;
    }
    if (fused_ok && chunks <= RX_FUSED_CHUNKS && (long long)chunks <= (long long)ctx->fused_scan_cap) {
        radix_column_scan_fused_kernel<<<dim3((unsigned)chunks), dim3(256), 0, ctx->stream>>>(tile_hist, tiles, (u32)chunks, chunk_sum,
                                                                                             (unsigned int *)(ctx->d_small + SM_RX_SYNC));
        HIPC(hipGetLastError());
        return BWTS_OK;
    }
    radix_chunk_sum_kernel<<<dim3((unsigned)chunks), dim3(256), 0, ctx->stream>>>(tile_hist, tiles, chunks, chunk_sum);
    BWTS_TRY(exclusive_sum_u32(ctx, chunk_sum, chunks * 256, scan_temp));
    radix_chunk_apply_kernel<<<dim3((unsigned)chunks), dim3(256), 0, ctx->stream>>>(tile_hist, tiles, chunks, chunk_sum);
    HIPC(hipGetLastError());
    return BWTS_OK;
}

// Stable sort of bare u64 keys on bits [lo_bit, lo_bit + bits): 16 bytes per element and pass.
// Returns in *result_buf which of keys[] holds the output.
int radix_sort_keys(bwts_ctx *ctx, u64 *keys[2], u32 *tile_hist, void *scan_temp, u64 m, int lo_bit, int bits, int *result_buf)
{
    int cur = 0;
    for (int shift = lo_bit; shift < lo_bit + bits; shift += 8) {
        BWTS_TRY(radix_pass_offsets(ctx, keys[cur], m, shift, tile_hist, false, scan_temp));
        BWTS_TRY(launch_scatter(ctx, radix_scatter2_kernel<RX_THREADS, RX_ITEMS, RX_MINW, false, false, true>, RX_LDS, m, 16 * m, false,
                                keys[cur], nullptr, keys[cur ^ 1], nullptr, tile_hist, m, shift,
                                nullptr, nullptr));
        cur ^= 1;
    }
    *result_buf = cur;
    return BWTS_OK;
}

bool radix_packed_applicable(const bwts_ctx *ctx, u64 m, int key_bits)
{
    const int passes = ((key_bits < 1 ? 1 : key_bits) + 7) / 8;
    return !knob_off(ctx, "BWTS_RX_PACK") && passes >= 3 && passes <= 5 && m >= 65536;
}

int radix_sort_pairs(bwts_ctx *ctx, const SortPlan &plan, u64 m, int key_bits, int *result_buf)
{
    int cur = 0;
    if (m == 0) { *result_buf = 0; return BWTS_OK; }
    if (key_bits < 1) key_bits = 1;
    if (key_bits > 64) key_bits = 64;
    const int passes = (key_bits + 7) / 8;
    if (plan.lean_last && !plan.keys_split) return BWTS_E_INTERNAL;

    if (!knob_off(ctx, "BWTS_RX_SMALL") && m <= RS_MAX && !plan.sym_src && !plan.vals_identity && !plan.keys_split) {
        SpanGuard g(ctx, BWTS_K_RADIX_SCATTER, m, 24 * m);
        radix_sort_small_kernel<<<dim3(1), dim3(RS_THREADS), 0, ctx->stream>>>(plan.keys[0], plan.vals[0], plan.keys[1], plan.vals[1], (u32)m, passes);
        HIPC(hipGetLastError());
        *result_buf = 1;
        return BWTS_OK;
    }
    if (plan.keys_split) {      // round 0 of the forward transform: keybuild left the keys split for the packed passes
        if (!plan.sym_final || !plan.vals_identity || !radix_packed_applicable(ctx, m, key_bits)) return BWTS_E_INTERNAL;
        if (passes == 5) return radix_sort_packed<true>(ctx, plan, m, passes, result_buf);
        return radix_sort_packed<false>(ctx, plan, m, passes, result_buf);
    }

    for (int p = 0; p < passes; p++) {
        const int shift = 8 * p;
        BWTS_TRY(radix_pass_offsets(ctx, plan.keys[cur], m, shift, plan.tile_hist, false, plan.scan_temp));
        // the first pass of a sort over positions reads no values (value = index); the byte stream, if any, rides along
        const bool ident = plan.vals_identity && p == 0, has_sym = plan.sym_src != nullptr;
        const u8 *sin = !has_sym ? nullptr : p == 0 ? plan.sym_src : plan.sym_buf[(p - 1) & 1];
        u8 *sout = !has_sym ? nullptr : p == passes - 1 ? plan.sym_final : plan.sym_buf[p & 1];
        const auto kernel = has_sym ? (ident ? radix_scatter2_kernel<RX_THREADS, RX_ITEMS, RX_MINW, true, true>
                                             : radix_scatter2_kernel<RX_THREADS, RX_ITEMS, RX_MINW, true, false>)
                                    : (ident ? radix_scatter2_kernel<RX_THREADS, RX_ITEMS, RX_MINW, false, true>
                                             : radix_scatter2_kernel<RX_THREADS, RX_ITEMS, RX_MINW, false, false>);
        BWTS_TRY(launch_scatter(ctx, kernel, RX_LDS, m, ((has_sym ? 26 : 24) - (ident ? 4 : 0)) * m, has_sym && !ident,
                                plan.keys[cur], plan.vals[cur], plan.keys[cur ^ 1], plan.vals[cur ^ 1],
                                plan.tile_hist, m, shift, sin, sout));
        cur ^= 1;
    }
    *result_buf = cur;
    return BWTS_OK;
}

// ------------------------------------------------------------------------------------
// test hook: the ranking of one tile alone (bwts_debug_rank_steps)
// ------------------------------------------------------------------------------------
// One workgroup ranks RX_TILE caller-given digits, item j of lane l of wave w at [w][j][l], with rank_split<K> on counters of its
// own, and writes every valid item's rank among its wave's earlier elements with its digit (~0 for an invalid item).
template <int K>
__global__ __launch_bounds__(RX_THREADS) void rank_steps_kernel(const u8 *__restrict__ digits, const u8 *__restrict__ valid, u32 *__restrict__ ranks)
{
    __shared__ u32 cnt[RX_WAVES][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < RX_WAVES * 256; i += RX_THREADS) ((u32 *)cnt)[i] = 0;
    u32 d[RX_ITEMS], vmask = 0;
#pragma unroll
    for (int j = 0; j < RX_ITEMS; j++) {
        const u32 i = ((u32)w * RX_ITEMS + (u32)j) * 64u + (u32)lane;
        d[j] = digits[i];
        vmask |= (valid[i] ? 1u : 0u) << j;
    }
    __syncthreads();
    Pos16<RX_ITEMS> pos;
    rank_split<K>(cnt[w], pos, [&](int j) { return d[j]; }, [&](int j) { return (bool)((vmask >> j) & 1u); });
#pragma unroll
    for (int j = 0; j < RX_ITEMS; j++)
        ranks[((u32)w * RX_ITEMS + (u32)j) * 64u + (u32)lane] = (vmask >> j) & 1u ? pos.get(j) : ~0u;
}

int radix_debug_rank_steps(bwts_ctx *ctx, const u8 *d_digits, const u8 *d_valid, int atomic_items, u32 *d_ranks, u32 shipped[4])
{
    shipped[0] = RX_ATOMIC_FIRST; shipped[1] = RX_ATOMIC_MIDDLE; shipped[2] = RX_ATOMIC_LAST; shipped[3] = RX_ATOMIC_LEAN;
    void (*kernel)(const u8 *, const u8 *, u32 *) = nullptr;
    switch (atomic_items) {
    case 0: kernel = rank_steps_kernel<0>; break;
    case 2: kernel = rank_steps_kernel<2>; break;
    case 4: kernel = rank_steps_kernel<4>; break;
    case 6: kernel = rank_steps_kernel<6>; break;
    case 8: kernel = rank_steps_kernel<8>; break;
    case 10: kernel = rank_steps_kernel<10>; break;
    case 12: kernel = rank_steps_kernel<12>; break;
    case 14: kernel = rank_steps_kernel<14>; break;
    case 16: kernel = rank_steps_kernel<16>; break;
    default: return BWTS_E_ARG;
    }
    kernel<<<dim3(1), dim3(RX_THREADS), 0, ctx->stream>>>(d_digits, d_valid, d_ranks);
    HIPC(hipGetLastError());
    return BWTS_OK;
}
