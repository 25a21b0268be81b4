// device_utils.h -- wave64 / workgroup building blocks for gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint16_t u16;
typedef uint8_t  u8;

#define WAVE 64

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }
__device__ __forceinline__ int wave_id() { return (int)(threadIdx.x >> 6); }

__device__ __forceinline__ u64 lanemask_lt()
{
    return (1ull << lane_id()) - 1ull;
}

struct OpAdd { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct OpMax { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct OpMin { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? a : b; } };
struct OpXor { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a ^ b; } };

__device__ __forceinline__ u32 shfl_up_t(u32 v, int d) { return (u32)__shfl_up((int)v, d, 64); }
__device__ __forceinline__ u64 shfl_up_t(u64 v, int d)
{
    u32 lo = (u32)__shfl_up((int)(u32)v, d, 64);
    u32 hi = (u32)__shfl_up((int)(u32)(v >> 32), d, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_down_t(u64 v, int d)
{
    u32 lo = (u32)__shfl_down((int)(u32)v, d, 64);
    u32 hi = (u32)__shfl_down((int)(u32)(v >> 32), d, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u32 shfl_t(u32 v, int src) { return (u32)__shfl((int)v, src, 64); }
__device__ __forceinline__ u64 shfl_t(u64 v, int src)
{
    u32 lo = (u32)__shfl((int)(u32)v, src, 64);
    u32 hi = (u32)__shfl((int)(u32)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}

// inclusive scan across the 64 lanes of a wave (commutative op)
template <typename T, typename Op>
__device__ __forceinline__ T wave_scan_inclusive(T v, Op op)
{
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        T o = shfl_up_t(v, d);
        if (lane >= d) v = op(o, v);
    }
    return v;
}

// op over the 64 lanes of a wave, the result in every lane (commutative op)
template <typename Op>
__device__ __forceinline__ u32 wave_reduce(u32 v, Op op)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v = op((u32)__shfl_xor((int)v, d, 64), v);
    return v;
}

// The per-unit table of a segmented stage call (stage_cut.h: a unit is a tile or a block): one wave per segment, the lanes over
// the segment's units.  f.first(s): the segment's first unit, counted over the call; f.units(s): how many it has; f.store(s, first,
// units, j): writes what the stage keeps for the segment's unit j.
template <typename F>
__global__ __launch_bounds__(256) void unit_table_kernel(u64 count, F f)
{
    const u64 lane = (u64)lane_id();
    for (u64 s = (u64)blockIdx.x * 4 + (u64)wave_id(); s < count; s += (u64)gridDim.x * 4) {
        const u64 first = f.first(s), units = f.units(s);
        for (u64 j = lane; j < units; j += 64) f.store(s, first, units, j);
    }
}

// Workgroups of four waves for kernels that stride over their work by the grid, one wave an item: at most 2048, eight a CU.  (Of the
// three caps the table launches had -- 2^30, 2^20 and this one -- the tightest: a strided kernel covers every count under any cap.)
static inline unsigned wave_grid(u64 waves)
{
    const u64 wgs = (waves + 3) / 4;
    return (unsigned)(wgs < 2048 ? wgs : 2048);
}

template <typename F>
static inline void unit_table_launch(hipStream_t stream, u64 count, F f)
{
    unit_table_kernel<<<dim3(wave_grid(count)), dim3(256), 0, stream>>>(count, f);
}

// Workgroup-wide scan of one value per thread.  NWAVES = blockDim.x / 64.
// Returns the exclusive prefix of the calling thread; *total gets the block total.
// smem must hold NWAVES values; contains two barriers.
template <typename T, typename Op, int NWAVES>
__device__ __forceinline__ T block_scan_exclusive(T v, Op op, T identity, T *smem, T *total)
{
    const int lane = lane_id(), w = wave_id();
    T inc = wave_scan_inclusive(v, op);
    if (lane == 63) smem[w] = inc;
    __syncthreads();
    T wave_prefix = identity, tot = identity;
#pragma unroll
    for (int i = 0; i < NWAVES; i++) {
        T s = smem[i];
        if (i < w) wave_prefix = op(wave_prefix, s);
        tot = op(tot, s);
    }
    __syncthreads();
    T exc = shfl_up_t(inc, 1);
    if (lane == 0) exc = identity;
    *total = tot;
    return op(wave_prefix, exc);
}

// lanes of the wave whose 8-bit digit equals the caller's (restricted to `valid` lanes).
// The radix kernels are VALU-bound, and in the kernels that rank every item with wave_rank_step (the wide passes, the small sort, the
// LF kernels) most of their VALU work is this function -- 52 of a middle pass's 84 VALU instructions per item; the packed round-0
// passes give some of a tile's items to the LDS atomic unit instead (wave_rank_atomic_step).  It is written for instruction
// count: per digit bit, t = 0 / -1 from a sign-extended one-bit field, one compare for the ballot, and on each
// 32-bit half an XNOR with the ballot (lanes whose bit equals mine) folded in with an AND -- six instructions.
__device__ __forceinline__ u64 match_digit8(u32 digit, bool valid)
{
    const u64 vm = __ballot(valid);
    u32 plo = (u32)vm, phi = (u32)(vm >> 32);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const u32 t = (u32)__builtin_amdgcn_sbfe((int)digit, (unsigned)b, 1u);      // 0 or ~0
        const u64 m = __ballot((int)t < 0);                                              // sign test of t itself: no second extract
        plo &= ~((u32)m ^ t);
        phi &= ~((u32)(m >> 32) ^ t);
    }
    return ((u64)phi << 32) | plo;
}

// One item's step of the stable ranking every radix and LF kernel uses: the lanes of a wave that hold digit d take consecutive
// ranks, in lane order, from the wave's counter wave_hist[d] (u16 or u32), and the first lane of the run moves the counter past
// them.  rank(r) receives the item's rank among the wave's elements with its digit BEFORE the first fence, so the caller's
// store of it is not ordered behind the counter update.  The two wavefront fences are what makes the next item's read of the
// counter see this item's update: the lanes run in lockstep, but without them the compiler may move the LDS read of item j+1
// above the write of item j.  No atomics, no barrier.
template <typename C, typename Rank>
__device__ __forceinline__ void wave_rank_step(C *wave_hist, u32 d, bool valid, Rank rank)
{
    const u64 peers = match_digit8(d, valid);
    const u32 before = (u32)__popcll(peers & lanemask_lt());
    const u32 cnt = (u32)__popcll(peers);
    const u32 prev = wave_hist[d];
    rank(prev + before);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (valid && before == 0) wave_hist[d] = (C)(prev + cnt);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// The same step on the other unit: one returning LDS add of 1 on the wave's u32 counter of the digit, no ballots -- 4 VALU
// instructions an item where wave_rank_step takes 52, and the LDS atomic unit works while the VALU ranks other items.  Lanes with
// one digit are served one by one, so a wave full of equal digits (sorted, repetitive keys) is where the ballot step is the
// faster of the two.  Invalid lanes issue nothing.
// Why the ranks are the ones wave_rank_step gives, so that a tile may rank any of its items with either step on the same
// counters: (1) inside one instruction the lanes that add to the same address are served in lane order (a property of this
// chip's LDS, pinned by tests/test_rank_atomic_gpu.py), so a lane gets the counter's value plus the number of lower lanes with its
// digit -- prev + before; (2) a wave's LDS instructions execute in program order, so the counter holds the number of the wave's
// elements with digit d in items 0 .. j-1 when item j's instruction -- atomic, or the read of a ballot step -- reaches it, and a
// ballot step's plain write of prev + cnt is the value 64 atomic lanes would have left.  Both kinds of rank are therefore "the
// wave's earlier elements with my digit, in element order", the ranking is stable, and the counter ends as the digit's count.
// rank(r) is handed the returned register and nothing here reads it: a caller that only keeps it (no arithmetic on it inside
// rank) lets the compiler issue the atomics of several items back to back and wait once, where they are first used.
template <typename Rank>
__device__ __forceinline__ void wave_rank_atomic_step(u32 *wave_cnt, u32 d, bool valid, Rank rank)
{
    if (valid) rank(__hip_atomic_fetch_add(&wave_cnt[d], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}

// After the ranking: thread d < 256 turns column d of the waves' counters into each wave's start inside the digit (exclusive, in
// wave order), and the column totals are scanned over the workgroup.  Returns the calling thread's exclusive base: for d < 256 the
// number of the tile's elements with a smaller digit.  Contains block_scan_exclusive's two barriers; the caller stores the base
// where it needs it and synchronises before anyone reads it.
template <int NWAVES, typename C>
__device__ __forceinline__ u32 digit_bases(C (*whist)[256], u32 *scan_sm)
{
    const int tid = threadIdx.x;
    u32 run = 0;
    if (tid < 256) {
#pragma unroll
        for (int ww = 0; ww < NWAVES; ww++) {
            const u32 c = whist[ww][tid];
            whist[ww][tid] = (C)run;
            run += c;
        }
    }
    u32 total;
    return block_scan_exclusive<u32, OpAdd, NWAVES>(run, OpAdd(), 0u, scan_sm, &total);
}

// The same, with the digit's base folded into the waves' starts: whist[ww][d] comes out as the first slot, in the tile, of wave ww's
// elements with digit d, so a kernel that stages an item reads one word for it, not base and start.  The starts wait in registers
// for the scan (the column is read once and written once, as above; the sums are those of the plain form, C holds them when it
// holds a tile position).  The counts are read from cnt, which may be another array than whist (the u32 counters the atomic step
// needs, in memory that is reused once the starts are out): every read of cnt lies before the scan's barriers, every write of
// whist behind them, and all of whist is written.
template <int NWAVES, typename C>
__device__ __forceinline__ u32 digit_bases_folded(const u32 (*cnt)[256], C (*whist)[256], u32 *scan_sm)
{
    const int tid = threadIdx.x;
    u32 start[NWAVES], run = 0;
    if (tid < 256) {
#pragma unroll
        for (int ww = 0; ww < NWAVES; ww++) start[ww] = cnt[ww][tid];
#pragma unroll
        for (int ww = 0; ww < NWAVES; ww++) {
            const u32 c = start[ww];
            start[ww] = run;
            run += c;
        }
    }
    u32 total;
    const u32 exc = block_scan_exclusive<u32, OpAdd, NWAVES>(run, OpAdd(), 0u, scan_sm, &total);
    if (tid < 256) {
#pragma unroll
        for (int ww = 0; ww < NWAVES; ww++) whist[ww][tid] = (C)(start[ww] + exc);
    }
    return exc;
}

// One wave's 64 consecutive digits into its LDS bins.  Sorted and repetitive input (every pass but the first of a sort over text or
// over ranks with many equal values) puts runs of equal digits into neighbouring lanes, and same-address LDS atomics are served one
// lane at a time: a pass over such keys ran at 2.4 TB/s where unsorted keys reach 5.6.  So the lanes of a run elect their first one, and
// it adds the run's length (valid lanes are a prefix of the wave).  The neighbour's digit comes through DPP (row_shr:1 -- no trip
// through the LDS crossbar, which cost the 2-byte sweep over random digits 0.15 ms of 0.45); a row's first lane has no neighbour
// there and starts a run of its own: runs are at most 16 long.
__device__ __forceinline__ void hist_add_runs(u32 *wave_bins, u32 d, bool valid)
{
    const int lane = lane_id();
    const u32 dprev = (u32)__builtin_amdgcn_update_dpp((int)d, (int)d, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
    const bool head = valid && ((lane & 15) == 0 || d != dprev);
    const u64 hm = __ballot(head), vm = __ballot(valid);
    if (hm == vm) {                              // (no two neighbours alike -- three waves in four on random digits: nothing to add up)
        if (valid) atomicAdd(&wave_bins[d], 1u);
    } else if (head) {
        const u64 above = lane == 63 ? 0ull : hm >> (lane + 1);
        const u32 next = above ? (u32)lane + (u32)__ffsll((unsigned long long)above) : (u32)__popcll(vm);
        atomicAdd(&wave_bins[d], next - (u32)lane);
    }
}
