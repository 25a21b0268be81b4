// inverse.hip -- BWTS inverse transform on the GPU.
//
// Replaces the inline core of /root/reference/unbwts.c:31-86:
//   :34-43  histogram + exclusive scan -> row 0 of the scanned [tile][symbol] table (ctab_from_tiles_kernel)
//   :50-52  prev[i]=counts[B[i]]++ (stable LF map) -> lf_hist_kernel + column scan (radix.hip) + lf_rank_kernel
//   :66-86  cycle walk, smallest unvisited index first, text written backwards
//           -> splitter walk recording every segment's symbols, reduced-list ranking by pointer jumping,
//              placement of the recorded segments
// The reference follows ONE cycle at a time (n dependent loads).  Here every G-th index is a splitter; a lane walks
// from its splitter to the next one, so ~n/G walks run concurrently, and LF is chased exactly once.  Cycles that contain
// no splitter are found from per-class moments of the indices the walk visited (or, in the alternative modes, from the walk's
// index log or from visited marks) and resolved separately.
#include "internal.h"
#include "device_utils.h"
#include "scan_templ.h"

#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#define LF_THREADS 256
#define LF_WAVES   4
#define LF_ITEMS   16
#define LF_TILE    (LF_THREADS * LF_ITEMS)
#define LF_VISITED 0xffffffffu     // written over an entry once the walk has read it (LF is chased exactly once)

#define SMI_COUNTERS 320
// The used words of the inverse's counter block, d_small[SMI_COUNTERS ..] (IC_WORDS words, cleared before every walk; both forms)
enum InvCounter {
    IC_TICKET = 0, IC_VIRTUAL = 3, IC_LOG_CHUNKS = 5,           // the walk: next batch of splitter ids, virtual nodes (segments cut at `slot` symbols), log chunks handed out
    IC_OVERFLOW = 4,                                            // the walk: node pool exhausted; the one-lane scan: a cycle too long for one lane
    IC_UNREACHED = 1, IC_UNREACHED_NODES = 6,                   // elements no walk visited; nodes no level-2 walk reached
    IC_LIST_CYCLES = 2, IC_FREE_CYCLES = 7, IC_UNIT_CYCLES = 9, // cycles of the reduced list; without a splitter by the one-lane scan, or by the unit-node ranking
    IC_LISTED_CLASSES = 10, IC_MOM_FALLBACK = 11,               // moments: classes handed to the element-by-element search; the moments do not name the unreached elements
    IC_LENGTH_SUM = 13, IC_WORDS = 16                           // sum of all cycle lengths: n when every element has its place
};
static inline unsigned long long *inv_counter(bwts_ctx *ctx, int c) { return (unsigned long long *)(ctx->d_small + SMI_COUNTERS + c); }
static inline u64 inv_count(const bwts_ctx *ctx, int c) { return ctx->h_small[SMI_COUNTERS + c]; }

// ------------------------------------------------------------------------------------
// stable LF map
// ------------------------------------------------------------------------------------
// per-tile symbol counts.  The order inside the tile does not matter here: a thread takes 16 consecutive bytes (one
// 16-byte load when the tile is aligned) and counts into one of 16 lane-interleaved copies of the bins (skewed text would
// otherwise serialise a wave on its most frequent symbols).
#define LFH_COPIES 16
__global__ __launch_bounds__(LF_THREADS) void lf_hist_kernel(const u8 *__restrict__ B, u64 n, u32 *__restrict__ tile_hist)
{
    __shared__ u32 bins[LFH_COPIES][256];
    const int tid = threadIdx.x;
    u32 *mine = bins[tid & (LFH_COPIES - 1)];
    for (int i = tid; i < LFH_COPIES * 256; i += LF_THREADS) ((u32 *)bins)[i] = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * LF_TILE;
    const u64 i0 = base + (u64)tid * LF_ITEMS;
    static_assert(LF_ITEMS == 16, "one 16-byte load per thread");
    if (i0 + LF_ITEMS <= n && (((uintptr_t)B + i0) & 15) == 0) {
        const uint4 q = *(const uint4 *)(B + i0);
        const u32 ws[4] = {q.x, q.y, q.z, q.w};
        // (a transform of text is made of runs: a thread adds each run of its 16 bytes once: the inverse of 1 GiB of real text 33.3 -> 32.0 ms)
        u32 cur = ws[0] & 255u, cnt = 0;
#pragma unroll
        for (int a = 0; a < 4; a++) {
#pragma unroll
            for (int bb = 0; bb < 4; bb++) {
                const u32 b = (ws[a] >> (8 * bb)) & 255u;
                if (b == cur) cnt++;
                else { atomicAdd(&mine[cur], cnt); cur = b; cnt = 1; }
            }
        }
        atomicAdd(&mine[cur], cnt);
    } else {
        for (int j = 0; j < LF_ITEMS; j++) if (i0 + j < n) atomicAdd(&mine[B[i0 + j]], 1u);
    }
    __syncthreads();
    u32 s = 0;
#pragma unroll
    for (int c = 0; c < LFH_COPIES; c++) s += bins[c][tid];
    tile_hist[(u64)blockIdx.x * 256 + tid] = s;
}

__global__ __launch_bounds__(LF_THREADS) void lf_rank_kernel(const u8 *__restrict__ B, u64 n, const u32 *__restrict__ tile_off,
                                                             u32 *__restrict__ LF)
{
    __shared__ u32 whist[LF_WAVES][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const u64 wave_base = (u64)blockIdx.x * LF_TILE + (u64)w * (64 * LF_ITEMS);
    for (int i = tid; i < LF_WAVES * 256; i += LF_THREADS) ((u32 *)whist)[i] = 0;
    u32 sym[LF_ITEMS], rnk[LF_ITEMS];
#pragma unroll
    for (int j = 0; j < LF_ITEMS; j++) {
        const u64 i = wave_base + (u64)j * 64 + lane;
        sym[j] = i < n ? (u32)B[i] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LF_ITEMS; j++) {
        const bool valid = wave_base + (u64)j * 64 + lane < n;
        wave_rank_step(whist[w], sym[j], valid, [&](u32 r) { rnk[j] = r; });
    }
    __syncthreads();
    {
        u32 run = tile_off[(u64)blockIdx.x * 256 + tid];
#pragma unroll
        for (int ww = 0; ww < LF_WAVES; ww++) {
            const u32 c = whist[ww][tid];
            whist[ww][tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LF_ITEMS; j++) {
        const u64 i = wave_base + (u64)j * 64 + lane;
        if (i < n) LF[i] = whist[w][sym[j]] + rnk[j];
    }
}

// C[c] = first slot of symbol c = tile 0's offset in the scanned [tile][symbol] table; C[256] = n.  The table is 32-bit:
// a boundary equal to 2^32 (n = 2^32, symbols above the largest one present) reads as a value below its predecessor --
// unless the predecessor is 0 too, i.e. one symbol holds all 2^32 positions: then every entry reads 0 and B[0] says which
// symbol that is.
__global__ void ctab_from_tiles_kernel(const u32 *__restrict__ tile_off, u64 n, const u8 *__restrict__ B, u64 *__restrict__ C)
{
    if (threadIdx.x != 0) return;
    u64 prev = 0;
    bool all_zero = true;
    for (int c = 0; c < 256; c++) {
        u64 v = tile_off[c];
        all_zero = all_zero && v == 0;
        if (v < prev) v += 0x100000000ull;
        C[c] = v;
        prev = v;
    }
    if (all_zero && n == 0x100000000ull) {
        const int b = B[0];
        for (int c = b + 1; c < 256; c++) C[c] = n;
    }
    C[256] = n;
}

// ------------------------------------------------------------------------------------
// splitter walk (the only pass that chases LF)
// ------------------------------------------------------------------------------------
__device__ __forceinline__ u32 symbol_of(const u64 *Ctab, u32 y)
{
    // B[x] is the symbol whose C-range holds LF[x]: largest c with Ctab[c] <= y  (Ctab[256] = n)
    u32 lo = 0, hi = 255;
#pragma unroll
    for (int it = 0; it < 8; it++) {
        const u32 mid = (lo + hi + 1) >> 1;
        if (Ctab[mid] <= (u64)y) lo = mid; else hi = mid - 1;     // 64-bit: boundaries reach n = 2^32
    }
    return lo;
}

// A lane walks LF from its splitter to the next one.  Along the way it leaves evidence of the entries it visits
// (MARK below), keeps the smallest index seen, and records the symbols it passes -- B[x] read off LF[x] -- into
// its node's slot of `seg`, 4 at a time.  A walk that reaches `slot` steps without meeting a splitter closes its
// node there and continues as a fresh virtual node (ids >= s, handed out by an atomic counter), so no segment
// outgrows its slot.  A wave pulls batches of splitter ids from a shared counter and hands them to its lanes as
// they finish (one atomic per WALK_BATCH walks); every walk ends at the next splitter (LF is a permutation) and
// a lane that finds the counter exhausted stops asking, so every wave drains.
#ifndef WALK_BATCH
#define WALK_BATCH 128
#endif
// MARK: how the walk leaves evidence of the entries it visited, so that cycles without a splitter can be found:
//   0  index log   -- every step the wave appends the indices its active lanes stand on to its own log chunk, back to
//                     back (one contiguous store per wave and step; the log is a set, it does not say which node an
//                     index belongs to).  The unvisited complement comes from bucket_indices_kernel +
//                     unvisited_from_buckets_kernel.  The walk then costs one random line fill per step and nothing
//                     else that is random: measured 58 -> 35 ms at n = 2^30 against sentinel marks.
//   1  sentinel    -- the entry is overwritten with LF_VISITED (one extra random 32-byte write per step)
//   2  byte map    -- marks[x] = 1 (when LF_VISITED could be a real entry: n = 2^32)
// WALK_PROFILE (compile-time; no build defines it and no host code primes or prints the stamps any more) put wall-clock times of first start / pool exhausted / wave ends into ticket[8..12]:
// at n = 2^30 the pool runs dry at ~29 ms whatever the walker count (64 K .. 512 K lanes) and batch size, and the
// longest residual chain (~G ln(walkers) dependent steps) adds ~5 ms; only a smaller G shortens that tail.
#define IDX_RANGE_LOG2 20
#define IDX_MAX_BUCKETS 4096
#define IDX_THREADS 512
#define IDX_PER_THREAD 32
#define IDX_CHUNK (IDX_THREADS * IDX_PER_THREAD)      // entries of one log chunk (= one tile of bucket_indices_kernel)
#define IDX_FILL_STRIDE 32            // u32 words between two bucket counters (128 bytes)
#define MARK_LOG 0
#define MARK_SENTINEL 1
#define MARK_BYTEMAP 2
#define MARK_MOMENTS 3
//   3  moments     -- nothing is written per step: the workgroup keeps, per residue class of the index mod 2^10 (2^12 above n = 2^30), how many
//                     indices it visited, the sum of their quotients and the sum of the squares (three LDS atomics).  A class that
//                     misses one or two indices names them by arithmetic; a class that misses more is searched element by element
//                     (moments_chase_kernel: an element is unreached iff its own chase returns to it before it meets a splitter).
//                     (Classes by the high bits -- ranges -- were the first form: the few dozen unreached elements of a text are the
//                     rotations of its last, small Lyndon factors and sit in a handful of ranges, a dozen to each.)
//                     The micro-benchmark puts the log at 7 % of the walk, and its scan at 1.4 ms (tools/micro/walk_steps.hip).
#define MOM_LOG2_SMALL 10                    // classes: 2^10 up to n = 2^30 (20 KB of LDS), 2^12 above (80 KB: a class stays at 2^20 elements)
#define MOM_LOG2_LARGE 12
#define MOM_MAX_BUCKETS (1u << MOM_LOG2_LARGE)
// SYM: where the symbol of x comes from.  SYM_FROM_C: B[x] is the symbol whose C-range holds LF[x] (one BWT, one C table: nothing but LF is
// read).  SYM_FROM_INPUT: B[x] itself, loaded beside LF[x] -- the shared pass over independent segments, whose LF is built per segment
// with one C table each (inv_build_lf), so no single table names the symbol.
#define SYM_FROM_C 0
#define SYM_FROM_INPUT 1
template <int MARK, int SBW /* registers of recorded symbols per store: 16 = 64-byte blocks, 4 = 16-byte ones */, int SYM>
__device__ __forceinline__ void walk_record_body(u32 *LF, u8 *marks, u32 *idxlog, u64 s, u64 node_cap, int g, u32 slot,
                                                 const u64 *Cg, const u8 *Bsym, u8 *seg,
                                                 uint4 *noderec /* x next node, y segment length, z smallest element, w its offset */,
                                                 unsigned long long *ticket,
                                                 unsigned long long *vcount,
                                                 unsigned long long *overflow,
                                                 unsigned long long *chunk_ctr, u32 *chunk_fill, u64 log_chunks,
                                                 u32 nbuckets, u32 *bucket_seen,
                                                 int mom_shift, unsigned long long *mom /* [3][2^mom_shift]: counts, sums, sums of squares */)
{
    __shared__ u64 Ctab[SYM == SYM_FROM_C ? 257 : 1];
    extern __shared__ __attribute__((aligned(16))) unsigned long long walk_mom_sm[];     // MARK_MOMENTS: 2^mom_shift sums, sums of squares, counts
    const u32 mom_classes = MARK == MARK_MOMENTS ? 1u << mom_shift : 0u;
    unsigned long long *msum = walk_mom_sm, *msq = walk_mom_sm + mom_classes;
    u32 *mcnt = (u32 *)(walk_mom_sm + 2 * mom_classes);
    if (MARK == MARK_MOMENTS) for (u32 b = threadIdx.x; b < mom_classes; b += 256) { mcnt[b] = 0; msum[b] = 0; msq[b] = 0; }
    // (Round 3 tried two things here and measured both worse: fetching the next LF entry before the current step's symbol search and
    // moments -- the walk is bound by the memory system's line-fill rate, not by a lane's dependency chain, and the second read in
    // flight per lane only lengthens the queues: dna 2^32 119.7 -> 129.5 ms, zipf 2^30 27.4 -> 27.8 ms -- and count + sum in one
    // 64-bit LDS atomic, which changed nothing measurable.  profiles/history/NOTES.md.)
    // MARK_LOG: how many indices of each 2^IDX_RANGE_LOG2-range this workgroup visited.  A range that ends up with all of
    // its indices counted holds nothing unvisited, and its log entries need not be looked at again.
    __shared__ u32 bseen[MARK == MARK_LOG ? IDX_MAX_BUCKETS : 1];
    if (MARK == MARK_LOG) for (u32 b = threadIdx.x; b < nbuckets; b += 256) bseen[b] = 0;
    if (SYM == SYM_FROM_C) for (int i = threadIdx.x; i < 257; i += 256) Ctab[i] = Cg[i];
    __syncthreads();
    const u32 gmask = (1u << g) - 1u;
    bool have = false, done = false;
    u64 my = 0;
    u32 x = 0, len = 0, mn = 0, mnoff = 0;
    // 64 recorded symbols wait in 16 registers for one 64-byte store into the node's slot (four 16-byte words at once): with 16 symbols
    // per store the walk ran at 36 G steps/s, with 64 at 40 (tools/micro/walk_steps.hip: the scattered 16-byte stores cost 19 % of a bare chase,
    // the 64-byte ones 3 %)
    u32 sb[SBW];
    constexpr u32 SBM = 4 * SBW - 1;           // symbols per block - 1
#pragma unroll
    for (int q = 0; q < SBW; q++) sb[q] = 0;
    u64 bnext = 0, bend = 0;            // the wave's current batch of splitter ids (wave-uniform)
    bool exhausted = false;
#ifdef WALK_PROFILE
    unsigned long long *prof = ticket + 8;
    if (lane_id() == 0) atomicMin(&prof[0], (unsigned long long)wall_clock64());
    bool stamped = false;
#endif
    u64 lcur = 0, lbase = 0, lend = 0;  // MARK_LOG: the wave's open log chunk [lbase, lend) and its fill cursor (wave-uniform)
    for (;;) {
        const u64 need = __ballot(!have && !done);
        if (need) {
            if (bnext == bend && !exhausted) {
                const int leader = __ffsll((unsigned long long)need) - 1;
                unsigned long long basev = 0;
                if (lane_id() == leader) basev = atomicAdd(ticket, (unsigned long long)WALK_BATCH);
                basev = shfl_t((u64)basev, leader);
                bnext = basev;
                bend = basev + WALK_BATCH < s ? basev + WALK_BATCH : s;
                if (basev >= s) { exhausted = true; bnext = bend = 0; }
#ifdef WALK_PROFILE
                if (exhausted && !stamped) { stamped = true; if (lane_id() == leader) { atomicMin(&prof[1], (unsigned long long)wall_clock64()); atomicMax(&prof[3], (unsigned long long)wall_clock64()); } }
#endif
            }
            if (!have && !done) {
                const u64 id = bnext + (u64)__popcll(need & lanemask_lt());
                if (id < bend) {
                    have = true; my = id; x = (u32)(my << g); len = 0; mn = x; mnoff = 0;
#pragma unroll
                    for (int q = 0; q < SBW; q++) sb[q] = 0;
                }
                else if (exhausted) done = true;      // no work left anywhere: this lane never asks again
            }
            const u64 taken = bnext + (u64)__popcll(need);
            bnext = taken < bend ? taken : bend;
        }
        if (__ballot(have || !done) == 0) break;     // every lane has seen the counter run dry
        if (MARK == MARK_LOG) {
            // the indices the wave visits in this step go to its log back to back: one contiguous store per wave
            const u64 act = __ballot(have);
            const u32 na = (u32)__popcll(act);
            if (na) {
                if (lcur + na > lend) {
                    const int leader = __ffsll((unsigned long long)act) - 1;
                    unsigned long long cid = 0;
                    if (lane_id() == leader) {
                        if (lend) chunk_fill[lbase / IDX_CHUNK] = (u32)(lcur - lbase);
                        cid = atomicAdd(chunk_ctr, 1ull);
                        if (cid >= log_chunks) { atomicAdd(overflow, 1ull); cid = log_chunks - 1; }   // cannot happen (host sizes the log); stay in bounds
                    }
                    cid = shfl_t((u64)cid, leader);
                    lbase = lcur = cid * IDX_CHUNK;
                    lend = lbase + IDX_CHUNK;
                }
                if (have) { idxlog[lcur + (u64)__popcll(act & lanemask_lt())] = x; atomicAdd(&bseen[x >> IDX_RANGE_LOG2], 1u); }
                lcur += na;
            }
        }
        if (MARK == MARK_MOMENTS && have) {
            const u32 b = x & (mom_classes - 1u);                           // classes by the low bits: the unreached elements of real inputs cluster in rank
            const unsigned long long o = x >> mom_shift;
            atomicAdd(&mcnt[b], 1u); atomicAdd(&msum[b], o); atomicAdd(&msq[b], o * o);
        }
        if (have) {
            const u32 y = LF[x];
            const u32 bx = SYM == SYM_FROM_INPUT ? (u32)Bsym[x] : 0u;  // (depends on x alone: in flight together with LF[x])
            if (MARK == MARK_BYTEMAP) marks[x] = 1;
            else if (MARK == MARK_SENTINEL) LF[x] = LF_VISITED;       // the entry is not needed again
            {
                const u32 sh = (SYM == SYM_FROM_INPUT ? bx : symbol_of(Ctab, y)) << (8 * (len & 3u));
                const u32 w = (len >> 2) & (u32)(SBW - 1);
#pragma unroll
                for (int q = 0; q < SBW; q++) sb[q] |= w == (u32)q ? sh : 0u;
            }
            if ((len & SBM) == SBM) {                        // (only reached when the slot holds at least a block)
                uint4 *d = (uint4 *)(seg + my * slot + (len & ~SBM));
#pragma unroll
                for (int q = 0; q < SBW / 4; q++) d[q] = make_uint4(sb[4 * q], sb[4 * q + 1], sb[4 * q + 2], sb[4 * q + 3]);
#pragma unroll
                for (int q = 0; q < SBW; q++) sb[q] = 0;
            }
            len++;
            x = y;
            const bool at_splitter = (x & gmask) == 0;
            if (at_splitter || len == slot) {
                if (len & SBM) {                                                                             // slot is a multiple of 16
                    uint4 *d = (uint4 *)(seg + my * slot + (len & ~SBM));
                    const u32 rem = len & SBM;
#pragma unroll
                    for (int q = 0; q < SBW / 4; q++) if ((u32)q * 16u < rem) d[q] = make_uint4(sb[4 * q], sb[4 * q + 1], sb[4 * q + 2], sb[4 * q + 3]);
                }
                u64 next_node;
                if (at_splitter) {
                    next_node = x >> g;
                    have = false;
                } else {
                    next_node = s + atomicAdd(vcount, 1ull);
                    if (next_node >= node_cap) { atomicAdd(overflow, 1ull); next_node = node_cap - 1; }
                }
                noderec[my] = make_uint4((u32)next_node, len, mn, mnoff);
                if (!at_splitter) {
                    my = next_node; len = 0; mn = x; mnoff = 0;
#pragma unroll
                    for (int q = 0; q < SBW; q++) sb[q] = 0;
                }
            } else if (x < mn) { mn = x; mnoff = len; }
        }
    }
    if (MARK == MARK_LOG && lend && lane_id() == 0) chunk_fill[lbase / IDX_CHUNK] = (u32)(lcur - lbase);
    if (MARK == MARK_LOG) {
        __syncthreads();                  // every wave leaves the loop (the pool runs dry for all of them)
        for (u32 b = threadIdx.x; b < nbuckets; b += 256) { const u32 c = bseen[b]; if (c) atomicAdd(&bucket_seen[b], c); }
    }
    if (MARK == MARK_MOMENTS) {
        __syncthreads();
        for (u32 b = threadIdx.x; b < mom_classes; b += 256) {
            const u32 c = mcnt[b];
            if (c) { atomicAdd(&mom[b], (unsigned long long)c); atomicAdd(&mom[mom_classes + b], msum[b]); atomicAdd(&mom[2 * mom_classes + b], msq[b]); }
        }
    }
#ifdef WALK_PROFILE
    if (lane_id() == 0) { atomicMax(&prof[2], (unsigned long long)wall_clock64()); atomicMin(&prof[4], (unsigned long long)wall_clock64()); }
#endif
}
template <int MARK, int SBW = 16>
__global__ __launch_bounds__(256) void walk_record_kernel(u32 *__restrict__ LF, u8 *__restrict__ marks, u32 *__restrict__ idxlog, u64 s, u64 node_cap, int g, u32 slot,
                                                          const u64 *__restrict__ Cg, u8 *__restrict__ seg, uint4 *__restrict__ noderec,
                                                          unsigned long long *__restrict__ ticket,
                                                          unsigned long long *__restrict__ vcount,
                                                          unsigned long long *__restrict__ overflow,
                                                          unsigned long long *__restrict__ chunk_ctr, u32 *__restrict__ chunk_fill, u64 log_chunks,
                                                          u32 nbuckets, u32 *__restrict__ bucket_seen,
                                                          int mom_shift = 0, unsigned long long *__restrict__ mom = nullptr)
{
    walk_record_body<MARK, SBW, SYM_FROM_C>(LF, marks, idxlog, s, node_cap, g, slot, Cg, nullptr, seg, noderec, ticket, vcount, overflow, chunk_ctr, chunk_fill, log_chunks,
                                            nbuckets, bucket_seen, mom_shift, mom);
}
// the same walk over the shared pass's LF (cycles that each lie inside one segment): symbols from the input
template <int MARK, int SBW = 16>
__global__ __launch_bounds__(256) void walk_record_seg_kernel(u32 *__restrict__ LF, u8 *__restrict__ marks, u32 *__restrict__ idxlog, u64 s, u64 node_cap, int g, u32 slot,
                                                              const u8 *__restrict__ B, u8 *__restrict__ seg, uint4 *__restrict__ noderec,
                                                              unsigned long long *__restrict__ ticket,
                                                              unsigned long long *__restrict__ vcount,
                                                              unsigned long long *__restrict__ overflow,
                                                              unsigned long long *__restrict__ chunk_ctr, u32 *__restrict__ chunk_fill, u64 log_chunks,
                                                              u32 nbuckets, u32 *__restrict__ bucket_seen,
                                                              int mom_shift = 0, unsigned long long *__restrict__ mom = nullptr)
{
    walk_record_body<MARK, SBW, SYM_FROM_INPUT>(LF, marks, idxlog, s, node_cap, g, slot, nullptr, B, seg, noderec, ticket, vcount, overflow, chunk_ctr, chunk_fill, log_chunks,
                                                nbuckets, bucket_seen, mom_shift, mom);
}

// out[end_c - t] = B[LF^t(min_c)] (unbwts.c:73-82): node v's recorded symbols go to out[opos - i], wrapping to the
// cycle's end once the walk passes the cycle's smallest element.  A thread moves 16 symbols at a time: one aligned
// 16-byte load from the node's slot, bytes reversed in registers, one 16-byte store (the destination is not aligned in
// general: the store goes through a packed type, so the compiler picks what the target allows).  The one chunk of a
// node that straddles the wrap point, and a ragged tail, go byte by byte.
struct __attribute__((packed, aligned(1))) Unaligned16 { u32 w[4]; };
__global__ __launch_bounds__(256) void place_segments_kernel(const u8 *__restrict__ seg, u64 nodes, u32 slot, int tpn_log2,
                                                             const uint4 *__restrict__ noderec, const u32 *__restrict__ opos,
                                                             const u32 *__restrict__ wrap_at, const u32 *__restrict__ cyc_len,
                                                             u8 *__restrict__ out)
{
    const u64 gid = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 v = gid >> tpn_log2;
    if (v >= nodes) return;
    const u32 sub = (u32)(gid & ((1ull << tpn_log2) - 1ull)), tpn = 1u << tpn_log2;
    const u32 len = noderec[v].y, o = opos[v], wr = wrap_at[v], L = cyc_len[v];
    const u8 *src = seg + v * slot;
    for (u32 c = sub * 16; c < len; c += tpn * 16) {
        if (c + 16 <= len && (c + 16 <= wr || c >= wr)) {
            const uint4 q = *(const uint4 *)(src + c);
            // symbols c .. c+15 land on out[base - 15 .. base], last symbol first
            const u64 base = c >= wr ? (u64)o - c + L : (u64)o - c;
            Unaligned16 r;
            r.w[0] = __builtin_bswap32(q.w); r.w[1] = __builtin_bswap32(q.z);
            r.w[2] = __builtin_bswap32(q.y); r.w[3] = __builtin_bswap32(q.x);
            *(Unaligned16 *)(out + base - 15) = r;
        } else {
            const u32 e = c + 16 < len ? c + 16 : len;
            for (u32 i = c; i < e; i++) out[i >= wr ? (u64)o - i + L : (u64)o - i] = src[i];
        }
    }
}

// ------------------------------------------------------------------------------------
// elements no walk reached (cycles without a splitter): one sweep, wave-aggregated append
// ------------------------------------------------------------------------------------
template <int MARK>
__global__ __launch_bounds__(256) void collect_unvisited_kernel(const u32 *__restrict__ LF, const u8 *__restrict__ marks, u64 n,
                                                                u32 *__restrict__ uidx, u32 *__restrict__ ulf, u64 cap,
                                                                unsigned long long *__restrict__ count)
{
    for (u64 base = (u64)blockIdx.x * 256; base < n; base += (u64)gridDim.x * 256) {
        const u64 i = base + threadIdx.x;
        bool un = false;
        u32 v = 0;
        if (i < n) {
            if (MARK == MARK_BYTEMAP) { un = marks[i] == 0; if (un) v = LF[i]; }
            else { v = LF[i]; un = v != LF_VISITED; }
        }
        const u64 m = __ballot(un);
        if (m) {
            const int leader = __ffsll((unsigned long long)m) - 1;
            unsigned long long b = 0;
            if (lane_id() == leader) b = atomicAdd(count, (unsigned long long)__popcll(m));
            b = shfl_t((u64)b, leader);
            if (un) {
                const u64 at = b + (u64)__popcll(m & lanemask_lt());
                if (at < cap) { uidx[at] = (u32)i; ulf[at] = v; }
            }
        }
    }
}

// ---- index-log mode: which indices did no walk log? ------------------------------------------------------------------
// Step 1: the logged indices are appended to buckets of 2^IDX_RANGE_LOG2 consecutive index values.  A workgroup takes
// one log chunk (its first chunk_fill[] entries): counts per bucket in LDS, reserves room in every bucket the chunk
// touches (one global atomic each; the counters sit on separate cache lines), orders the chunk by bucket in LDS and
// copies it out, so a bucket's share leaves as one contiguous run instead of one request per entry.
// Step 2: one workgroup per bucket sets a bit per logged index in an LDS bitmap and reports the zero bits.
// Step 0: the walk counted the visited indices of every bucket; only DEFICIENT buckets (count < size) can hold an unvisited
// index, and only their log entries take part in steps 1 and 2 (natural inputs: a few dozen unvisited elements, so a
// few percent of the buckets).
__global__ __launch_bounds__(256) void bucket_deficit_kernel(const u32 *__restrict__ bucket_seen, u32 nbuckets, u64 n, u32 *__restrict__ deficient)
{
    const u32 b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nbuckets) return;
    const u64 lo = (u64)b << IDX_RANGE_LOG2;
    const u64 size = n - lo < (1ull << IDX_RANGE_LOG2) ? n - lo : (1ull << IDX_RANGE_LOG2);
    deficient[b] = (u64)bucket_seen[b] < size ? 1u : 0u;
}

static inline size_t bucket_indices_lds_bytes(u32 nbuckets) { return (size_t)IDX_CHUNK * 4 + 3 * (size_t)nbuckets * 4; }
__global__ __launch_bounds__(IDX_THREADS) void bucket_indices_kernel(const u32 *__restrict__ idxlog, const u32 *__restrict__ chunk_fill,
                                                                     u32 nbuckets, const u32 *__restrict__ deficient,
                                                                     u32 *__restrict__ bucket_fill, u32 *__restrict__ bucket_data)
{
    extern __shared__ __attribute__((aligned(16))) u32 idx_lds[];
    u32 *sorted = idx_lds;                    // IDX_CHUNK entries ordered by bucket
    u32 *cnt = idx_lds + IDX_CHUNK;           // per bucket: count, then the fill cursor within `sorted`
    u32 *delta = cnt + nbuckets;              // per bucket: (reserved offset in the bucket) - (start in `sorted`)
    u32 *defl = delta + nbuckets;             // per bucket: takes part?
    __shared__ u32 scan_sm[IDX_THREADS / 64];
    const int tid = threadIdx.x;
    const u32 clen = chunk_fill[blockIdx.x];
    if (clen == 0) return;
    const u32 *src = idxlog + (u64)blockIdx.x * IDX_CHUNK;
    u32 x[IDX_PER_THREAD];
#pragma unroll
    for (int q = 0; q < IDX_PER_THREAD; q++) {
        const u32 i = (u32)q * IDX_THREADS + tid;
        x[q] = i < clen ? src[i] : 0u;
    }
    for (u32 b = tid; b < nbuckets; b += IDX_THREADS) { cnt[b] = 0; defl[b] = deficient[b]; }
    __syncthreads();
    u32 keep = 0;                             // bit q: entry q exists and its bucket takes part
#pragma unroll
    for (int q = 0; q < IDX_PER_THREAD; q++)
        if ((u32)q * IDX_THREADS + tid < clen && defl[x[q] >> IDX_RANGE_LOG2]) { keep |= 1u << q; atomicAdd(&cnt[x[q] >> IDX_RANGE_LOG2], 1u); }
    if (__syncthreads_or(keep != 0) == 0) return;       // nothing of this chunk lies in a deficient bucket
    // exclusive scan of the counts -> start of each bucket's run in `sorted`; room in the bucket from a global atomic
    u32 kept = 0;                             // entries of this chunk that take part
    {
        const u32 per = (nbuckets + IDX_THREADS - 1) / IDX_THREADS;      // buckets a thread scans (<= 8)
        u32 c[8], run = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const u32 b = (u32)tid * per + j;
            c[j] = (u32)j < per && b < nbuckets ? cnt[b] : 0u;
            run += c[j];
        }
        u32 exc = block_scan_exclusive<u32, OpAdd, IDX_THREADS / 64>(run, OpAdd(), 0u, scan_sm, &kept);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const u32 b = (u32)tid * per + j;
            if ((u32)j < per && b < nbuckets) {
                const u32 g = c[j] ? atomicAdd(&bucket_fill[(size_t)b * IDX_FILL_STRIDE], c[j]) : 0u;
                cnt[b] = exc;
                delta[b] = g - exc;
                exc += c[j];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < IDX_PER_THREAD; q++)
        if ((keep >> q) & 1u) sorted[atomicAdd(&cnt[x[q] >> IDX_RANGE_LOG2], 1u)] = x[q];
    __syncthreads();
    for (u32 i = tid; i < kept; i += IDX_THREADS) {
        const u32 v = sorted[i], b = v >> IDX_RANGE_LOG2;
        bucket_data[((u64)b << IDX_RANGE_LOG2) + (u32)(delta[b] + i)] = v;
    }
}

__global__ __launch_bounds__(1024) void unvisited_from_buckets_kernel(const u32 *__restrict__ deficient, const u32 *__restrict__ bucket_fill,
                                                                      const u32 *__restrict__ bucket_data,
                                                                      const u32 *__restrict__ LF, u64 n, u32 *__restrict__ uidx,
                                                                      u32 *__restrict__ ulf, u64 cap, unsigned long long *__restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) u32 bm[];      // 2^IDX_RANGE_LOG2 bits = 128 KB (dynamic: above the static limit)
    const u32 b = blockIdx.x;
    if (!deficient[b]) return;
    for (u32 w = threadIdx.x; w < (1u << IDX_RANGE_LOG2) / 32; w += 1024) bm[w] = 0;
    __syncthreads();
    const u32 fill = bucket_fill[(size_t)b * IDX_FILL_STRIDE];
    const u32 *src = bucket_data + ((u64)b << IDX_RANGE_LOG2);
    for (u32 i = threadIdx.x; i < fill; i += 1024) {
        const u32 o = src[i] & ((1u << IDX_RANGE_LOG2) - 1u);
        atomicOr(&bm[o >> 5], 1u << (o & 31u));
    }
    __syncthreads();
    // natural inputs leave a few dozen zero bits; constant or sorted inputs leave nearly all of them: the room in the
    // list is reserved once per wave and step, not once per element
    const u64 lo = (u64)b << IDX_RANGE_LOG2;
    for (u32 w0 = 0; w0 < (1u << IDX_RANGE_LOG2) / 32; w0 += 1024) {
        const u32 w = w0 + threadIdx.x;
        u32 zeros = ~bm[w];
        const u64 xbase = lo + (u64)w * 32;
        if (xbase >= n) zeros = 0;
        else if (n - xbase < 32) zeros &= (1u << (u32)(n - xbase)) - 1u;
        const u32 mine = (u32)__popc(zeros);
        const u32 inc = wave_scan_inclusive(mine, OpAdd());
        const u32 tot = shfl_t(inc, 63);
        if (tot == 0) continue;
        unsigned long long base = 0;
        if (lane_id() == 63) base = atomicAdd(count, (unsigned long long)tot);
        base = shfl_t((u64)base, 63);
        u64 at = base + (inc - mine);
        while (zeros) {
            const u32 bit = (u32)__ffs((int)zeros) - 1u;
            zeros &= zeros - 1u;
            const u64 x = xbase + bit;
            if (at < cap) { uidx[at] = (u32)x; ulf[at] = LF[x]; }
            at++;
        }
    }
}

// ------------------------------------------------------------------------------------
// reduced-list ranking (splitter nodes): two levels, linear work
// ------------------------------------------------------------------------------------
// node v (noderec[v]): x = next node on its cycle, y = elements in its segment, z = smallest element of the segment,
// w = that element's distance from the node's first element.  Wanted per node: where its segment goes in the text, i.e.
// its cycle's end position, the cycle's length, and the node's distance from the cycle's smallest element.
//
// Pointer jumping over all nodes is O(s log s) work in 2 log s launches; that is what kept the splitter spacing G large.
// Instead every L2_H-th node is a level-2 splitter: a lane walks the node list from its level-2 splitter to the next one
// (lr2_walk_kernel: sums, minima, visit marks), nodes no such walk reached -- node cycles without a level-2 splitter --
// join the level-2 list as they are (lr2_collect / lr2_fill), the level-2 list (~ s / L2_H entries) is ranked by pointer
// jumping, and a second walk hands the positions down to the nodes (lr2_distribute_kernel).
#define L2_H 32
#define LR_NIL 0xffffffffu

__global__ __launch_bounds__(256) void lr2_walk_kernel(const uint4 *__restrict__ noderec, u64 s2, u8 *__restrict__ visited, uint4 *__restrict__ rec2)
{
    const u64 w = (u64)blockIdx.x * 256 + threadIdx.x;
    if (w >= s2) return;
    u32 v = (u32)(w * L2_H), acc = 0, mn = 0, mnoff = 0;
    bool first = true;
    do {
        const uint4 r = noderec[v];
        visited[v] = 1;
        if (first || r.z < mn) { mn = r.z; mnoff = acc + r.w; first = false; }
        acc += r.y;
        v = r.x;
    } while (v % L2_H != 0);
    rec2[w] = make_uint4(v / L2_H, acc, mn, mnoff);
}

// nodes on cycles without a level-2 splitter: each becomes a level-2 entry of its own (id = s2 + position in U)
__global__ __launch_bounds__(256) void lr2_collect_kernel(const u8 *__restrict__ visited, u64 s_all, u64 s2, u32 *__restrict__ U,
                                                          u32 *__restrict__ id2of, unsigned long long *__restrict__ count)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    const bool un = v < s_all && !visited[v];
    const u64 m = __ballot(un);
    if (m == 0) return;
    const int leader = __ffsll((unsigned long long)m) - 1;
    unsigned long long b = 0;
    if (lane_id() == leader) b = atomicAdd(count, (unsigned long long)__popcll(m));
    b = shfl_t((u64)b, leader);
    if (un) {
        const u64 at = b + (u64)__popcll(m & lanemask_lt());
        U[at] = (u32)v;
        id2of[v] = (u32)(s2 + at);
    }
}
__global__ __launch_bounds__(256) void lr2_fill_kernel(const u32 *__restrict__ U, u64 nu2, u64 s2, const uint4 *__restrict__ noderec,
                                                       const u32 *__restrict__ id2of, uint4 *__restrict__ rec2)
{
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j >= nu2) return;
    const uint4 r = noderec[U[j]];
    rec2[s2 + j] = make_uint4(id2of[r.x], r.y, r.z, r.w);       // the successor of an unreached node is unreached too
}

// ---- pointer jumping over the level-2 list -------------------------------------------------------------------------
// A round reads the record of the entry it hops to: the fields travel together (16 and 8 bytes), so a round costs one
// random line fill per entry instead of three (two).
//   LrMin  x = smallest entry id seen (-> leader), y = smallest element seen, z = hop target
//   LrSum  x = segment lengths summed up to the cut, y = hop target (LR_NIL at the cut)
typedef uint4 LrMin;
typedef uint2 LrSum;

__global__ __launch_bounds__(256) void lr_init_kernel(u64 s, const uint4 *__restrict__ rec2, LrMin *__restrict__ rec)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v < s) { const uint4 r = rec2[v]; rec[v] = make_uint4((u32)v, r.z, r.x, 0u); }
}

// after r rounds an entry has folded in the 2^r entries that follow it
__global__ __launch_bounds__(256) void lr_jump_min_kernel(u64 s, const LrMin *__restrict__ in, LrMin *__restrict__ out)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v >= s) return;
    const LrMin a = in[v];
    const LrMin b = in[a.z];
    out[v] = make_uint4(a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y, b.z, 0u);
}

// cut every cycle in front of its leader, then suffix sums of the lengths
__global__ __launch_bounds__(256) void lr_cut_kernel(u64 s, const uint4 *__restrict__ rec2, const LrMin *__restrict__ rec, LrSum *__restrict__ sh)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v < s) { const uint4 r = rec2[v]; sh[v] = make_uint2(r.y, r.x == rec[v].x ? LR_NIL : r.x); }
}

__global__ __launch_bounds__(256) void lr_jump_sum_kernel(u64 s, const LrSum *__restrict__ in, LrSum *__restrict__ out)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v >= s) return;
    const LrSum a = in[v];
    if (a.y == LR_NIL) out[v] = a;
    else { const LrSum b = in[a.y]; out[v] = make_uint2(a.x + b.x, b.y); }
}

// One record per LF cycle, for the ordering by smallest element (unbwts.c:62-77).  leader = level-2 leader entry, or
// LR_NIL for a cycle without a splitter (resolved by tiny_cycle_scan_kernel).
struct CycleRec { u32 leader; u32 minelem; u32 len; u32 pad; };

// dist[v] = elements between the leader's first element and v's; the entry whose stretch holds the cycle's smallest
// element publishes that element's distance; leaders append a cycle record
__global__ __launch_bounds__(256) void lr_finish_kernel(u64 s, const LrMin *__restrict__ rec, const LrSum *__restrict__ sh,
                                                        const uint4 *__restrict__ rec2, u32 *__restrict__ dist,
                                                        u32 *__restrict__ min_dist /* by leader */, CycleRec *__restrict__ recs,
                                                        unsigned long long *__restrict__ nrec)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v >= s) return;
    const LrMin r = rec[v];
    const u32 l = r.x;
    const u32 L = sh[l].x;
    const u32 d = L - sh[v].x;
    dist[v] = d;
    const uint4 r2 = rec2[v];
    if (r2.z == r.y) min_dist[l] = d + r2.w;
    if (l == (u32)v) {
        const unsigned long long at = atomicAdd(nrec, 1ull);
        CycleRec c; c.leader = l; c.minelem = r.y; c.len = L; c.pad = 0;
        recs[at] = c;
    }
}

// level-2 entry -> distance of its first element from the cycle's smallest element, the cycle's length and end
__global__ __launch_bounds__(256) void lr_place2_kernel(u64 s, const LrMin *__restrict__ rec, const LrSum *__restrict__ sh,
                                                        const u32 *__restrict__ dist, const u32 *__restrict__ min_dist,
                                                        const u32 *__restrict__ end_by_leader, uint4 *__restrict__ place2)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v >= s) return;
    const u32 l = rec[v].x;
    const u32 L = sh[l].x;                       // a cycle of 2^32 elements reads as 0: the arithmetic below is mod 2^32
    const u32 dm = min_dist[l];
    const u32 d = dist[v];
    const u32 t = d >= dm ? d - dm : d + L - dm;
    place2[v] = make_uint4(t, L, end_by_leader[l], 0u);
}

// hands the positions down to the nodes: opos = text position of the node's first symbol, wrap_at = symbols until the
// walk passes the cycle's smallest element (the text position wraps to the cycle's end there), cyc_len
__global__ __launch_bounds__(256) void lr2_distribute_kernel(const uint4 *__restrict__ noderec, u64 s2, u64 s2all, const u32 *__restrict__ U,
                                                             const uint4 *__restrict__ place2, u32 *__restrict__ opos,
                                                             u32 *__restrict__ wrap_at, u32 *__restrict__ cyc_len)
{
    const u64 w = (u64)blockIdx.x * 256 + threadIdx.x;
    if (w >= s2all) return;
    const uint4 pl = place2[w];
    const u64 L = pl.y ? (u64)pl.y : 0x100000000ull;
    u64 t = pl.x;
    if (w >= s2) {
        const u32 v = U[w - s2];
        opos[v] = pl.z - (u32)t; wrap_at[v] = (u32)(L - t); cyc_len[v] = (u32)L;
        return;
    }
    u32 v = (u32)(w * L2_H);
    do {
        const uint4 r = noderec[v];
        opos[v] = pl.z - (u32)t; wrap_at[v] = (u32)(L - t); cyc_len[v] = (u32)L;
        t += r.y;
        if (t >= L) t -= L;
        v = r.x;
    } while (v % L2_H != 0);
}

// ------------------------------------------------------------------------------------
// MARK_MOMENTS: the unreached elements from the ranges' counts, sums and sums of squares
// ------------------------------------------------------------------------------------
// missing = size - count; one missing index: its offset is (sum of all offsets) - (sum seen); two: their sum A and the sum of their
// squares B give (o1 - o2)^2 = 2 B - A^2.  More: the class stays OPEN.
// Real text leaves a few hundred unreached elements (the cycles of its short Lyndon factors), and with 2^10 classes a few dozen
// classes miss three or more: what the arithmetic cannot name, the CYCLES can -- an unreached element's whole cycle is unreached, so
// every element found by arithmetic walks its cycle and the smallest such element of a cycle adds the cycle's members that sit in
// open classes to the list and to their classes' moments; then the open classes are looked at again (fewer missing now), up to
// MOM_PASSES times.  Classes still open after that go onto the list for moments_chase_kernel.  One workgroup: the classes are few.
// cstat[class]: MOM_OPEN, 0 = nothing missing, p = named by arithmetic in pass p.
// counters: [1] unreached elements (as for the other marks), [10] listed classes, [11] the arithmetic did not come out / no room (fall back to the log)
#define MOM_OPEN 0xffffffffu
#define MOM_PASSES 3
__global__ __launch_bounds__(1024) void moments_resolve_kernel(unsigned long long *__restrict__ mom, u32 *__restrict__ cstat, u64 n, int shift /* log2 of the class count */,
                                                               const u32 *__restrict__ LF, u32 *__restrict__ uidx, u32 *__restrict__ ulf, u64 ucap,
                                                               u32 *__restrict__ def_list, unsigned long long *__restrict__ counters, u32 cap)
{
    __shared__ unsigned long long s_from, s_to, s_listed;
    const u64 classes = 1ull << shift;
    const u32 cmask = (u32)classes - 1u;
    for (u64 b = threadIdx.x; b < classes; b += 1024) cstat[b] = MOM_OPEN;
    __threadfence(); __syncthreads();
    for (u32 pass = 1; pass <= MOM_PASSES + 1; pass++) {
        const bool arith = pass <= MOM_PASSES;              // the last look only sorts the classes into complete and listed
        if (threadIdx.x == 0) { s_from = counters[1]; counters[10] = 0; }
        __threadfence(); __syncthreads();
        for (u64 b = threadIdx.x; b < classes && b < n; b += 1024) {
            if (cstat[b] != MOM_OPEN) continue;
            const u64 size = (n - b + classes - 1) >> shift;                 // indices x < n with x mod classes = b: x = o * classes + b, o < size
            const u64 cnt = mom[b];
            if (cnt > size) { atomicAdd(&counters[11], 1ull); continue; }
            const u64 d = size - cnt;
            if (d == 0) { cstat[b] = 0; continue; }
            if (d > 2 || !arith) { const unsigned long long at = atomicAdd(&counters[10], 1ull); def_list[at] = (u32)b; continue; }
            // sums over all offsets 0 .. size - 1 (mod 2^64: the differences below are small and come out exact)
            const u64 sall = size * (size - 1) / 2;
            u64 f[3] = {size - 1, size, 2 * size - 1};                        // (size-1) size (2 size - 1) / 6, dividing before the products overflow
            { int two = 0, three = 0; for (int i = 0; i < 3; i++) { if (!two && f[i] % 2 == 0) { f[i] /= 2; two = 1; } } for (int i = 0; i < 3; i++) { if (!three && f[i] % 3 == 0) { f[i] /= 3; three = 1; } } }
            const u64 qall = f[0] * f[1] * f[2];
            const u64 A = sall - mom[classes + b], B = qall - mom[2 * classes + b];
            if (d == 1) {
                if (A >= size || A * A != B) { atomicAdd(&counters[11], 1ull); continue; }
                const unsigned long long at = atomicAdd(&counters[1], 1ull);
                if (at < ucap) { const u32 x = (u32)((A << shift) | b); uidx[at] = x; ulf[at] = LF[x]; } else atomicAdd(&counters[11], 1ull);
            } else {
                const u64 D = 2 * B - A * A;                                     // (o1 - o2)^2
                u64 r = (u64)sqrt((double)D);
                while (r * r > D) r--;
                while ((r + 1) * (r + 1) <= D) r++;
                const u64 o1 = (A - r) / 2, o2 = (A + r) / 2;
                if (r * r != D || r == 0 || ((A - r) & 1) || o2 >= size || o1 * o1 + o2 * o2 != B) { atomicAdd(&counters[11], 1ull); continue; }
                const unsigned long long at = atomicAdd(&counters[1], 2ull);
                if (at + 1 < ucap) {
                    const u32 x1 = (u32)((o1 << shift) | b), x2 = (u32)((o2 << shift) | b);
                    uidx[at] = x1; ulf[at] = LF[x1]; uidx[at + 1] = x2; ulf[at + 1] = LF[x2];
                } else atomicAdd(&counters[11], 1ull);
            }
            cstat[b] = pass;
        }
        __threadfence(); __syncthreads();
        if (threadIdx.x == 0) { s_to = counters[1]; s_listed = counters[10]; }
        __syncthreads();
        if (!arith || s_listed == 0 || counters[11]) break;              // (the same values for every thread: one decision)
        // the cycles of what this pass named
        const u64 from = s_from, to = s_to < ucap ? s_to : ucap;
        for (u64 i = from + threadIdx.x; i < to; i += 1024) {
            const u32 x = uidx[i];
            bool leader = true, open_seen = false;
            u32 steps = 0;
            for (u32 y = ulf[i]; y != x; y = LF[y]) {
                const u32 st = cstat[y & cmask];
                if (st == pass && y < x) { leader = false; break; }
                if (st == MOM_OPEN) open_seen = true;
                if (++steps > cap) { atomicAdd(&counters[11], 1ull); leader = false; break; }
            }
            if (!leader || !open_seen) continue;
            for (u32 y = ulf[i]; y != x; y = LF[y]) {
                const u32 cls = y & cmask;
                if (cstat[cls] != MOM_OPEN) continue;
                const unsigned long long at = atomicAdd(&counters[1], 1ull);
                if (at < ucap) { uidx[at] = y; ulf[at] = LF[y]; } else atomicAdd(&counters[11], 1ull);
                const unsigned long long o = y >> shift;
                atomicAdd(&mom[cls], 1ull); atomicAdd(&mom[classes + cls], o); atomicAdd(&mom[2 * classes + cls], o * o);
            }
        }
        __threadfence(); __syncthreads();
    }
}
// (own launch, after the one above: all ranges are listed) more elements to search than the budget allows: fall back to the log instead
__global__ void moments_budget_kernel(unsigned long long *__restrict__ counters, u64 per_class, u64 budget)
{
    if (threadIdx.x == 0 && blockIdx.x == 0 && counters[10] * per_class > budget) { counters[11] += 1; counters[10] = 0; }
}
// every element of the listed ranges follows LF until it stands on a splitter (a walk came through it: reached) or on itself
// (its cycle holds no splitter: unreached).  `cap` steps without either: counters[11] (the caller falls back to the log).
__global__ __launch_bounds__(256) void moments_chase_kernel(const u32 *__restrict__ def_list, const unsigned long long *__restrict__ counters_in, u64 n, int shift, int g,
                                                            const u32 *__restrict__ LF, u32 cap, u32 *__restrict__ uidx, u32 *__restrict__ ulf, u64 ucap,
                                                            unsigned long long *__restrict__ counters, const u32 *__restrict__ cstat)
{
    const u32 cmask = (1u << shift) - 1u;
    const u64 classes = counters_in[10];
    const u64 members = (n + (1ull << shift) - 1) >> shift;                  // quotients a class may hold
    const u64 per = (members + 255) / 256;                                   // 256-element pieces per class
    const u32 gmask = (1u << g) - 1u;
    for (u64 w = blockIdx.x; w < classes * per; w += gridDim.x) {
        const u64 x0 = (((w % per) * 256 + threadIdx.x) << shift) | (u64)def_list[w / per];
        bool un = false;
        if (x0 < n) {
            if ((x0 & gmask) != 0) {                                         // a splitter is where a walk starts: reached
                // (a cycle that holds an element of a class no longer open is on the list already: moments_resolve_kernel walked it)
                u32 y = LF[x0], steps = 0;
                bool listed = false;
                for (;;) {
                    if (y == (u32)x0) { un = !listed; break; }
                    if ((y & gmask) == 0) break;
                    if (cstat[y & cmask] != MOM_OPEN) listed = true;
                    if (++steps > cap) { atomicAdd(&counters[11], 1ull); break; }
                    y = LF[y];
                }
            }
        }
        const u64 m = __ballot(un);
        if (m) {
            const int leader = __ffsll((unsigned long long)m) - 1;
            unsigned long long bse = 0;
            if (lane_id() == leader) bse = atomicAdd(&counters[1], (unsigned long long)__popcll(m));
            bse = shfl_t((u64)bse, leader);
            if (un) { const u64 at = bse + (u64)__popcll(m & lanemask_lt()); if (at < ucap) { uidx[at] = (u32)x0; ulf[at] = LF[x0]; } }
        }
    }
}

// ------------------------------------------------------------------------------------
// cycles without a splitter (elements no walk reached)
// ------------------------------------------------------------------------------------
// Natural inputs leave a few dozen such elements (tiny Lyndon factors); a constant or sorted input leaves nearly all n
// (LF is close to the identity).  Everything here is sized by their number and stays on the device.
// An unreached element follows its own cycle until it meets a smaller element (not the cycle's minimum: done) or
// returns to itself (it is the minimum: it appends the cycle's record).  `cap` bounds the steps of one lane.
__global__ __launch_bounds__(256) void tiny_cycle_scan_kernel(const u32 *__restrict__ uidx, const u32 *__restrict__ ulf, u64 nu,
                                                              const u32 *__restrict__ LF, u32 cap, uint2 *__restrict__ tiny /* x smallest element, y length */,
                                                              unsigned long long *__restrict__ count, unsigned long long *__restrict__ overflow)
{
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    bool ismin = false;
    u32 x = 0, len = 1;
    if (q < nu) {
        x = uidx[q];
        u32 y = ulf[q];
        ismin = true;
        while (y != x) {
            if (y < x) { ismin = false; break; }
            y = LF[y];
            if (++len > cap) { atomicAdd(overflow, 1ull); ismin = false; break; }
        }
    }
    const u64 m = __ballot(ismin);
    if (m == 0) return;
    const int leader = __ffsll((unsigned long long)m) - 1;
    unsigned long long b = 0;
    if (lane_id() == leader) b = atomicAdd(count, (unsigned long long)__popcll(m));
    b = shfl_t((u64)b, leader);
    if (ismin) tiny[b + (u64)__popcll(m & lanemask_lt())] = make_uint2(x, len);
}

// ---- cycle order: by smallest element, the cycle holding index 0 ends the text (unbwts.c:62-77) ------------------------
// record i of the combined list: a cycle without a splitter (i < kt) or a cycle of the reduced list
struct CycleList {
    const uint2 *tiny; u64 kt; const CycleRec *recs; u64 kc;
    __device__ __forceinline__ u32 minelem(u64 i) const { return i < kt ? tiny[i].x : recs[i - kt].minelem; }
    __device__ __forceinline__ u32 len(u64 i) const { return i < kt ? tiny[i].y : recs[i - kt].len; }
};
__global__ __launch_bounds__(256) void cycle_keys_kernel(CycleList cl, u64 *__restrict__ keys, u32 *__restrict__ vals)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < cl.kt + cl.kc) { keys[i] = cl.minelem(i); vals[i] = (u32)i; }
}
struct CycleLenIn {
    CycleList cl; const u32 *order;
    __device__ __forceinline__ u32 operator()(u64 j) const { return cl.len(order[j]); }
};
struct CycleEndOut {
    CycleList cl; const u32 *order; u32 last; u32 *end_by_leader; u32 *end_of_tiny; u64 *total;
    __device__ __forceinline__ void operator()(u64 j, u32 used) const
    {
        const u32 i = order[j];
        const u32 end = last - used;                    // n - 1 - (elements of the cycles ordered before this one)
        if (i < cl.kt) end_of_tiny[i] = end;
        else end_by_leader[cl.recs[i - cl.kt].leader] = end;
        if (j + 1 == cl.kt + cl.kc) *total = (u64)used + cl.len(i);     // == n (mod 2^32 for n = 2^32)
    }
};

// The shared pass over a run of independent segments (offsets off[0 .. count], run-relative once `base` is taken off): a cycle lies
// inside one segment, so the cycles of earlier segments are ordered first and their lengths sum to that segment's start.  The cycle
// with smallest element m ends at  off[s + 1] - 1 - (used - off[s]),  s = the segment that holds m.
struct SegCycleEndOut {
    CycleList cl; const u32 *order; const u64 *off; u64 count, base; u32 *end_by_leader; u32 *end_of_tiny; u64 *total;
    __device__ __forceinline__ void operator()(u64 j, u32 used) const
    {
        const u32 i = order[j];
        const u64 m = (u64)cl.minelem(i) + base;
        u64 lo = 0, hi = count;                         // largest s with off[s] <= m  (off[0] = base <= m < off[count])
        while (hi - lo > 1) { const u64 mid = (lo + hi) >> 1; if (off[mid] <= m) lo = mid; else hi = mid; }
        const u32 end = (u32)(off[lo + 1] - base) - 1u - (used - (u32)(off[lo] - base));     // (mod 2^32, like the whole-input form)
        if (i < cl.kt) end_of_tiny[i] = end;
        else end_by_leader[cl.recs[i - cl.kt].leader] = end;
        if (j + 1 == cl.kt + cl.kc) *total = (u64)used + cl.len(i);
    }
};

// out[end - t] = B[LF^t(min)] for a cycle without a splitter: unbwts.c:73-82, one lane per cycle
template <int SYM>
__device__ __forceinline__ void tiny_place_body(const uint2 *tiny, u64 kt, const u32 *end_of_tiny, const u32 *LF, const u64 *Ctab /* in LDS */, const u8 *Bsym, u8 *out)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= kt) return;
    const uint2 c = tiny[i];
    u32 x = c.x, pos = end_of_tiny[i];
    for (u32 t = 0; t < c.y; t++) {
        const u32 y = LF[x];
        out[pos--] = SYM == SYM_FROM_INPUT ? Bsym[x] : (u8)symbol_of(Ctab, y);
        x = y;
    }
}
__global__ __launch_bounds__(256) void tiny_place_kernel(const uint2 *__restrict__ tiny, u64 kt, const u32 *__restrict__ end_of_tiny,
                                                         const u32 *__restrict__ LF, const u64 *__restrict__ Cg, u8 *__restrict__ out)
{
    __shared__ u64 Ctab[257];
    for (int i = threadIdx.x; i < 257; i += 256) Ctab[i] = Cg[i];
    __syncthreads();
    tiny_place_body<SYM_FROM_C>(tiny, kt, end_of_tiny, LF, Ctab, nullptr, out);
}
__global__ __launch_bounds__(256) void tiny_place_seg_kernel(const uint2 *__restrict__ tiny, u64 kt, const u32 *__restrict__ end_of_tiny,
                                                             const u32 *__restrict__ LF, const u8 *__restrict__ B, u8 *__restrict__ out)
{
    tiny_place_body<SYM_FROM_INPUT>(tiny, kt, end_of_tiny, LF, nullptr, B, out);
}

// ------------------------------------------------------------------------------------
// driver
// ------------------------------------------------------------------------------------
static int grid1(u64 m) { return (int)((m + 255) / 256); }
static int bit_length(u64 x) { int b = 0; for (; x; x >>= 1) b++; return b; }
int inverse_splitter_log2(u64 n) { const int g = bit_length(n) - 24; return g < 4 ? 4 : g > 8 ? 8 : g; }
static int splitter_log2(const bwts_ctx *ctx, u64 n)
{
    const char *env = bwts_knob(ctx, "BWTS_SPLIT_LOG2");
    const int v = env ? atoi(env) : -1;
    return v >= 0 && v <= 20 ? v : inverse_splitter_log2(n);
}
#define UNV_CAP0 (1ull << 20)     // room for unreached elements before their number is known
// Spare bytes behind the last array of an attempt's arena block (both forms).  No kernel is known to need them: they are what the
// anonymous 256 KiB of the former hand-made sums left over once the moments tables, which lived off it, were declared.
#define INV_ARENA_SLACK ((size_t)1 << 15)
// the error of the launches queued since the last check, as a return code
static int launched(bwts_ctx *ctx) { HIPC(hipGetLastError()); return BWTS_OK; }
// the cycle sort's buffers, a whole pair sort of m elements in side arena 1: keys, values, the radix tables, scan scratch, and the
// 4 KiB of slack that every such block carries
static int cycle_sort_plan(bwts_ctx *ctx, u64 m, SortPlan *cp)
{
    char *sb = nullptr; BlockLayout L;
    L.arrays(m, &cp->keys[0], &cp->keys[1], &cp->vals[0], &cp->vals[1]);
    L.raw(&cp->tile_hist, radix_tile_hist_bytes(m)); L.raw(&cp->scan_temp, scan_temp_bytes(m)); L.pad(4096);
    BWTS_TRY(aux_reserve_slot(ctx, 1, L.bytes(), &sb));
    L.place(sb);
    return BWTS_OK;
}
// the one block an attempt (InvRun, WideRun) holds in the arena
template <typename RUN> static int arena_place(bwts_ctx *ctx, RUN &r)
{
    BlockLayout L; r.declare(L);
    BWTS_TRY(arena_take(ctx, L));
    r.dC = ctx->d_small + 1024;         // symbol boundaries C[0..256] (unbwts.c:38-43)
    return BWTS_OK;
}

enum InvOutcome { INV_DONE,
    INV_RETRY_DENSE,    // the node pool overflowed (adversarial LF), or too many unreached elements for the unit-node ranking: g = 0
    INV_AMBIGUOUS,      // sentinel marks at n = 2^32: the one entry equal to LF_VISITED sat in a cycle without a splitter
    INV_NEED_LOG        // the moments do not name the unreached elements: the index log does
};
// The record of one attempt (ctx->inv_report, read by bwts_debug_inverse_report; include/bwts_test.h names the words): values the stages
// hold on the host anyway, stored as they become known.  An attempt that ends with an error code keeps IR_ERROR as its outcome.
enum InvReportWord { IR_G, IR_MARK, IR_OUTCOME, IR_S, IR_VIRTUAL, IR_NODE_CAP, IR_NU, IR_NU2, IR_UCAP_FIRST, IR_SECOND_COLLECT,
                     IR_LISTED, IR_MOM_FALLBACK, IR_UNIT_RANK, IR_KC, IR_KT, IR_FORM };
enum InvReportForm { IR_FORM_NARROW, IR_FORM_WIDE, IR_FORM_WIDE_COMPACT, IR_FORM_NARROW_SEGMENTED };
#define IR_ERROR 255
static_assert(IR_FORM < INV_REPORT_WORDS, "the record's words");
static u64 *inv_report_open(bwts_ctx *ctx /* null: sizes only */, u64 *spill)
{
    u64 *w = ctx && ctx->inv_attempts_made < INV_REPORT_MAX ? ctx->inv_report[ctx->inv_attempts_made] : spill;
    if (ctx) ctx->inv_attempts_made++;
    memset(w, 0, INV_REPORT_WORDS * sizeof(u64));
    w[IR_OUTCOME] = IR_ERROR;
    return w;
}

#include "wide_inverse.h"         // the 64-bit form; its node ranking (WiRanking, UnitRank) also serves the unit-node route below

// wi_finish_kernel for the main path: the cycles of the unit-node ranking go straight into the record form of the cycles
// without a splitter (smallest element, length) plus their leader
__global__ __launch_bounds__(256) void unit_finish_kernel(u64 s, const WiMin *__restrict__ rec, const WiSum *__restrict__ sh, const WiNode *__restrict__ nodes,
                                                          u64 *__restrict__ dist, u64 *__restrict__ min_dist, uint2 *__restrict__ tiny, u32 *__restrict__ leader,
                                                          unsigned long long *__restrict__ ncyc)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v >= s) return;
    const WiMin r = rec[v];
    const u64 L = sh[r.leader].sum, d = L - sh[v].sum;
    dist[v] = d;
    if (nodes[v].mn == r.mn) min_dist[r.leader] = d + nodes[v].off;
    if (r.leader == (u32)v) {
        const unsigned long long at = atomicAdd(ncyc, 1ull);
        tiny[at] = make_uint2((u32)r.mn, (u32)L);
        leader[at] = r.leader;
    }
}
__global__ __launch_bounds__(256) void unit_ends_kernel(const u32 *__restrict__ leader, const u32 *__restrict__ end_of_tiny, u64 m, u32 *__restrict__ end_by_leader)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < m) end_by_leader[leader[i]] = end_of_tiny[i];
}

// ---- what one attempt holds in the arena: every group declares its arrays once, into the attempt's one BlockLayout ----
struct LfTables {           // the LF map and what builds it
    u32 *LF = nullptr, *tile_hist = nullptr; void *scan_temp = nullptr;
    void declare(BlockLayout &L, u64 n) { L.array(&LF, n); L.raw(&tile_hist, radix_tile_hist_bytes(n)); L.raw(&scan_temp, scan_temp_bytes(n)); }
};
struct NodeTables {         // per node of the reduced list (splitters and virtual nodes): record, recorded symbols, place in the text
    uint4 *noderec = nullptr; u32 *opos = nullptr, *wrap = nullptr, *clen = nullptr, *id2of = nullptr, *U = nullptr; u8 *visited2 = nullptr, *seg = nullptr;
    void declare(BlockLayout &L, u64 node_cap, u32 slot) { L.arrays(node_cap, &noderec, &opos, &wrap, &clen, &id2of, &U, &visited2); L.array(&seg, node_cap * slot); }
};
struct Level2Tables {       // the level-2 list: its records, the two ping-pong pairs of the ranking, the cycles of the reduced list
    uint4 *rec2 = nullptr, *place2 = nullptr; LrMin *lrmin[2] = {nullptr, nullptr}; LrSum *lrsum[2] = {nullptr, nullptr};
    u32 *dist = nullptr, *min_dist = nullptr, *end_by_leader = nullptr; CycleRec *recs2 = nullptr;
    void declare(BlockLayout &L, u64 l2cap) { L.arrays(l2cap, &rec2, &place2, &lrmin[0], &lrmin[1], &lrsum[0], &lrsum[1], &dist, &min_dist, &end_by_leader, &recs2); }
};
struct MomentTables {       // MARK_MOMENTS: the classes' moments, the copy moments_resolve_kernel adds to, listed classes, class states
    unsigned long long *mom = nullptr, *work = nullptr; u32 *def_list = nullptr, *cstat = nullptr;
    void declare(BlockLayout &L) { L.arrays(3 * MOM_MAX_BUCKETS, &mom, &work); L.arrays(MOM_MAX_BUCKETS, &def_list, &cstat); }
};
struct LogTables {          // MARK_LOG: the index log in chunks, the indices of deficient ranges by range, per-range counters
    u32 *idxlog = nullptr, *chunk_fill = nullptr, *bucket_data = nullptr, *bucket_fill = nullptr, *bucket_seen = nullptr;
    u32 *deficient() const { return bucket_seen + IDX_MAX_BUCKETS; }       // bucket_seen: counts, then deficit flags
    void declare(BlockLayout &L, u64 log_chunks, u32 nbuckets)
    {
        L.array(&idxlog, log_chunks * IDX_CHUNK); L.array(&chunk_fill, log_chunks); L.array(&bucket_data, (u64)nbuckets << IDX_RANGE_LOG2);
        L.array(&bucket_fill, (u64)IDX_MAX_BUCKETS * IDX_FILL_STRIDE); L.array(&bucket_seen, 2 * IDX_MAX_BUCKETS);
    }
};
// A run of consecutive segments that one shared pass inverts: its slice off[0 .. count] of the call's device offset table (absolute
// offsets; off[0] = base, the run's first byte, which the pass's indices are relative to)
struct InvSegs { const u64 *off; u64 count, base; };
#define SEG_MOMENTS_MAX_SEGMENTS 128    // a pass over more segments than this looks for its unreached elements with the index log first
// One attempt with splitter spacing 2^g and one way of marking: its sizes (plain arithmetic), its arrays, what one stage hands to the next
struct InvRun {
    u64 n, G, s, tiles, node_cap, l2cap, log_chunks, mom_classes;
    const InvSegs *segs;                                        // the shared pass over segments, or null: the input is one BWT
    const u8 *B = nullptr;                                      // ... whose symbols the walk and the placement read from the input
    int g, mark, mom_shift; u32 slot, nbuckets; unsigned wblocks;
    LfTables lf; NodeTables nd; Level2Tables l2; MomentTables mt; LogTables lg;
    u8 *marks = nullptr; u64 *dC = nullptr;                     // the byte map (MARK_BYTEMAP); symbol boundaries
    u64 ucap = 0; u32 *uidx = nullptr, *ulf = nullptr, *end_of_tiny = nullptr; uint2 *tiny = nullptr;       // side block 0: the unreached elements and their cycles
    u64 s_all = 0, s2 = 0, nu = 0, nu2 = 0, s2all = 0, kc = 0, kt = 0;
    int cur = 0, sc = 0;                                        // which side of lrmin[] / lrsum[] holds the ranking
    bool unit_rank = false;                                     // the unit-node route: its block, taken from the device for the call
    UnitRank unit; u32 *uend = nullptr, *uleader = nullptr; ScopedDeviceBlock ub;
    u64 rep_spill[INV_REPORT_WORDS], *rep;                      // this attempt's record
    InvRun(bwts_ctx *ctx /* null: sizes only */, u64 n_, int g_, int mark_, const InvSegs *segs_ = nullptr) : n(n_), segs(segs_), g(g_), mark(mark_), ub(ctx)
    {
        u64 walker_cap = 524288;                                // lanes of the walk
        if (const char *e = ctx ? bwts_knob(ctx, "BWTS_WALKERS") : nullptr) { const long v = atol(e); if (v >= 256 && v <= (1 << 22)) walker_cap = (u64)v; }
        mom_shift = n > (1ull << 30) ? MOM_LOG2_LARGE : MOM_LOG2_SMALL; mom_classes = 1ull << mom_shift;      // residue classes, and their log2
        G = 1ull << g; s = (n + G - 1) / G; tiles = (n + LF_TILE - 1) / LF_TILE;
        // a segment longer than `slot` steps is cut into virtual nodes; room for s/8 of them (natural data needs ~2 %)
        slot = (u32)(4 * G < 16 ? 16 : 4 * G);
        node_cap = g == 0 ? s : s + s / 8 + 1024;
        l2cap = node_cap / L2_H + 2 + node_cap;                 // worst case: no node is reached by a level-2 walk
        wblocks = (unsigned)(((s < walker_cap ? s : walker_cap) + 255) / 256);
        log_chunks = n / (IDX_CHUNK - 64) + (u64)wblocks * 4 + 2;     // a closed chunk wastes < 64 entries; every wave may leave one open
        nbuckets = (u32)((n + (1ull << IDX_RANGE_LOG2) - 1) >> IDX_RANGE_LOG2);
        rep = inv_report_open(ctx, rep_spill);
        rep[IR_G] = (u64)g; rep[IR_MARK] = (u64)mark; rep[IR_S] = s; rep[IR_NODE_CAP] = node_cap; rep[IR_FORM] = segs ? IR_FORM_NARROW_SEGMENTED : IR_FORM_NARROW;
    }
    void declare(BlockLayout &L)            // the mark-specific buffers only for the mark that runs
    {
        lf.declare(L, n);
        if (mark == MARK_MOMENTS) mt.declare(L);
        if (mark == MARK_BYTEMAP) L.array(&marks, n);
        if (mark == MARK_LOG) lg.declare(L, log_chunks, nbuckets);
        nd.declare(L, node_cap, slot); l2.declare(L, l2cap); L.pad(INV_ARENA_SLACK);
    }
};
// bytes the narrow attempt (n, g, mark) reserves: no context, no device (bwts_debug_inverse_arena asks too)
size_t inverse_attempt_bytes(u64 n, int g, int mark) { InvRun r(nullptr, n, g, mark); BlockLayout L; r.declare(L); return L.bytes(); }
// What the host path's helper thread allocates before the transform runs: the default attempt at the closest splitter spacing the
// narrow form picks (g = 4, slot 64, moments) -- the node tables shrink faster with g than the records grow, so it bounds every g >= 4.
size_t inverse_arena_bytes(u64 n) { return inverse_attempt_bytes(n, 4, MARK_MOMENTS); }
__global__ __launch_bounds__(256) void seg_lf_shared_kernel(const u8 *__restrict__ B, const u64 *__restrict__ seg_off, u64 count, u64 run_base, u32 *__restrict__ LF);   // (with seg_lf_kernel, below)
// stable LF map (unbwts.c:50-52) and C; the byte map starts clear.  Over segments: the stable LF map of every segment, as indices of the run; no C
static int inv_build_lf(bwts_ctx *ctx, InvRun &r, const u8 *d_in)
{
    r.B = d_in;
    if (r.mark == MARK_BYTEMAP) HIPC(hipMemsetAsync(r.marks, 0, r.n, ctx->stream));
    SpanGuard sg(ctx, BWTS_K_LF_BUILD, r.n, 5 * r.n);
    if (r.segs) {
        seg_lf_shared_kernel<<<dim3((unsigned)((r.segs->count + 3) / 4)), dim3(256), 0, ctx->stream>>>(d_in, r.segs->off, r.segs->count, r.segs->base, r.lf.LF);
        return launched(ctx);
    }
    lf_hist_kernel<<<dim3((unsigned)r.tiles), dim3(LF_THREADS), 0, ctx->stream>>>(d_in, r.n, r.lf.tile_hist);
    BWTS_TRY(radix_column_scan(ctx, r.lf.tile_hist, r.tiles, r.lf.scan_temp));
    // the scanned table's first row is C itself: no separate histogram sweep, no host round trip before the walk
    ctab_from_tiles_kernel<<<dim3(1), dim3(64), 0, ctx->stream>>>(r.lf.tile_hist, r.n, d_in, r.dC);
    lf_rank_kernel<<<dim3((unsigned)r.tiles), dim3(LF_THREADS), 0, ctx->stream>>>(d_in, r.n, r.lf.tile_hist, r.lf.LF);
    return launched(ctx);
}
template <int MARK> static int launch_walk(bwts_ctx *ctx, const InvRun &r)
{
    constexpr bool mom = MARK == MARK_MOMENTS;
    if (r.segs) {
        if (mom) BWTS_TRY(ensure_dyn_lds(ctx, (const void *)walk_record_seg_kernel<MARK>, (size_t)MOM_MAX_BUCKETS * 20));
        walk_record_seg_kernel<MARK><<<dim3(r.wblocks), dim3(256), mom ? (size_t)r.mom_classes * 20 : 0, ctx->stream>>>(
            r.lf.LF, r.marks, r.lg.idxlog, r.s, r.node_cap, r.g, r.slot, r.B, r.nd.seg, r.nd.noderec, inv_counter(ctx, IC_TICKET), inv_counter(ctx, IC_VIRTUAL),
            inv_counter(ctx, IC_OVERFLOW), inv_counter(ctx, IC_LOG_CHUNKS), r.lg.chunk_fill, r.log_chunks, r.nbuckets, r.lg.bucket_seen, mom ? r.mom_shift : 0, r.mt.mom);
        return launched(ctx);
    }
    if (mom) BWTS_TRY(ensure_dyn_lds(ctx, (const void *)walk_record_kernel<MARK>, (size_t)MOM_MAX_BUCKETS * 20));
    walk_record_kernel<MARK><<<dim3(r.wblocks), dim3(256), mom ? (size_t)r.mom_classes * 20 : 0, ctx->stream>>>(
        r.lf.LF, r.marks, r.lg.idxlog, r.s, r.node_cap, r.g, r.slot, r.dC, r.nd.seg, r.nd.noderec, inv_counter(ctx, IC_TICKET), inv_counter(ctx, IC_VIRTUAL),
        inv_counter(ctx, IC_OVERFLOW), inv_counter(ctx, IC_LOG_CHUNKS), r.lg.chunk_fill, r.log_chunks, r.nbuckets, r.lg.bucket_seen, mom ? r.mom_shift : 0, r.mt.mom);
    return launched(ctx);
}
// the walk: marks, segment symbols, reduced list.  Virtual nodes join the reduced list: its size is only known afterwards.
static int inv_walk(bwts_ctx *ctx, InvRun &r, InvOutcome *out)
{
    HIPC(hipMemsetAsync(inv_counter(ctx, 0), 0, IC_WORDS * sizeof(u64), ctx->stream));
    if (r.mark == MARK_LOG) {
        HIPC(hipMemsetAsync(r.lg.chunk_fill, 0, r.log_chunks * sizeof(u32), ctx->stream));
        HIPC(hipMemsetAsync(r.lg.bucket_seen, 0, IDX_MAX_BUCKETS * sizeof(u32), ctx->stream));
    }
    if (r.mark == MARK_MOMENTS) HIPC(hipMemsetAsync(r.mt.mom, 0, 3 * r.mom_classes * sizeof(u64), ctx->stream));
    {
        SpanGuard sg(ctx, BWTS_K_WALK, r.n, 6 * r.n);
        int (*const launch[4])(bwts_ctx *, const InvRun &) = {launch_walk<MARK_LOG>, launch_walk<MARK_SENTINEL>, launch_walk<MARK_BYTEMAP>, launch_walk<MARK_MOMENTS>};
        BWTS_TRY(launch[r.mark](ctx, r));
    }
    BWTS_TRY(read_small(ctx, SMI_COUNTERS, IC_WORDS));
    r.rep[IR_VIRTUAL] = inv_count(ctx, IC_VIRTUAL);
    if (inv_count(ctx, IC_OVERFLOW)) { *out = INV_RETRY_DENSE; return BWTS_OK; }   // node pool exhausted (adversarial LF): plain pointer jumping
    r.s_all = r.s + inv_count(ctx, IC_VIRTUAL); r.s2 = (r.s_all + L2_H - 1) / L2_H;
    return BWTS_OK;
}
static int inv_collect(bwts_ctx *ctx, InvRun &r, bool first_time)
{
    SpanGuard sg(ctx, BWTS_K_OTHER, r.n, 4 * r.n);
    unsigned long long *ctr = inv_counter(ctx, 0), *found = inv_counter(ctx, IC_UNREACHED);
    u32 *LF = r.lf.LF; u64 blocks = (r.n + 255) / 256; if (blocks > 8192) blocks = 8192;
    if (r.mark == MARK_MOMENTS) {
        if (!first_time) HIPC(hipMemsetAsync(inv_counter(ctx, IC_LISTED_CLASSES), 0, 2 * sizeof(u64), ctx->stream));    // ... and IC_MOM_FALLBACK
        const u64 per_class = (r.n + r.mom_classes - 1) >> r.mom_shift;
        const u64 budget = (4ull << 20) > per_class ? (4ull << 20) : per_class;        // elements the search may look at (at least one class)
        HIPC(hipMemcpyAsync(r.mt.work, r.mt.mom, 3 * r.mom_classes * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream));
        moments_resolve_kernel<<<dim3(1), dim3(1024), 0, ctx->stream>>>(r.mt.work, r.mt.cstat, r.n, r.mom_shift, LF, r.uidx, r.ulf, r.ucap, r.mt.def_list, ctr, 1u << 16);
        moments_budget_kernel<<<dim3(1), dim3(64), 0, ctx->stream>>>(ctr, per_class, budget);
        moments_chase_kernel<<<dim3(2048), dim3(256), 0, ctx->stream>>>(r.mt.def_list, ctr, r.n, r.mom_shift, r.g, LF, 1u << 16, r.uidx, r.ulf, r.ucap, ctr, r.mt.cstat);
    } else if (r.mark == MARK_LOG) {
        const int bm_bytes = (int)((1u << IDX_RANGE_LOG2) / 8);
        if (first_time) {
            HIPC(hipMemsetAsync(r.lg.bucket_fill, 0, (size_t)r.nbuckets * IDX_FILL_STRIDE * sizeof(u32), ctx->stream));
            BWTS_TRY(ensure_dyn_lds(ctx, (const void *)unvisited_from_buckets_kernel, (size_t)bm_bytes));
            BWTS_TRY(ensure_dyn_lds(ctx, (const void *)bucket_indices_kernel, bucket_indices_lds_bytes(IDX_MAX_BUCKETS)));
            bucket_deficit_kernel<<<dim3((r.nbuckets + 255) / 256), dim3(256), 0, ctx->stream>>>(r.lg.bucket_seen, r.nbuckets, r.n, r.lg.deficient());
            bucket_indices_kernel<<<dim3((unsigned)r.log_chunks), dim3(IDX_THREADS), bucket_indices_lds_bytes(r.nbuckets), ctx->stream>>>(
                r.lg.idxlog, r.lg.chunk_fill, r.nbuckets, r.lg.deficient(), r.lg.bucket_fill, r.lg.bucket_data);
        }
        unvisited_from_buckets_kernel<<<dim3(r.nbuckets), dim3(1024), bm_bytes, ctx->stream>>>(r.lg.deficient(), r.lg.bucket_fill, r.lg.bucket_data, LF, r.n, r.uidx, r.ulf,
                                                                                              r.ucap, found);
    } else if (r.mark == MARK_BYTEMAP)
        collect_unvisited_kernel<MARK_BYTEMAP><<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(LF, r.marks, r.n, r.uidx, r.ulf, r.ucap, found);
    else
        collect_unvisited_kernel<MARK_SENTINEL><<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(LF, r.marks, r.n, r.uidx, r.ulf, r.ucap, found);
    return launched(ctx);
}
// Elements in cycles without a splitter, in lists sized by their number: count first, and where the first room was too small lay the lists out
// again and collect again.  The level-2 walk over the node list is queued in between: one read-back brings both counts (elements, nodes).
static int inv_find_unreached(bwts_ctx *ctx, InvRun &r, InvOutcome *out)
{
    const size_t ucap = ctx->unv_hint > UNV_CAP0 ? ctx->unv_hint : UNV_CAP0;
    BWTS_TRY(lay_out_unreached(ctx, r, ucap > r.n ? (size_t)r.n : ucap, 0, &r.tiny, &r.end_of_tiny));
    BWTS_TRY(inv_collect(ctx, r, true));
    r.rep[IR_UCAP_FIRST] = r.ucap;
    {
        SpanGuard sg(ctx, BWTS_K_LISTRANK, r.s_all, 32 * r.s_all);
        HIPC(hipMemsetAsync(r.nd.visited2, 0, r.s_all, ctx->stream));
        lr2_walk_kernel<<<dim3(grid1(r.s2)), dim3(256), 0, ctx->stream>>>(r.nd.noderec, r.s2, r.nd.visited2, r.l2.rec2);
        lr2_collect_kernel<<<dim3(grid1(r.s_all)), dim3(256), 0, ctx->stream>>>(r.nd.visited2, r.s_all, r.s2, r.nd.U, r.nd.id2of, inv_counter(ctx, IC_UNREACHED_NODES));
        HIPC(hipGetLastError());
    }
    BWTS_TRY(read_small(ctx, SMI_COUNTERS, IC_WORDS));
    r.nu = inv_count(ctx, IC_UNREACHED); r.nu2 = inv_count(ctx, IC_UNREACHED_NODES);
    r.rep[IR_NU] = r.nu; r.rep[IR_NU2] = r.nu2; r.rep[IR_LISTED] = inv_count(ctx, IC_LISTED_CLASSES); r.rep[IR_MOM_FALLBACK] = inv_count(ctx, IC_MOM_FALLBACK);
    const bool inv_trace = [ctx] { const char *e = bwts_knob(ctx, "BWTS_INV_TRACE"); return e && atoi(e) == 1; }();
    if (inv_trace && r.mark == MARK_MOMENTS)
        fprintf(stderr, "[inverse] moments: shift %d, unreached found %llu, ranges searched %llu, fallback flag %llu\n", r.mom_shift, (unsigned long long)r.nu,
                (unsigned long long)inv_count(ctx, IC_LISTED_CLASSES), (unsigned long long)inv_count(ctx, IC_MOM_FALLBACK));
    if (r.mark == MARK_MOMENTS && inv_count(ctx, IC_MOM_FALLBACK)) { *out = INV_NEED_LOG; return BWTS_OK; }
    ctx->tm.unvisited = r.nu;
    if (r.nu > r.n || r.nu2 > r.s_all) return BWTS_E_INTERNAL;
    ctx->unv_hint = (size_t)r.nu;
    if (r.nu > r.ucap) {
        BWTS_TRY(lay_out_unreached(ctx, r, r.nu, 0, &r.tiny, &r.end_of_tiny));
        HIPC(hipMemsetAsync(inv_counter(ctx, IC_UNREACHED), 0, sizeof(u64), ctx->stream));
        BWTS_TRY(inv_collect(ctx, r, false));
        r.rep[IR_SECOND_COLLECT] = 1;
    }
    r.s2all = r.s2 + r.nu2;
    return BWTS_OK;
}
// level-2 list ranking by pointer jumping; cycle records of the reduced list
static int inv_rank_node_list(bwts_ctx *ctx, InvRun &r)
{
    SpanGuard sg(ctx, BWTS_K_LISTRANK, r.s2all, 0);
    const int R = bit_length(r.s2all), gb = grid1(r.s2all);      // 2^R > s2all >= any cycle's entry count
    Level2Tables &t = r.l2;
    if (r.nu2) lr2_fill_kernel<<<dim3(grid1(r.nu2)), dim3(256), 0, ctx->stream>>>(r.nd.U, r.nu2, r.s2, r.nd.noderec, r.nd.id2of, t.rec2);
    lr_init_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.s2all, t.rec2, t.lrmin[0]);
    for (int i = 0; i < R; i++, r.cur ^= 1) lr_jump_min_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.s2all, t.lrmin[r.cur], t.lrmin[r.cur ^ 1]);
    lr_cut_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.s2all, t.rec2, t.lrmin[r.cur], t.lrsum[0]);
    for (int i = 0; i < R; i++, r.sc ^= 1) lr_jump_sum_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.s2all, t.lrsum[r.sc], t.lrsum[r.sc ^ 1]);
    lr_finish_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.s2all, t.lrmin[r.cur], t.lrsum[r.sc], t.rec2, t.dist, t.min_dist, t.recs2, inv_counter(ctx, IC_LIST_CYCLES));
    return launched(ctx);
}
// cycles without a splitter: one lane per unreached element follows its cycle; where one is too long for that, the unit-node ranking
static int inv_free_cycles(bwts_ctx *ctx, InvRun &r, InvOutcome *out)
{
    if (r.nu) {
        SpanGuard sg(ctx, BWTS_K_OTHER, r.nu, 8 * r.nu);
        tiny_cycle_scan_kernel<<<dim3(grid1(r.nu)), dim3(256), 0, ctx->stream>>>(r.uidx, r.ulf, r.nu, r.lf.LF, one_lane_cap(r.nu, r.G), r.tiny, inv_counter(ctx, IC_FREE_CYCLES),
                                                                                inv_counter(ctx, IC_OVERFLOW));
        HIPC(hipGetLastError());
    }
    BWTS_TRY(read_small(ctx, SMI_COUNTERS, IC_WORDS));
    r.kc = inv_count(ctx, IC_LIST_CYCLES); r.kt = inv_count(ctx, IC_FREE_CYCLES);
    r.rep[IR_KC] = r.kc; r.rep[IR_KT] = r.kt;
    if (r.kc == 0 || r.kc > r.s2all || r.kt > r.nu) return BWTS_E_INTERNAL;
    r.unit_rank = inv_count(ctx, IC_OVERFLOW) != 0;
    r.rep[IR_UNIT_RANK] = r.unit_rank;
    if (!r.unit_rank) return BWTS_OK;
    // A cycle without a splitter too long for one lane (sorted or periodic data: 1^b 0^c with n = 2^k, c = 2 * odd has a cycle of
    // n / 2 odd elements): every unreached element becomes a node of one symbol and the pointer-jumping kernels of the 64-bit
    // form rank that list -- memory and work by the number of unreached elements, not by n (wide_inverse.h).
    if (r.nu >= 0x7ffffff0ull) { *out = INV_RETRY_DENSE; return BWTS_OK; }
    SpanGuard sg(ctx, BWTS_K_LISTRANK, r.nu, 0);
    BlockLayout L; r.unit.declare(L, r.nu); L.array(&r.uend, r.nu); L.array(&r.uleader, r.nu);
    if (r.ub.take(L.bytes()) != BWTS_OK) { *out = INV_RETRY_DENSE; return BWTS_OK; }      // 112 bytes per unreached element
    L.place(r.ub.p);
    const int gb = grid1(r.nu);
    HIPC(hipMemsetAsync(inv_counter(ctx, IC_UNIT_CYCLES), 0, sizeof(u64), ctx->stream));
    wi_unit_index_kernel<u32><<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.uidx, r.nu, r.lf.LF);        // LF[x] of an unreached x lives on in ulf
    wi_unit_nodes_kernel<u32><<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.uidx, r.ulf, r.nu, r.lf.LF, r.unit.nodes);
    wi_rank_nodes(ctx, r.nu, r.unit.nodes, r.unit.rk);
    unit_finish_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.nu, r.unit.rk.min_of(), r.unit.rk.sum_of(), r.unit.nodes, r.unit.dist, r.unit.min_dist, r.tiny, r.uleader,
                                                               inv_counter(ctx, IC_UNIT_CYCLES));
    HIPC(hipGetLastError());
    BWTS_TRY(read_small(ctx, SMI_COUNTERS + IC_UNIT_CYCLES, 1));
    r.kt = inv_count(ctx, IC_UNIT_CYCLES);              // these cycles take the place of the one-lane scan's
    r.rep[IR_KT] = r.kt;
    return r.kt == 0 || r.kt > r.nu ? BWTS_E_INTERNAL : BWTS_OK;
}
// order the cycles by smallest element on the device: sort (minelem, record), prefix sums of the lengths; then every node's place
static int inv_order_cycles(bwts_ctx *ctx, InvRun &r)
{
    const u64 kall = r.kc + r.kt;
    ctx->tm.factors = kall;
    SpanGuard sg(ctx, BWTS_K_LISTRANK, kall, 0);
    const CycleList cl{r.tiny, r.kt, r.l2.recs2, r.kc};
    SortPlan cp;
    BWTS_TRY(cycle_sort_plan(ctx, kall, &cp));
    cycle_keys_kernel<<<dim3(grid1(kall)), dim3(256), 0, ctx->stream>>>(cl, cp.keys[0], cp.vals[0]);
    int res = 0, kbits = bit_length(r.n - 1);
    BWTS_TRY(radix_sort_pairs(ctx, cp, kall, kbits < 1 ? 1 : kbits, &res));
    CycleLenIn lin{cl, cp.vals[res]};
    u64 *total = ctx->d_small + SMI_COUNTERS + IC_LENGTH_SUM;
    if (r.segs) {
        SegCycleEndOut lout{cl, cp.vals[res], r.segs->off, r.segs->count, r.segs->base, r.l2.end_by_leader, r.end_of_tiny, total};
        BWTS_TRY((device_scan<false, u32>(ctx, kall, lin, lout, OpAdd(), 0u, cp.scan_temp)));
    } else {
        CycleEndOut lout{cl, cp.vals[res], (u32)(r.n - 1), r.l2.end_by_leader, r.end_of_tiny, total};
        BWTS_TRY((device_scan<false, u32>(ctx, kall, lin, lout, OpAdd(), 0u, cp.scan_temp)));
    }
    if (r.unit_rank) unit_ends_kernel<<<dim3(grid1(r.kt)), dim3(256), 0, ctx->stream>>>(r.uleader, r.end_of_tiny, r.kt, r.uend);
    lr_place2_kernel<<<dim3(grid1(r.s2all)), dim3(256), 0, ctx->stream>>>(r.s2all, r.l2.lrmin[r.cur], r.l2.lrsum[r.sc], r.l2.dist, r.l2.min_dist, r.l2.end_by_leader, r.l2.place2);
    lr2_distribute_kernel<<<dim3(grid1(r.s2all)), dim3(256), 0, ctx->stream>>>(r.nd.noderec, r.s2, r.s2all, r.nd.U, r.l2.place2, r.nd.opos, r.nd.wrap, r.nd.clen);
    return launched(ctx);
}
// the recorded segments go to their places in the text (unbwts.c:73-82); the sum of the cycle lengths says whether every element was placed
static int inv_place(bwts_ctx *ctx, InvRun &r, u8 *d_out, InvOutcome *out)
{
    {
        SpanGuard sg(ctx, BWTS_K_WALK_EMIT, r.n, 2 * r.n);
        const int tpn_log2 = r.g < 4 ? 0 : r.g > 12 ? 8 : r.g - 4;      // one 16-symbol chunk per thread at the expected segment length (G)
        const u64 threads = r.s_all << tpn_log2;
        place_segments_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream>>>(r.nd.seg, r.s_all, r.slot, tpn_log2, r.nd.noderec, r.nd.opos, r.nd.wrap,
                                                                                                      r.nd.clen, d_out);
        if (r.unit_rank && r.segs)
            wi_unit_place_seg_kernel<u32><<<dim3(grid1(r.nu)), dim3(256), 0, ctx->stream>>>(r.nu, r.unit.rk.min_of(), r.unit.rk.sum_of(), r.unit.dist, r.unit.min_dist, r.uend,
                                                                                            r.uidx, r.B, d_out);
        else if (r.unit_rank)
            wi_unit_place_kernel<u32><<<dim3(grid1(r.nu)), dim3(256), 0, ctx->stream>>>(r.nu, r.unit.rk.min_of(), r.unit.rk.sum_of(), r.unit.dist, r.unit.min_dist, r.uend, r.ulf,
                                                                                        r.dC, d_out);
        else if (r.kt && r.segs) tiny_place_seg_kernel<<<dim3(grid1(r.kt)), dim3(256), 0, ctx->stream>>>(r.tiny, r.kt, r.end_of_tiny, r.lf.LF, r.B, d_out);
        else if (r.kt) tiny_place_kernel<<<dim3(grid1(r.kt)), dim3(256), 0, ctx->stream>>>(r.tiny, r.kt, r.end_of_tiny, r.lf.LF, r.dC, d_out);
        HIPC(hipGetLastError());
    }
    BWTS_TRY(read_small(ctx, SMI_COUNTERS + IC_LENGTH_SUM, 1));
    if ((u32)inv_count(ctx, IC_LENGTH_SUM) == (u32)r.n) return BWTS_OK;
    // n = 2^32 only: the one entry whose value equals LF_VISITED sat in a cycle without a splitter and was taken for visited
    if (r.mark == MARK_SENTINEL && r.n == 0x100000000ull) { *out = INV_AMBIGUOUS; return BWTS_OK; }
    return BWTS_E_INTERNAL;
}
// One attempt with splitter spacing 2^g: the stages in order; one that sets *out to anything but INV_DONE ends the attempt there.
static int inverse_stages(bwts_ctx *ctx, InvRun &r, const u8 *d_in, u8 *d_out, InvOutcome *out)
{
    BWTS_TRY(arena_place(ctx, r));
    BWTS_TRY(inv_build_lf(ctx, r, d_in));
    BWTS_TRY(inv_walk(ctx, r, out));
    if (*out != INV_DONE) return BWTS_OK;
    BWTS_TRY(inv_find_unreached(ctx, r, out));
    if (*out != INV_DONE) return BWTS_OK;
    BWTS_TRY(inv_rank_node_list(ctx, r));
    BWTS_TRY(inv_free_cycles(ctx, r, out));
    if (*out != INV_DONE) return BWTS_OK;
    BWTS_TRY(inv_order_cycles(ctx, r));
    return inv_place(ctx, r, d_out, out);
}
static int inverse_attempt(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, int g, int mark, const InvSegs *segs, InvOutcome *out)
{
    InvRun r(ctx, n, g, mark, segs);
    *out = INV_DONE;
    BWTS_TRY(inverse_stages(ctx, r, d_in, d_out, out));
    r.rep[IR_OUTCOME] = (u64)*out;
    return BWTS_OK;
}

// The narrow form's chain of attempts over [0, n), n <= 2^32: one BWT (segs null), or the shared pass over a run of segments.  The caller
// has set tm.attempts = 1 and cleared the attempt records.
static int inverse_narrow_chain(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, const InvSegs *segs)
{
    // how the unreached elements are found: per-class moments (default), the index log, or the two mark forms
    // (BWTS_INV_MARK=log|sentinel|bytemap, BWTS_BYTEMARK=1: tests, and the fallback chain below)
    // (A shared pass over many segments starts with the index log: every segment of a transform ends in short Lyndon factors, about 15
    // unreached elements each, and beyond a few thousand of them the moments' classes all miss more than the arithmetic names.  Measured,
    // profiles/segments_shared_inverse_1gib.txt: with the moments first, passes over 8 .. 128 segments of 64 KiB and of 1 MiB took one
    // attempt, 256 x 1 MiB and every 1 GiB set (1 024 to 262 144 segments) ran the walk twice.)
    int mark = segs && segs->count > SEG_MOMENTS_MAX_SEGMENTS ? MARK_LOG : MARK_MOMENTS;
    const char *me = bwts_knob(ctx, "BWTS_INV_MARK");
    if (me && !strcmp(me, "moments")) mark = MARK_MOMENTS;
    if (me && !strcmp(me, "log")) mark = MARK_LOG;
    if (me && !strcmp(me, "sentinel")) mark = MARK_SENTINEL;
    if ((me && !strcmp(me, "bytemap")) || bwts_knob(ctx, "BWTS_BYTEMARK")) mark = MARK_BYTEMAP;
    // The fallback chain: every outcome but INV_DONE names the next (g, mark).  Worst case the walk runs five times (moments -> index
    // log -> byte map at n = 2^32 -> every element a splitter, with sentinel and then byte-map marks); natural inputs take one.
    // bwts_timings.attempts says how many it was.
    int g = splitter_log2(ctx, n);
    bool dense = false;
    for (;; ctx->tm.attempts++) {
        InvOutcome out;
        BWTS_TRY(inverse_attempt(ctx, d_in, n, d_out, g, mark, segs, &out));
        if (out == INV_DONE) return BWTS_OK;
        if (out == INV_NEED_LOG) mark = MARK_LOG;           // many unreached elements (low-entropy input): the walk again, logging every index it visits
        else if (out == INV_AMBIGUOUS) mark = MARK_BYTEMAP; // sentinel marks only
        else {                                              // INV_RETRY_DENSE, once: on the simplest marks
            if (dense) return BWTS_E_INTERNAL;
            dense = true; g = 0;
            if (mark == MARK_LOG || mark == MARK_MOMENTS) mark = MARK_SENTINEL;
        }
    }
}

int inverse_device_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out)
{
    // beyond 32-bit indices: the 64-bit form (wide_inverse.h); BWTS_FORCE_WIDE sends every input there (tests)
    const int force_wide = [ctx] { const char *e = bwts_knob(ctx, "BWTS_FORCE_WIDE"); return e ? atoi(e) : 0; }();
    ctx->tm.attempts = 1;
    ctx->inv_attempts_made = 0;
    if (n > 0x80000000ull) {
        // one byte value only: LF is the identity, n cycles of one element, the text is the input (unbwts.c:66-86 walks each of them
        // in one step).  The general route holds ~110 bytes per element of cycles that meet no splitter -- all of them here --, which
        // beyond 2^31 elements no device has; so large inputs are looked at first (eight probes, then the histogram only if they agree).
        bool constant = false;
        BWTS_TRY(constant_input_probe(ctx, d_in, n, &constant));
        if (constant) {
            HIPC(hipMemcpyAsync(d_out, d_in, n, hipMemcpyDefault, ctx->stream));
            ctx->tm.factors = n; ctx->tm.unvisited = 0;
            return BWTS_OK;
        }
    }
    if (n > 0x100000000ull || force_wide) return inverse_wide_impl(ctx, d_in, n, d_out);
    return inverse_narrow_chain(ctx, d_in, n, d_out, nullptr);
}

// ------------------------------------------------------------------------------------
// independent segments (bwts_inverse_segments)
// ------------------------------------------------------------------------------------
// LF per segment: LF[i] = C_s[B[i]] + (occurrences of B[i] in segment s before i), as an index local to the segment.  One wave per
// segment: byte histogram in LDS, exclusive scan, then 64 positions per step in order -- a lane's rank among the lanes holding the same
// byte comes from eight ballots, and the last such lane advances the byte's counter.
#define SEG_INV_VISITED 0xffffffffu
// one wave, one segment S[0 .. L): LFseg[p] = add + C[S[p]] + occ(S[p], p); cnt: the wave's 256 counters in LDS
__device__ __forceinline__ void seg_lf_wave(const u8 *__restrict__ S, u64 L, u32 add, u32 *__restrict__ LFseg, u32 *cnt)
{
    const int lane = lane_id();
    for (int c = lane; c < 256; c += 64) cnt[c] = 0;
    __builtin_amdgcn_wave_barrier();
    for (u64 p = (u64)lane; p < L; p += 64) atomicAdd(&cnt[S[p]], 1u);
    // the counters are this wave's alone and a wave's LDS operations complete in order; the barriers keep the compiler from moving
    // one phase's accesses across the next's
    __builtin_amdgcn_wave_barrier();
    {
        const u32 v0 = cnt[4 * lane], v1 = cnt[4 * lane + 1], v2 = cnt[4 * lane + 2], v3 = cnt[4 * lane + 3];
        const u32 sum = v0 + v1 + v2 + v3;
        const u32 ex = wave_scan_inclusive(sum, OpAdd()) - sum;
        cnt[4 * lane] = ex; cnt[4 * lane + 1] = ex + v0; cnt[4 * lane + 2] = ex + v0 + v1; cnt[4 * lane + 3] = ex + v0 + v1 + v2;
    }
    __builtin_amdgcn_wave_barrier();
    // (the steps are serial -- a step's ranks start from the counters the one before left -- but their bytes are not: four steps' loads
    // are in flight together, else every step waits out a memory round trip: 0.8 us a step at 1 MiB segments)
    for (u64 q0 = 0; q0 < L; q0 += 256) {
        u32 bs[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { const u64 p = q0 + 64 * k + (u64)lane; bs[k] = p < L ? (u32)S[p] : 0u; }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const u64 p = q0 + 64 * k + (u64)lane;
            const bool act = p < L;
            const u32 b = bs[k];
            u64 match = __ballot(act);
#pragma unroll
            for (int bit = 0; bit < 8; bit++) {
                const u64 ones = __ballot((b >> bit) & 1u);
                match &= ((b >> bit) & 1u) ? ones : ~ones;
            }
            if (act) {
                const u32 at = cnt[b];
                LFseg[p] = add + at + (u32)__popcll(match & lanemask_lt());
                if ((match >> lane) == 1ull) cnt[b] = at + (u32)__popcll(match);      // the group's last lane
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}
__global__ __launch_bounds__(256) void seg_lf_kernel(const u8 *__restrict__ B, const u64 *__restrict__ seg_off, u64 count, u64 big, u32 *__restrict__ LF)
{
    __shared__ u32 cnt_all[4][256];
    const u64 s = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= count) return;
    const u64 base = seg_off[s], L = seg_off[s + 1] - base;
    if (L >= big) return;
    seg_lf_wave(B + base, L, 0u, LF + base, cnt_all[threadIdx.x >> 6]);
}
// The shared pass's LF: the same per segment, as indices of the run -- a permutation of the run's [0, n) whose cycles each lie inside one
// segment.  seg_off: the run's slice of the offset table (absolute offsets, seg_off[0] = run_base); B and LF start at the run.
__global__ __launch_bounds__(256) void seg_lf_shared_kernel(const u8 *__restrict__ B, const u64 *__restrict__ seg_off, u64 count, u64 run_base, u32 *__restrict__ LF)
{
    __shared__ u32 cnt_all[4][256];
    const u64 s = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= count) return;
    const u64 base = seg_off[s] - run_base, L = seg_off[s + 1] - seg_off[s];
    seg_lf_wave(B + base, L, (u32)base, LF + base, cnt_all[threadIdx.x >> 6]);
}

// The cycle walk of unbwts.c:62-86 inside one segment, one lane per segment: cycles by smallest index, each written from the end of
// what is left of the segment backwards.
__global__ __launch_bounds__(64) void seg_walk_kernel(const u8 *__restrict__ B, u32 *__restrict__ LF, const u64 *__restrict__ seg_off, u64 count, u64 big,
                                                       u8 *__restrict__ out, unsigned long long *__restrict__ cycles)
{
    const u64 s = (u64)blockIdx.x * 64 + threadIdx.x;       // one wave per workgroup: the chains spread over every CU
    u64 ncyc = 0;
    if (s < count) {
        const u64 base = seg_off[s], L = seg_off[s + 1] - base;
        if (L < big) {
            u32 *lf = LF + base;
            const u8 *b = B + base;
            u8 *o = out + base;
            u64 pos = L;
            u32 start = 0;
            while (pos > 0) {
                while (start < L && lf[start] == SEG_INV_VISITED) start++;
                if (start >= L) break;
                u32 x = start;
                do {
                    const u32 nx = lf[x];
                    o[--pos] = b[x];
                    lf[x] = SEG_INV_VISITED;
                    x = nx;
                } while (x != start && pos > 0);
                ncyc++;
            }
        }
    }
    if (ncyc) atomicAdd(cycles, (unsigned long long)ncyc);
}

// measured on 1 GiB (profiles/segments_1gib_zipf_text.txt): one step of a walk with 16 384 chains in flight ~5.3 us; 262 144 chains of
// 4 KiB: 12 G steps/s; a single-input inverse of 64 KiB ~0.3 ms
#define SEG_WALK_STEP_US 5.0
#define SEG_WALK_STEPS_PER_US 12000.0
#define SEG_CALL_US 300.0
// the shared pass (plan B), measured (profiles/segments_shared_inverse_1gib.txt): a pass of two 100 000-byte segments takes 0.9 ms, 0.5 of
// them in the LF builder; 1 GiB goes at 19 000 bytes/us (55 .. 59 ms for segments of 4 KiB .. 1 MiB), 64 MiB at 14 000 -- the lower rate is
// the one used, so that the lane walk keeps the sets where the two plans are close; the LF builder gives a segment one wave, 64 positions
// a step, so the longest segment of a run adds its steps (1 MiB: 16 384 steps, 10.2 - 3.1 ms); and every segment leaves about min(length,
// 15) elements that no walk reaches, 0.5 .. 0.9 ns each through the index log and the second collection (64 MiB of 8 .. 256-byte segments:
// 48.8 .. 7.2 ms, where the lane walk takes 31.3 .. 4.9).  A single call's bytes go at the whole-input rate (1 GiB in 32.6 ms).
#define SEG_SHARED_PASS_US 400.0
#define SEG_SHARED_BYTES_PER_US 14000.0
#define SEG_SHARED_UNREACHED_PER_US 1400.0
#define SEG_SHARED_UNREACHED_PER_SEGMENT 16
#define SEG_SHARED_LF_STEP_US 0.45
#define SEG_SINGLE_BYTES_PER_US 33000.0
static int length_bits(u64 len) { int b = 0; for (u64 x = len; x; x >>= 1) b++; return b; }          // len < 2^b
// Plan A: the power of two `big` that minimises (lane walk of the segments below it) + (a single call for each of the others)
static u64 seg_inverse_threshold(const std::vector<u64> &off, double *cost_out = nullptr)
{
    const u64 count = (u64)off.size() - 1;
    u64 cnt[66] = {0}, bytes[66] = {0}, maxlen[66] = {0};
    for (u64 s = 0; s < count; s++) {
        const u64 len = off[s + 1] - off[s];
        const int b = length_bits(len);
        cnt[b]++; bytes[b] += len; if (len > maxlen[b]) maxlen[b] = len;
    }
    // threshold 2^b: segments with len < 2^b walk, the rest are single calls
    double best = 1e300;
    int best_b = 65;
    u64 small_bytes = 0, small_max = 0, calls = count;
    for (int b = 0; b <= 65; b++) {
        if (b > 0) { small_bytes += bytes[b]; if (maxlen[b] > small_max) small_max = maxlen[b]; calls -= cnt[b]; }
        double walk = 0;
        if (small_bytes) {
            walk = (double)small_max * SEG_WALK_STEP_US;
            const double thr = (double)small_bytes / SEG_WALK_STEPS_PER_US;
            if (thr > walk) walk = thr;
        }
        const double cost = walk + (double)calls * SEG_CALL_US;
        if (cost < best) { best = cost; best_b = b; }
    }
    if (cost_out) {
        // (for the comparison with plan B, which counts them: the single calls' bytes)
        u64 single_bytes = 0;
        for (int b = best_b + 1; b <= 65; b++) single_bytes += bytes[b];
        *cost_out = best + (double)single_bytes / SEG_SINGLE_BYTES_PER_US;
    }
    return best_b >= 64 ? ~0ull : 1ull << best_b;
}
// Plan B: the power of two `big` that minimises (one shared pass per maximal run of segments below it) + (a single call for each of the others)
static u64 seg_shared_threshold(const std::vector<u64> &off, double *cost_out)
{
    const u64 count = (u64)off.size() - 1;
    u64 cnt[67] = {0}, bytes[67] = {0}, maxlen[67] = {0}, unreached[67] = {0};     // unreached: the estimate, min(length, 16) a segment
    long long run_starts[67] = {0};          // difference array over b: segment s starts a run at threshold 2^b for bits(s) <= b < bits(s - 1)
    int prev = 66;
    for (u64 s = 0; s < count; s++) {
        const u64 len = off[s + 1] - off[s];
        const int b = length_bits(len);
        cnt[b]++; bytes[b] += len; if (len > maxlen[b]) maxlen[b] = len;
        unreached[b] += len < SEG_SHARED_UNREACHED_PER_SEGMENT ? len : SEG_SHARED_UNREACHED_PER_SEGMENT;
        if (b < prev) { run_starts[b]++; run_starts[prev]--; }
        prev = b;
    }
    double best = 1e300;
    int best_b = 65;
    u64 shared_bytes = 0, shared_unreached = 0, shared_max = 0, calls = count, single_bytes = off[count];
    long long runs = 0;
    for (int b = 0; b <= 65; b++) {
        runs += run_starts[b];
        if (b > 0) {
            shared_bytes += bytes[b]; single_bytes -= bytes[b]; calls -= cnt[b];
            shared_unreached += unreached[b];
            if (maxlen[b] > shared_max) shared_max = maxlen[b];
        }
        const double cost = (double)runs * SEG_SHARED_PASS_US + (double)shared_bytes / SEG_SHARED_BYTES_PER_US + (double)shared_unreached / SEG_SHARED_UNREACHED_PER_US +
                            (double)((shared_max + 63) / 64) * SEG_SHARED_LF_STEP_US + (double)calls * SEG_CALL_US + (double)single_bytes / SEG_SINGLE_BYTES_PER_US;
        if (cost < best) { best = cost; best_b = b; }
    }
    *cost_out = best;
    return best_b >= 64 ? ~0ull : 1ull << best_b;
}

// What a segmented inverse does with a set of segments.  Plan A (SEG_PLAN_LANE): segments below `big` are walked one lane each, in one
// pass over the call.  Plan B (SEG_PLAN_SHARED): every maximal run of consecutive segments below `big` goes through one shared pass of
// the splitter walk.  In both the segments of `big` bytes or more take a single-input call each.
enum { SEG_PLAN_LANE = 0, SEG_PLAN_SHARED = 1, SEG_PLAN_SHARED_NOMEM = 2 /* (reports only) plan B refused for memory: plan A ran */ };
struct SegInvPlan { int plan; u64 big, runs, own_segs, own_bytes, single_segs, single_bytes, longest_run, longest_run_segs; };
// the routes of the set under (plan, big)
static SegInvPlan seg_plan_routes(const std::vector<u64> &off, int plan, u64 big)
{
    SegInvPlan p = {plan, big, 0, 0, 0, 0, 0, 0, 0};
    const u64 count = (u64)off.size() - 1;
    u64 run = 0, run_segs = 0;
    for (u64 s = 0; s < count; s++) {
        const u64 len = off[s + 1] - off[s];
        if (len >= big) { p.single_segs++; p.single_bytes += len; run = run_segs = 0; continue; }
        if (run == 0) p.runs++;
        run += len; run_segs++; p.own_segs++; p.own_bytes += len;
        if (run > p.longest_run) { p.longest_run = run; p.longest_run_segs = run_segs; }
    }
    if (plan == SEG_PLAN_LANE) p.runs = p.own_segs ? 1 : 0;            // one lane walk over the whole call
    return p;
}
// force_plan: -1 the cost estimate chooses, else the plan; force_big: 0 the plan's own threshold, else `big`
static SegInvPlan seg_inverse_plan(const std::vector<u64> &off, int force_plan, u64 force_big)
{
    double cost_a = 0, cost_b = 0;
    const u64 big_a = seg_inverse_threshold(off, &cost_a), big_b = seg_shared_threshold(off, &cost_b);
    const int plan = force_plan >= 0 ? force_plan : cost_b < cost_a ? SEG_PLAN_SHARED : SEG_PLAN_LANE;
    return seg_plan_routes(off, plan, force_big ? force_big : plan == SEG_PLAN_SHARED ? big_b : big_a);
}
// ... with the context's test switches: BWTS_SEG_INV_PLAN=lane|shared forces the plan, BWTS_SEG_INV_BIG sets `big` (1 = every segment alone)
static SegInvPlan seg_inverse_plan(const bwts_ctx *ctx)
{
    int force_plan = -1; u64 force_big = 0;
    if (const char *e = bwts_knob(ctx, "BWTS_SEG_INV_PLAN")) force_plan = !strcmp(e, "shared") ? SEG_PLAN_SHARED : !strcmp(e, "lane") ? SEG_PLAN_LANE : -1;
    if (const char *e = bwts_knob(ctx, "BWTS_SEG_INV_BIG")) { const long long v = atoll(e); if (v >= 1) force_big = (u64)v; }
    return seg_inverse_plan(ctx->seg_off, force_plan, force_big);
}
static size_t seg_lane_arena_bytes(u64 n) { return align_up(n * 4, 256) + (1 << 16); }
// a shared pass's first attempt over a run of n bytes in `segs` segments: the default spacing, and the marks inverse_narrow_chain starts with
static size_t seg_pass_arena_bytes(u64 n, u64 segs)
{
    return n == 0 ? 0 : segs > SEG_MOMENTS_MAX_SEGMENTS ? inverse_attempt_bytes(n, inverse_splitter_log2(n), MARK_LOG) : inverse_arena_bytes(n);
}
static size_t seg_plan_arena_bytes(const SegInvPlan &p, u64 n)
{
    return p.plan == SEG_PLAN_SHARED ? seg_pass_arena_bytes(p.longest_run, p.longest_run_segs) : seg_lane_arena_bytes(n);
}
// what the host path reserves ahead for the context's current segment table: by the plan the call will take
size_t inverse_segments_arena_bytes(const bwts_ctx *ctx, u64 n)
{
    if (ctx->seg_off.size() <= 2) return inverse_arena_bytes(n);
    return seg_plan_arena_bytes(seg_inverse_plan(ctx), n);
}
// bwts_debug_segments_plan: the plan for a set of lengths, no context and no device (so no test switch either)
int inverse_segments_plan_words(const u64 *lengths, u64 count, u64 out[8])
{
    std::vector<u64> off(count + 1);
    off[0] = 0;
    for (u64 s = 0; s < count; s++) {
        if (lengths[s] == 0 || lengths[s] > 0x100000000ull - off[s]) return -1;
        off[s + 1] = off[s] + lengths[s];
    }
    const SegInvPlan p = seg_inverse_plan(off, -1, 0);
    const u64 w[8] = {(u64)p.plan, p.big, p.runs, p.own_segs, p.own_bytes, p.single_segs, p.single_bytes, (u64)seg_plan_arena_bytes(p, off[count])};
    memcpy(out, w, sizeof w);
    return p.plan;
}

// the sums a segmented call reports in bwts_timings: all cycles, the unreached elements summed over the passes, the largest attempt count
struct SegTotals {
    u64 cycles = 0, unvisited = 0; u32 attempts = 1;
    void add_last_pass(const bwts_ctx *ctx) { cycles += ctx->tm.factors; unvisited += ctx->tm.unvisited; if (ctx->tm.attempts > attempts) attempts = ctx->tm.attempts; }
};
static int seg_single_calls(bwts_ctx *ctx, const u8 *d_in, u8 *d_out, u64 big, SegTotals &t)
{
    const std::vector<u64> &off = ctx->seg_off;
    for (u64 s = 0; s + 1 < (u64)off.size(); s++) {
        const u64 len = off[s + 1] - off[s];
        if (len < big) continue;
        BWTS_TRY(inverse_device_impl(ctx, d_in + off[s], len, d_out + off[s]));
        t.add_last_pass(ctx);
    }
    return BWTS_OK;
}
// Plan A.  The walk costs its longest segment in dependent steps (or its bytes at the walk's throughput, when many chains share the
// chip); a single call costs a fixed latency per segment.
static int inverse_segments_lane(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, const SegInvPlan &pl, SegTotals &t)
{
    const u64 count = (u64)ctx->seg_off.size() - 1, big = pl.big, small = pl.own_bytes;
    BWTS_TRY(seg_single_calls(ctx, d_in, d_out, big, t));
    if (small) {
        BWTS_TRY(arena_reserve(ctx, seg_lane_arena_bytes(n)));
        u32 *LF = arena_array<u32>(ctx, n);
        if (!LF) return BWTS_E_NOMEM;
        unsigned long long *d_cyc = (unsigned long long *)(ctx->d_small + SMI_COUNTERS);
        HIPC(hipMemsetAsync(d_cyc, 0, sizeof(u64), ctx->stream));
        {
            SpanGuard sg(ctx, BWTS_K_LF_BUILD, small, 5 * small);
            seg_lf_kernel<<<dim3((unsigned)((count + 3) / 4)), dim3(256), 0, ctx->stream>>>(d_in, d_seg_off(ctx), count, big, LF);
            HIPC(hipGetLastError());
        }
        {
            SpanGuard sg(ctx, BWTS_K_WALK, small, 10 * small);
            seg_walk_kernel<<<dim3((unsigned)((count + 63) / 64)), dim3(64), 0, ctx->stream>>>(d_in, LF, d_seg_off(ctx), count, big, d_out, d_cyc);
            HIPC(hipGetLastError());
        }
        BWTS_TRY(read_small(ctx, SMI_COUNTERS, 1));
        t.cycles += ctx->h_small[SMI_COUNTERS];
    }
    return BWTS_OK;
}
// Plan B.  Every run's pass is the narrow form's chain of attempts over the run (LF per segment as indices of the run, symbols from the
// input, cycle ends per segment); it holds about what a single-input inverse of the run holds, reserved for the longest run before
// anything runs, so that a refusal (BWTS_E_NOMEM) leaves the call to plan A.
static int inverse_segments_shared(bwts_ctx *ctx, const u8 *d_in, u8 *d_out, const SegInvPlan &pl, SegTotals &t)
{
    const std::vector<u64> &off = ctx->seg_off;
    const u64 count = (u64)off.size() - 1, big = pl.big;
    if (pl.longest_run) BWTS_TRY(arena_reserve(ctx, seg_pass_arena_bytes(pl.longest_run, pl.longest_run_segs)));
    for (u64 a = 0; a < count;) {
        if (off[a + 1] - off[a] >= big) { a++; continue; }
        u64 b = a + 1;
        while (b < count && off[b + 1] - off[b] < big) b++;
        const InvSegs run = {d_seg_off(ctx) + a, b - a, off[a]};
        ctx->tm.attempts = 1;
        ctx->inv_attempts_made = 0;
        BWTS_TRY(inverse_narrow_chain(ctx, d_in + off[a], off[b] - off[a], d_out + off[a], &run));
        t.add_last_pass(ctx);
        a = b;
    }
    return seg_single_calls(ctx, d_in, d_out, big, t);          // (after the passes: bwts_debug_inverse_report describes the last pass that ran)
}

int inverse_segments_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out)
{
    const u64 count = (u64)ctx->seg_off.size() - 1;
    u64 *rep = ctx->seg_report;
    memset(rep, 0, sizeof ctx->seg_report);
    SegTotals t;
    if (count == 1) {
        BWTS_TRY(inverse_device_impl(ctx, d_in, n, d_out));
        rep[SR_SINGLE_SEGS] = 1; rep[SR_SINGLE_BYTES] = n; rep[SR_ATTEMPTS] = ctx->tm.attempts;
        return BWTS_OK;
    }
    SegInvPlan pl = seg_inverse_plan(ctx);
    int rc = BWTS_E_NOMEM, taken = pl.plan;
    if (pl.plan == SEG_PLAN_SHARED) {
        rc = inverse_segments_shared(ctx, d_in, d_out, pl, t);
        if (rc == BWTS_E_NOMEM) {                                   // no room for a pass: today's plan, from the start
            u64 big = 0;
            if (const char *e = bwts_knob(ctx, "BWTS_SEG_INV_BIG")) { const long long v = atoll(e); if (v >= 1) big = (u64)v; }
            pl = seg_inverse_plan(ctx->seg_off, SEG_PLAN_LANE, big);
            taken = SEG_PLAN_SHARED_NOMEM;
            t = SegTotals();
        }
    }
    if (pl.plan == SEG_PLAN_LANE) rc = inverse_segments_lane(ctx, d_in, n, d_out, pl, t);
    BWTS_TRY(rc);
    rep[SR_PLAN] = (u64)taken; rep[SR_BIG] = pl.big; rep[SR_RUNS] = pl.runs; rep[SR_OWN_SEGS] = pl.own_segs; rep[SR_OWN_BYTES] = pl.own_bytes;
    rep[SR_SINGLE_SEGS] = pl.single_segs; rep[SR_SINGLE_BYTES] = pl.single_bytes; rep[SR_ATTEMPTS] = t.attempts;
    ctx->tm.n = n;
    ctx->tm.factors = t.cycles;
    ctx->tm.unvisited = t.unvisited;
    ctx->tm.attempts = t.attempts;
    return BWTS_OK;
}
