// chunk_rounds.h -- the rounds after round 0 when many elements are tied, third form: CHUNKS.  Included by forward.hip.
//
// dense_rounds() (forward.hip) runs a round as three n-sized launches -- the round kernel leaves (position, head, state) for
// every list element, a count sweep reads the states, the compaction reads all three again -- with two host round trips, and a
// workgroup looks at DG_SPAN list slots to decide DG_OWN of them (a quarter of its loads are halo).  Here the list is cut ONCE
// into chunks at group boundaries, and a chunk belongs to one workgroup in every round:
//   * groups never straddle chunks, so a round needs no halo and no global compaction: the workgroup walks its chunk in tiles of
//     CH_TILE slots cut at group starts, orders every group in LDS exactly like dense_round_kernel, and writes the members that
//     stay tied back IN PLACE, compacted to the front of the chunk (the write cursor never passes the read cursor);
//   * the rank array is only read by the round kernel: the new ranks of the elements whose rank changed go to a per-chunk move
//     list of records, which chunk_apply_records_kernel applies when the round's gathers are all done (a round's keys must come from
//     one version of the ranks);
//   * the grid is one workgroup per chunk in every round and the sizes live on the device, so the host has nothing to read back
//     between rounds except "is anything left / did anything split": once no larger group is left it enqueues two rounds per sync.
// The one-off order by smallest position covers the groups of up to CH_CAP members; the larger ones are put behind them, unordered.
// Of those, groups of up to CH_GROUP_MAX (= a tile) members go to chunks of their own kind at once -- WIDE chunks, which a second
// instantiation of the round kernel handles: every tile ordered by one segmented bitonic sort of the workgroup in LDS instead of
// by counting inside each group; a WIDE chunk whose groups have all fallen to CH_CAP members or fewer is taken over by the
// counting instantiation.  Groups of more than CH_GROUP_MAX members form the BIG LIST, which goes through the sort-based round
// (gather, two radix sorts, regroup -- the larger-group path of dense_rounds on a dense list); whatever falls to CH_GROUP_MAX
// members or fewer leaves it as new chunks appended behind the existing ones.  Groups only ever split, so an element is appended
// at most once and the chunk store never outgrows the list.
#pragma once

#ifndef CH_THREADS
#define CH_THREADS 512
#endif
#ifndef CH_ITEMS
#define CH_ITEMS   4
#endif
#define CH_TILE    (CH_THREADS * CH_ITEMS)
#define CH_CAP     DG_CAP
#define CH_WORDS   (CH_TILE / 64)
#define CH_WORDS_BACK ((CH_CAP + 63) / 64)
#ifndef CH_MIN_WAVES
#define CH_MIN_WAVES 8
#endif
#ifndef CH_FS
#define CH_FS      256
#endif
// (factors whose data a workgroup keeps in LDS: natural data has a dozen or two)
#define CH_GROUP_MAX CH_TILE             // largest group a chunk may hold (a tile of its own in a WIDE chunk)
#define CH_MIN_LIST 65536ull            // shorter lists keep the tile form (dense_rounds)
#define CH_CUT_SLACK 128                // table entries beyond a0 / CH_TILE: one ragged chunk per cut (chunk_table_capacity)
#define CH_SLOTS   4                    // result slots of rounds in flight
#define CH_SLOT_WORDS 16
#define SM_CHSLOT  (SM_DGCNT + 16)      // CH_SLOTS x CH_SLOT_WORDS words inside the dense rounds' counter block
enum { CHS_SPLIT = 0, CHS_ERR = 1, CHS_TOTAL = 2, CHS_EXIT = 3, CHS_STAY = 4, CHS_BIGGROUPS = 5 };

static_assert(CH_CAP * 4 <= CH_TILE, "a tile must hold several whole groups");
static_assert(16 + CH_SLOTS * CH_SLOT_WORDS <= DG_CNT_BIG + DG_CNT_SPREAD, "result slots live in the dense rounds' counter block");

// WIDE chunks -- those that hold a group of more than CH_CAP members (up to CH_GROUP_MAX: what leaves the big list) -- are handled by a
// second instantiation of the kernel, which orders every tile with one segmented bitonic sort of the whole workgroup over
// (group's first slot, rank at h, ranks at 2h and 3h, slot) instead of counting inside each group: N slots (a power of two >= the
// tile), the slots behind the tile sort behind it.  pay = group's first slot << 16 | slot.
__device__ __forceinline__ void chunk_bitonic_sort(u32 *key, u64 *key23, u32 *pay, u32 N, int tid)
{
    for (u32 k = 2; k <= N; k <<= 1)
        for (u32 j = k >> 1; j > 0; j >>= 1) {
            for (u32 q = (u32)tid; q < N / 2; q += CH_THREADS) {
                const u32 i = ((q & ~(j - 1u)) << 1) | (q & (j - 1u)), l = i | j;
                const bool asc = (i & k) == 0;
                const u32 ka = key[i], kb = key[l], pa = pay[i], pb = pay[l];
                const u32 ga = pa >> 16, gb = pb >> 16;
                const u64 xa = key23[i], xb = key23[l];
                const bool gt = ga != gb ? ga > gb : ka != kb ? ka > kb : xa != xb ? xa > xb : pa > pb;
                if (gt == asc) { key23[i] = xb; key23[l] = xa; }
                if (gt == asc) { key[i] = kb; key[l] = ka; pay[i] = pb; pay[l] = pa; }
            }
            // a stage with j <= 64 stays inside blocks of 128 slots, and pair q belongs to block q / 64: wave w only ever touches blocks
            // w and w + 8.  Between two such stages the wave's own order is enough; the workgroup meets only around the wider ones.
            const u32 jn = j > 1 ? j >> 1 : k;          // the next stage's distance (k: the first stage of the next, doubled k)
            if (j > 64 || jn > 64) __syncthreads();
            else { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }
        }
    __syncthreads();
}

// chunk c = list slots [cstart[c], cstart[c] + ccount[c]); the region up to cstart[c + 1] (or the store's tail) is its own.
// The kernel is bound by its VALU instructions as much as by memory (PMC on the first version: ~350 per element, VALU busy 51 %,
// waves waiting 65 % of their cycles), so everything per element is 32-bit arithmetic: positions are u32 (n <= 2^32; lengths are
// kept modulo 2^32, which the wrap-around of the cyclic successor absorbs); the factor of a position comes from a 256-entry
// directory over the positions' top bits plus (nearly always) one comparison, and its start, length and the steps reduced
// modulo the length from one 16-byte LDS read (FSL: at most CH_FS factors -- natural data has a dozen or two; inputs with more
// take the instantiation with the general 64-bit arithmetic); and a slot's group extent comes from the wave's own __ballot word
// (which is exactly the 64 slots of its lanes) plus two per-word neighbour values, not from a bit search over LDS per lane.
template <bool CYCLIC, int NKEYS, bool FSL /* cyclic, at most CH_FS factors: their data sits in LDS */, bool WIDE /* the chunks flagged in cwide, and only those */>
__global__ __launch_bounds__(CH_THREADS, WIDE ? 4 : CH_MIN_WAVES) void chunk_round_kernel(u32 *idx, u32 *head, const u32 *__restrict__ cstart, u32 *__restrict__ ccount,
                                                                 u8 *__restrict__ cwide, u64 *__restrict__ mv, u32 *__restrict__ mvcount,
                                                                 const u32 *__restrict__ rank, u64 n, u64 h,
                                                                 const u32 *__restrict__ fstart, u64 k,
                                                                 PrevSym prev, u8 *__restrict__ out, unsigned long long *__restrict__ result)
{
    static_assert(NKEYS == 3, "the step is always quadrupled; NKEYS stays so the kernel keeps the symbol its PMC records name");
    __shared__ u32 hd[CH_TILE];              // group heads of the tile
    __shared__ u32 key[CH_TILE];             // successor ranks
    __shared__ u64 key23[CH_TILE];           // ... and the ranks two and three steps on
    __shared__ u64 startm[CH_WORDS];         // bit = a group starts at this slot
    __shared__ u64 keepm[CH_WORDS];          // bit = the element sorted into this slot stays tied
    __shared__ u32 kpre[CH_WORDS];
    __shared__ uint4 ftab[FSL ? CH_FS + 1 : 1];         // per factor: start, length (mod 2^32), the steps h and 2h modulo the length
    __shared__ u32 fhm3[FSL ? CH_FS : 1];               // ... and 3h
    __shared__ u32 fdir[FSL ? 256 : 1];                 // factor that holds position b << dsh: a lookup starts there
    __shared__ u32 hd2[WIDE ? CH_TILE : 1];  // (WIDE) the heads, while hd carries the sort's payload
    __shared__ u32 s_surv, s_nmv, s_split, s_err, s_wide;
    const int tid0 = threadIdx.x;
    const u32 c = blockIdx.x;
    if ((cwide[c] != 0) != WIDE) return;
    const u64 base = (u64)(u32)__builtin_amdgcn_readfirstlane((int)cstart[c]);
    const u32 cnt = (u32)__builtin_amdgcn_readfirstlane((int)ccount[c]);
    if (cnt == 0) { if (tid0 == 0) mvcount[c] = 0; return; }
    if (tid0 == 0) { s_nmv = 0; s_split = 0; s_err = 0; s_wide = 0; }
    // the step, wave-uniform.  Cyclic with the factors in LDS: per factor the step(s) reduced modulo its length (a division only
    // for factors shorter than the step: the short ones at the text's end), and a 256-entry directory over the positions' top bits
    // so that finding a position's factor is one table read and (nearly always) one comparison.  Suffixes: p + j h < n <=> p < nhj.
    u32 nh1 = 0, nh2 = 0, nh3 = 0;
    const u32 h32 = (u32)h, k32 = (u32)k;
    int dsh = 0;
    if (FSL) {
        for (u32 f = tid0; f < k32; f += CH_THREADS) {
            const u64 s0 = fstart[f], L = (f + 1 < k32 ? (u64)fstart[f + 1] : n) - s0;
            ftab[f] = make_uint4((u32)s0, (u32)L, (u32)(h < L ? h : h % L), (u32)(2 * h < L ? 2 * h : (2 * h) % L));
            fhm3[f] = (u32)(3 * h < L ? 3 * h : (3 * h) % L);
        }
        { int bl = 0; for (u64 x = n - 1; x; x >>= 1) bl++; dsh = bl > 8 ? bl - 8 : 0; }
        if (tid0 < 256) {
            const u64 want = (u64)tid0 << dsh;
            u32 lo = 0, hi = k32 - 1;
            while (lo < hi) { const u32 mid = (lo + hi + 1) >> 1; if ((u64)fstart[mid] <= want) lo = mid; else hi = mid - 1; }
            fdir[tid0] = lo;
        }
    } else if (!CYCLIC) {
        nh1 = h < n ? (u32)(n - h) : 0u;            // (h >= 1, so n - h fits)
        nh2 = 2 * h < n ? (u32)(n - 2 * h) : 0u; nh3 = 3 * h < n ? (u32)(n - 3 * h) : 0u;
    }
    u32 rp = 0, wp = 0;                      // read / write cursors inside the chunk (uniform)
#ifdef CH_PROFILE
    long long pt[7] = {0, 0, 0, 0, 0, 0, 0}, tprev = clock64();
#define CH_MARK(i) do { const long long tn__ = clock64(); pt[i] += tn__ - tprev; tprev = tn__; } while (0)
#else
#define CH_MARK(i) do { } while (0)
#endif
    while (rp < cnt) {
        // (an opaque copy of the thread id per iteration: left to itself the compiler hoists every address it can form from
        // tid out of the loop and keeps ~80 registers of them alive through the whole body -- 132 VGPRs instead of 48)
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63;
        const u32 wv = (u32)__builtin_amdgcn_readfirstlane(tid >> 6);
        const u32 len = cnt - rp < CH_TILE ? cnt - rp : (u32)CH_TILE;
        const bool final_tile = rp + len == cnt;
        u32 myh[CH_ITEMS], myp[CH_ITEMS];
#pragma unroll
        for (int j = 0; j < CH_ITEMS; j++) {
            const u32 sl = (u32)j * CH_THREADS + tid;
            myh[j] = sl < len ? head[base + rp + sl] : 0u;
            myp[j] = sl < len ? idx[base + rp + sl] : 0u;
        }
#pragma unroll
        for (int j = 0; j < CH_ITEMS; j++) hd[j * CH_THREADS + tid] = myh[j];
        if (tid < CH_WORDS) keepm[tid] = 0;
        __syncthreads();
        CH_MARK(0);
        // successor ranks: they depend on the positions alone, so the gathers are issued now and fly while the group extents are
        // worked out (slots of a group that is left for the next tile are gathered for nothing)
        // (Round 4 tried all twelve gathers of a lane in one straight run of loads -- the compiler drains them item by item, three in
        // flight, because the next item's factor search stands between: 8 % SLOWER, five more spilled registers and no shorter waits.)
        u32 my_key[CH_ITEMS];
        u64 my_key23[CH_ITEMS];
        u32 ppos[CH_ITEMS];                      // position of the previous symbol, T[cprev(p)] (mk_bwts_sa.c:172-188), while the factor is at hand
#pragma unroll
        for (int j = 0; j < CH_ITEMS; j++) {
            my_key[j] = 0; ppos[j] = 0;
            my_key23[j] = 0;
            if ((u32)j * CH_THREADS + tid >= len) continue;
            const u32 p = myp[j];
            if (CYCLIC) {
                u32 q1, q2, q3;
                if (FSL) {
                    // offset in the factor + step, minus the factor's length when the sum passes it (a carry out of 32 bits passes
                    // it too; a length of 2^32 is kept as 0: the subtraction then does nothing and the wrapped sum is already right)
                    u32 f = fdir[p >> dsh];
                    while (f + 1 < k32 && ftab[f + 1].x <= p) f++;
                    const uint4 ft = ftab[f];
                    const u32 s0 = ft.x, L = ft.y, dd = p - s0;
                    ppos[j] = dd ? p - 1u : s0 + L - 1u;
                    u32 o = dd + ft.z;
                    o = (o < dd || o >= L) ? o - L : o;
                    q1 = s0 + o;
                    u32 o2 = dd + ft.w, o3 = dd + fhm3[f];
                    o2 = (o2 < dd || o2 >= L) ? o2 - L : o2;
                    o3 = (o3 < dd || o3 >= L) ? o3 - L : o3;
                    q2 = s0 + o2; q3 = s0 + o3;
                } else {
                    const u64 f = factor_of(fstart, k, (u64)p);
                    const u64 s0 = fstart[f], e1 = factor_end(fstart, k, n, f);
                    ppos[j] = p == s0 ? (u32)(e1 - 1) : p - 1u;
                    q1 = (u32)cyclic_successor(p, s0, e1 - s0, h);
                    q2 = (u32)cyclic_successor(p, s0, e1 - s0, 2 * h); q3 = (u32)cyclic_successor(p, s0, e1 - s0, 3 * h);
                }
                my_key[j] = rank[q1];
                const u32 r2 = rank[q2], r3 = rank[q3];
                my_key23[j] = ((u64)r2 << 32) | r3;
            } else {
                my_key[j] = p < nh1 ? rank[p + h32] + 1u : 0u;
                const u32 r2 = p < nh2 ? rank[p + 2u * h32] + 1u : 0u, r3 = p < nh3 ? rank[p + 3u * h32] + 1u : 0u;
                my_key23[j] = ((u64)r2 << 32) | r3;
            }
        }
        // group starts: the 64 slots of a wave's item j are exactly word j * 8 + wave of the tile
        u64 stm[CH_ITEMS];
#pragma unroll
        for (int j = 0; j < CH_ITEMS; j++) {
            const u32 sl = (u32)j * CH_THREADS + tid;
            // slot 0 starts a group by construction (chunks and tiles are cut at group starts); slots past the end count as starts
            const bool st = sl >= len || sl == 0 || myh[j] != hd[sl - 1];
            stm[j] = __ballot(st);
            if (lane == 0) startm[(u32)j * (CH_THREADS / 64) + wv] = stm[j];
        }
        __syncthreads();
        const u64 le = lane == 63 ? ~0ull : (2ull << lane) - 1ull;       // slots of the word at or below mine
        u32 plen = len;
        u32 dst[CH_ITEMS], newhead[CH_ITEMS], dl[CH_ITEMS];      // dl: new rank - old rank
        bool alone[CH_ITEMS], act[CH_ITEMS];
        u32 split_here = 0;
        if constexpr (WIDE) {
            // ---- every group of the tile ordered by one segmented sort of the workgroup ----
            if (!final_tile) {
                int w = CH_WORDS - 1;
                u64 m = startm[w];
                while (m == 0 && w > 0) { w--; m = startm[w]; }
                plen = (u32)w * 64u + 63u - (u32)__clzll((long long)m);
            }
            plen = (u32)__builtin_amdgcn_readfirstlane((int)plen);
            if (plen == 0) {
                // one group fills the tile: it ends exactly here (the next slot shows another head), or it is too large to be in a chunk
                if (head[base + rp + len] != hd[0]) plen = len;
                else { if (tid == 0) s_err = 1; break; }
            }
            u32 N = 64; while (N < plen) N <<= 1;
            // every slot's group: the last start at or below it
            u32 gsl[CH_ITEMS];
#pragma unroll
            for (int j = 0; j < CH_ITEMS; j++) {
                const u32 sl = (u32)j * CH_THREADS + tid;
                gsl[j] = 0;
                if (sl < plen) {
                    u32 w = (u32)j * (CH_THREADS / 64) + wv;
                    u64 m = stm[j] & le;
                    while (m == 0ull) { w--; m = startm[w]; }          // (slot 0 starts a group: the walk ends)
                    gsl[j] = w * 64u + 63u - (u32)__clzll((long long)m);
                }
            }
            __syncthreads();                            // (every read of the heads in hd and of the start words is done)
#pragma unroll
            for (int j = 0; j < CH_ITEMS; j++) {
                const u32 sl = (u32)j * CH_THREADS + tid;
                hd2[WIDE ? sl : 0] = myh[j];
                if (sl < N) {
                    const bool real = sl < plen;
                    key[sl] = real ? my_key[j] : 0xffffffffu;
                    key23[sl] = real ? my_key23[j] : ~0ull;
                    hd[sl] = ((real ? gsl[j] : 0xffffu) << 16) | sl;
                }
            }
            __syncthreads();
            chunk_bitonic_sort(key, key23, hd, N, tid);
            // sorted slot t of this thread: whose element, which group, does a run of equal keys start / end here?
            bool rstart[CH_ITEMS], rend[CH_ITEMS];
            u32 src[CH_ITEMS], gst[CH_ITEMS];
            u64 rsm[CH_ITEMS];
#pragma unroll
            for (int j = 0; j < CH_ITEMS; j++) {
                const u32 t = (u32)j * CH_THREADS + tid;
                rstart[j] = true; rend[j] = true; src[j] = 0; gst[j] = 0;
                if (t < plen) {
                    const u32 pt = hd[t], kt = key[t];
                    const u64 xt = key23[t];
                    gst[j] = pt >> 16; src[j] = pt & 0xffffu;
                    if (t > gst[j]) rstart[j] = key[t - 1] != kt || key23[t - 1] != xt;
                    if (t + 1 < plen && (hd[t + 1] >> 16) == gst[j]) rend[j] = key[t + 1] != kt || key23[t + 1] != xt;
                }
                rsm[j] = __ballot(rstart[j]);
            }
            __syncthreads();                            // (the start words of the groups have been read by everyone: they now hold the runs')
#pragma unroll
            for (int j = 0; j < CH_ITEMS; j++)
                if (lane == 0) startm[(u32)j * (CH_THREADS / 64) + wv] = rsm[j];
            // the elements' positions through LDS (the keys are not needed any more)
#pragma unroll
            for (int j = 0; j < CH_ITEMS; j++) {
                const u32 sl = (u32)j * CH_THREADS + tid;
                if (sl < plen) key[sl] = myp[j];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < CH_ITEMS; j++) {
                const u32 t = (u32)j * CH_THREADS + tid;
                act[j] = t < plen;
                dst[j] = t; newhead[j] = 0; alone[j] = false; ppos[j] = 0; dl[j] = 0;
                if (!act[j]) continue;
                u32 w = (u32)j * (CH_THREADS / 64) + wv;
                u64 m = rsm[j] & le;
                while (m == 0ull) { w--; m = startm[w]; }              // (a group's first slot starts a run: the walk ends there at the latest)
                const u32 rbeg = w * 64u + 63u - (u32)__clzll((long long)m);
                const u32 less = rbeg - gst[j];
                const u32 p = key[src[j]];
                myp[j] = p;
                newhead[j] = hd2[WIDE ? gst[j] : 0] + less;
                dl[j] = less;
                alone[j] = rstart[j] && rend[j];
                split_here |= less != 0 ? 1u : 0u;
                if (!alone[j] && t - rbeg >= CH_CAP) s_wide = 1;        // a run of more than CH_CAP members stays: the chunk stays WIDE
                if (CYCLIC && out && alone[j] && !prev.P) {
                    if (FSL) {
                        u32 f = fdir[p >> dsh];
                        while (f + 1 < k32 && ftab[f + 1].x <= p) f++;
                        const uint4 ft = ftab[f];
                        ppos[j] = p != ft.x ? p - 1u : ft.x + ft.y - 1u;
                    } else {
                        const u64 f = factor_of(fstart, k, (u64)p);
                        const u64 s0 = fstart[f], e1 = factor_end(fstart, k, n, f);
                        ppos[j] = p == s0 ? (u32)(e1 - 1) : p - 1u;
                    }
                }
            }
            CH_MARK(1); CH_MARK(2);
        } else {
        // the group the tile's last start opens may go on in the next tile: it is left for that one
        if (!final_tile) {
            int w = CH_WORDS - 1;
            u64 m = startm[w];
            while (m == 0 && w > 0) { w--; m = startm[w]; }
            plen = (u32)w * 64u + 63u - (u32)__clzll((long long)m);
        }
        plen = (u32)__builtin_amdgcn_readfirstlane((int)plen);        // uniform: keep it (and the cursors) in scalar registers
        if (plen == 0) { if (tid == 0) s_err = 1; break; }          // a group of a whole tile: larger than CH_CAP, cannot be here
        // per word (lane l < CH_WORDS of every wave <-> word l): the last start before it, the first start behind it
        int cin_l = -1, cout_l = -1;
        if (lane < CH_WORDS) {
#pragma unroll
            for (int d = 1; d <= CH_WORDS_BACK; d++)
                if (cin_l < 0 && lane >= d) { const u64 pm = startm[lane - d]; if (pm) cin_l = (lane - d) * 64 + 63 - __clzll((long long)pm); }
#pragma unroll
            for (int d = 1; d <= CH_WORDS_BACK; d++)
                if (cout_l < 0 && lane + d < CH_WORDS) { const u64 nm = startm[lane + d]; if (nm) cout_l = (lane + d) * 64 + __ffsll((unsigned long long)nm) - 1; }
        }
        u32 gs[CH_ITEMS], sz[CH_ITEMS];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < CH_ITEMS; j++) {
            const u32 sl = (u32)j * CH_THREADS + tid;
            const u32 w = (u32)j * (CH_THREADS / 64) + wv;
            act[j] = sl < plen;
            gs[j] = 0; sz[j] = 0;
            const int cin = __builtin_amdgcn_readlane(cin_l, (int)w), cout = __builtin_amdgcn_readlane(cout_l, (int)w);
            const u64 below = stm[j] & le, above = stm[j] & ~le;
            const int g = below ? (int)(w * 64u) + 63 - __clzll((long long)below) : cin;
            int e = above ? (int)(w * 64u) + __ffsll((unsigned long long)above) - 1 : cout;
            if (e < 0 || (u32)e > plen) e = (int)plen;
            if (!act[j]) continue;
            if (g < 0 || e - g > CH_CAP) {
                bad = true; act[j] = false;
                if (atomicCAS(&result[5], 0ull, 1ull + c) == 0ull) {       // first failure: where (read by the host under BWTS_ROUND_TRACE)
                    result[6] = ((u64)(u32)g << 32) | (u32)e;
                    result[7] = ((u64)plen << 48) | ((u64)len << 32) | ((u64)rp << 16) | sl;
                }
                continue;
            }
            gs[j] = (u32)g; sz[j] = (u32)(e - g);
        }
        if (bad) s_err = 1;
        CH_MARK(1);
#pragma unroll
        for (int j = 0; j < CH_ITEMS; j++)
            if (act[j]) {
                key[j * CH_THREADS + tid] = my_key[j];
                key23[j * CH_THREADS + tid] = my_key23[j];
            }
        __syncthreads();
        CH_MARK(2);
        // order inside the group by counting (as dense_round_kernel)
#pragma unroll
        for (int j = 0; j < CH_ITEMS; j++) {
            const u32 sl = (u32)j * CH_THREADS + tid;
            dst[j] = sl; newhead[j] = 0; alone[j] = false; dl[j] = 0;
            if (!act[j]) continue;
            const u32 g0 = gs[j], gsz = sz[j], mine = key[sl];
            u32 less = 0, eq = 0, eq_before = 0;
            const u64 mine23 = key23[sl];
            u32 m = 0;
            for (; m + 4 <= gsz; m += 4) {
                u32 ko[4]; u64 ko23[4];
#pragma unroll
                for (int q = 0; q < 4; q++) { ko[q] = key[g0 + m + q]; ko23[q] = key23[g0 + m + q]; }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const bool same = ko[q] == mine && ko23[q] == mine23;
                    less += (ko[q] < mine || (ko[q] == mine && ko23[q] < mine23)) ? 1u : 0u;
                    eq += same ? 1u : 0u;
                    eq_before += (same && g0 + m + q < sl) ? 1u : 0u;
                }
            }
            for (; m < gsz; m++) {
                const u32 ko = key[g0 + m];
                const u64 ko23 = key23[g0 + m];
                const bool same = ko == mine && ko23 == mine23;
                less += (ko < mine || (ko == mine && ko23 < mine23)) ? 1u : 0u;
                eq += same ? 1u : 0u;
                eq_before += (same && g0 + m < sl) ? 1u : 0u;
            }
            dst[j] = g0 + less + eq_before;
            newhead[j] = myh[j] + less;
            dl[j] = less;
            alone[j] = eq == 1;
            split_here |= eq < gsz ? 1u : 0u;
        }
        }
        CH_MARK(3);
        u32 pv[CH_ITEMS];
        bool wr[CH_ITEMS];
#pragma unroll
        for (int j = 0; j < CH_ITEMS; j++) {
            // a member writes its byte once, when it is alone (ppos: its cyclic predecessor when the factors sit in LDS and no
            // previous-symbol array exists)
            wr[j] = out && act[j] && alone[j];
            pv[j] = wr[j] ? (prev.P ? (u32)prev.P[myp[j]] : (u32)prev.T[ppos[j]]) : 0u;
        }
#pragma unroll
        for (int j = 0; j < CH_ITEMS; j++)
            if (act[j] && !alone[j]) atomicOr((unsigned long long *)&keepm[dst[j] >> 6], 1ull << (dst[j] & 63u));
        // the members whose rank changed: (new rank, position) to the chunk's record list (any order)
#pragma unroll
        for (int j = 0; j < CH_ITEMS; j++) {
            const bool mvd = act[j] && dl[j] != 0;
            const u64 mm = __ballot(mvd);
            if (mm) {
                const int leader = __ffsll((unsigned long long)mm) - 1;
                u32 b0 = 0;
                if (lane == leader) b0 = atomicAdd(&s_nmv, (u32)__popcll(mm));
                b0 = shfl_t(b0, leader);
                if (mvd) mv[base + b0 + (u32)__popcll(mm & (le >> 1))] = ((u64)newhead[j] << 32) | (u64)myp[j];
            }
        }
#pragma unroll
        for (int j = 0; j < CH_ITEMS; j++)
            if (wr[j]) out[newhead[j]] = (u8)pv[j];
        if (split_here) s_split = 1;
        __syncthreads();
        CH_MARK(4);
        if (tid < 64) {
            const u32 cpop = tid < CH_WORDS ? (u32)__popcll(keepm[tid < CH_WORDS ? tid : 0]) : 0u;
            const u32 inc = wave_scan_inclusive(cpop, OpAdd());
            if (tid < CH_WORDS) kpre[tid] = inc - cpop;
            if (tid == CH_WORDS - 1) s_surv = inc;
        }
        __syncthreads();
        // the members that stay, in sorted order, to the front of the chunk: wp + survivors <= rp + plen, and every load of this
        // tile is behind the barriers above, so nothing unread is overwritten
#pragma unroll
        for (int j = 0; j < CH_ITEMS; j++)
            if (act[j] && !alone[j]) {
                const u32 w = dst[j] >> 6, b = dst[j] & 63u;
                const u64 lowbits = keepm[w] & ((1ull << b) - 1ull);
                const u32 o = wp + kpre[w] + (u32)__popcll(lowbits);
                idx[base + o] = myp[j];
                head[base + o] = newhead[j];
            }
        wp += (u32)__builtin_amdgcn_readfirstlane((int)s_surv);
        rp += plen;
        __syncthreads();
        CH_MARK(5);
    }
    __syncthreads();
    if (tid0 == 0) {
        ccount[c] = wp;
        mvcount[c] = s_nmv;
        if (WIDE && !s_wide) cwide[c] = 0;          // only groups of up to CH_CAP members are left: the other instantiation takes over
        if (s_split && __hip_atomic_load(&result[CHS_SPLIT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
            __hip_atomic_store(&result[CHS_SPLIT], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s_err) __hip_atomic_store(&result[CHS_ERR], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef CH_PROFILE
        for (int i = 0; i < 6; i++) atomicAdd(&result[64 + 8 * (c & 63) + i], (unsigned long long)pt[i]);      // spread: one address would serialise
#endif
    }
#undef CH_MARK
}

// ---- the record pass: runs when every gather of the round is done ---------------------------------------------------------------
// A record is (new rank << 32 | position) of a member whose rank changed.
struct RecordTargets {
    u32 *rank; PrevSym prev; u8 *out; u32 *SA;
};
// MODE 0: the rounds: the new rank, nothing else to do.  MODE 1: the final lay-out of equal words: the same records for every member
// left, with its byte and suffix-array slot.
template <int MODE>
__global__ __launch_bounds__(256) void chunk_apply_records_kernel(u64 *__restrict__ mv, const u32 *__restrict__ cstart, const u32 *__restrict__ mvcount, RecordTargets cx)
{
    const u32 c = blockIdx.x;
    const u32 m = mvcount[c];
    const u64 base = cstart[c];
    // (four records per lane and step, read before any of them is applied: the rank array may alias the records as far as the
    // compiler knows, so one by one every record's load waited for the store before it)
    for (u32 i0 = 0; i0 < m; i0 += 1024) {
        u64 e[4];
#pragma unroll
        for (int t = 0; t < 4; t++) { const u32 i = i0 + (u32)t * 256 + threadIdx.x; e[t] = mv[base + (i < m ? i : m - 1)]; }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (i0 + (u32)t * 256 + threadIdx.x >= m) continue;
            const u32 q = (u32)e[t], nr = (u32)(e[t] >> 32);
            cx.rank[q] = nr;
            if (MODE == 1) {
                if (cx.out) cx.out[nr] = cx.prev((u64)q);
                if (cx.SA) cx.SA[nr] = q;
            }
        }
    }
}

// elements still tied over all chunks; with off, also the exclusive sums of ccount for chunk_compact_kernel.  One workgroup loops over
// the tables: up to a0 / CH_TILE + CH_CUT_SLACK chunks, 1024 per step (nothing here is indexed by chunk but the global tables)
__global__ __launch_bounds__(1024) void chunk_total_kernel(const u32 *__restrict__ ccount, u32 nchunks, unsigned long long *__restrict__ result,
                                                           u32 *__restrict__ off)
{
    __shared__ u64 sm[16];
    __shared__ u32 carry;
    u64 s = 0;
    for (u32 i = threadIdx.x; i < nchunks; i += 1024) s += ccount[i];
    s = wave_scan_inclusive(s, OpAdd());
    if (lane_id() == 63) sm[wave_id()] = s;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    if (threadIdx.x == 0) { u64 t = 0; for (int w = 0; w < 16; w++) t += sm[w]; result[CHS_TOTAL] = t; }
    if (!off) return;
    __shared__ u32 wtot[16];
    for (u32 i0 = 0; i0 < nchunks; i0 += 1024) {
        const u32 i = i0 + threadIdx.x;
        const u32 v = i < nchunks ? ccount[i] : 0u;
        const u32 inc = wave_scan_inclusive(v, OpAdd());
        __syncthreads();                                      // (wtot / carry of the previous step have been read)
        if (lane_id() == 63) wtot[wave_id()] = inc;
        __syncthreads();
        u32 before = carry;
        for (int w = 0; w < wave_id(); w++) before += wtot[w];
        if (i < nchunks) off[i] = before + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + inc;
    }
    __syncthreads();
    if (threadIdx.x == 0) off[nchunks] = carry;
}

// When most of the list has settled the chunks are nearly empty, and a round pays a workgroup's set-up per chunk for a handful
// of elements: the survivors are then copied, chunk after chunk (groups stay whole and in order), into the other pair of list arrays and
// new chunks are cut over the dense list.  off: exclusive sums of ccount.
__global__ __launch_bounds__(256) void chunk_compact_kernel(const u32 *__restrict__ idx, const u32 *__restrict__ head, const u32 *__restrict__ cstart,
                                                            const u32 *__restrict__ ccount, const u32 *__restrict__ off, u32 *__restrict__ nidx, u32 *__restrict__ nhead)
{
    const u32 c = blockIdx.x;
    const u64 base = cstart[c], o = off[c];
    const u32 cnt = ccount[c];
    for (u32 i = threadIdx.x; i < cnt; i += 256) { nidx[o + i] = idx[base + i]; nhead[o + i] = head[base + i]; }
}

// chunks c0 .. c0 + nch over list slots [lo, hi): chunk i nominally starts at lo + i * S, actually at the first group start at
// or after that (groups here have at most CH_GROUP_MAX members; a wave looks at 64 slots at a time).  One wave per chunk; it also
// walks the chunk once to see whether a group of more than CH_CAP members is in it (-> cwide).
__device__ __forceinline__ u64 chunk_group_start_at_or_after(const u32 *__restrict__ head, u64 lo, u64 hi, u64 s, int lane)
{
    if (s > hi) s = hi;
    if (s <= lo || s >= hi) return s;
    for (;;) {
        const u64 i = s + (u64)lane;
        const bool st = i >= hi || head[i] != head[i - 1];
        const u64 m = __ballot(st);
        if (m) return s + (u64)(__ffsll((unsigned long long)m) - 1);
        s += 64;
    }
}
__global__ __launch_bounds__(256) void chunk_init_kernel(const u32 *__restrict__ head, u64 lo, u64 hi, u32 S, u32 c0, u32 nch,
                                                         u32 *__restrict__ cstart, u32 *__restrict__ ccount, u32 *__restrict__ mvcount, u8 *__restrict__ cwide,
                                                         bool may_be_wide)
{
    const u32 i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= nch) return;
    const u64 s = chunk_group_start_at_or_after(head, lo, hi, lo + (u64)i * S, lane);
    const u64 e = i + 1 < nch ? chunk_group_start_at_or_after(head, lo, hi, lo + (u64)(i + 1) * S, lane) : hi;
    bool wide = false;
    if (may_be_wide) {
        u64 last = s;                           // the most recent group start seen
        for (u64 b = s; b < e && !wide; b += 64) {
            const u64 q = b + (u64)lane;
            const bool st = q < e && (q == s || head[q] != head[q - 1]);
            const u64 m = __ballot(st);
            if (m) {
                if (b + (u64)(__ffsll((unsigned long long)m) - 1) - last > CH_CAP) wide = true;
                last = b + 63u - (u64)__clzll((long long)m);
            }
        }
        if (e - last > CH_CAP) wide = true;
    }
    if (lane == 0) {
        cstart[c0 + i] = (u32)s;
        ccount[c0 + i] = (u32)(e - s);
        mvcount[c0 + i] = 0;
        cwide[c0 + i] = wide ? 1 : 0;
    }
}

// what is left when no group splits any more (equal infinite words): the members take their group's slots in list order -- as records
// (new rank = head + place in the group), whose byte and suffix-array slot the record pass writes
__global__ __launch_bounds__(256) void chunk_rest_records_kernel(const u32 *__restrict__ idx, const u32 *__restrict__ head, const u32 *__restrict__ cstart,
                                                                 const u32 *__restrict__ ccount, u64 *__restrict__ mv, u32 *__restrict__ mvcount)
{
    const u32 c = blockIdx.x;
    const u64 base = cstart[c];
    const u32 cnt = ccount[c];
    for (u32 i = threadIdx.x; i < cnt; i += 256) {
        const u32 hh = head[base + i];
        u32 o = 0;
        while (o < i && head[base + i - o - 1] == hh) o++;
        mv[base + i] = ((u64)(hh + o) << 32) | (u64)idx[base + i];
    }
    if (threadIdx.x == 0) mvcount[c] = cnt;
}

// ---- the one-off order, by GROUP RECORDS ----------------------------------------------------------------------------------------
// The list only has to come out with its groups in the order of their smallest positions.  Sorting the elements for that (round 2, and
// the first form of this file) moves 32 bytes per element and pass; the groups are two or three members each on text, so one record per
// group -- (size << 32 | smallest position, list index of its first member) -- is sorted instead, the sizes are scanned in sorted order
// and the members copied to their places (go_expand_kernel).  Members of groups larger than CH_CAP are not ordered at all: they are
// compacted, in list (= SA) order, behind everything else and become the big list.
// tile_counts[t] (exclusive-scanned in place before go_write_kernel; entry [tiles] = totals): low word = group records, high = big elements
__global__ __launch_bounds__(DG_THREADS) void go_count_kernel(const u32 *__restrict__ idx, const u32 *__restrict__ head, u64 a, u64 *__restrict__ tile_counts)
{
    __shared__ u32 hd[DG_SPAN];
    __shared__ u64 startm[DG_SPAN / 64];
    __shared__ u64 wsum[DG_THREADS / 64];
    const int tid = threadIdx.x;
    const long long e0 = (long long)blockIdx.x * DG_OWN - DG_CAP;
    DgSlots ds;
    dg_detect(idx, head, a, e0, hd, startm, ds);
    u64 c = 0;
#pragma unroll
    for (int j = 0; j < DG_ITEMS; j++) {
        const u32 sl = (u32)j * DG_THREADS + tid;
        if (ds.kind[j] == 1 && ds.gs[j] == sl) c += 1ull;
        if (ds.kind[j] == 2) c += 1ull << 32;
    }
    c = wave_scan_inclusive(c, OpAdd());
    if (lane_id() == 63) wsum[wave_id()] = c;
    __syncthreads();
    if (tid == 0) { u64 t = 0; for (int w = 0; w < DG_THREADS / 64; w++) t += wsum[w]; tile_counts[blockIdx.x] = t; }
}
__global__ __launch_bounds__(DG_THREADS) void go_write_kernel(const u32 *__restrict__ idx, const u32 *__restrict__ head, u64 a, const u64 *__restrict__ tile_off, u64 tiles,
                                                              u64 *__restrict__ rkeys, u32 *__restrict__ rvals, u32 *__restrict__ st_idx, u32 *__restrict__ st_head,
                                                              bool pairs /* n <= 2^31: bit 31 of a position is free to tell the two record forms apart */)
{
    __shared__ u32 hd[DG_SPAN];
    __shared__ u32 pos[DG_SPAN];
    __shared__ u64 startm[DG_SPAN / 64];
    __shared__ u32 wcnt[2][DG_ITEMS][DG_THREADS / 64];           // per (item row, wave): records, big elements -- rows are consecutive slot ranges
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long e0 = (long long)blockIdx.x * DG_OWN - DG_CAP;
    DgSlots ds;
    dg_detect(idx, head, a, e0, hd, startm, ds);
#pragma unroll
    for (int j = 0; j < DG_ITEMS; j++)
        if (ds.kind[j] == 1) pos[j * DG_THREADS + tid] = ds.idx[j];
    u64 rm[DG_ITEMS], bm[DG_ITEMS];
#pragma unroll
    for (int j = 0; j < DG_ITEMS; j++) {
        const u32 sl = (u32)j * DG_THREADS + tid;
        rm[j] = __ballot(ds.kind[j] == 1 && ds.gs[j] == sl);
        bm[j] = __ballot(ds.kind[j] == 2);
        if (lane == 0) { wcnt[0][j][wv] = (u32)__popcll(rm[j]); wcnt[1][j][wv] = (u32)__popcll(bm[j]); }
    }
    __syncthreads();
    const u64 off = tile_off[blockIdx.x], tot = tile_off[tiles];
    const u64 a_small = a - (tot >> 32);                       // the larger groups' members land behind the smaller groups' (list order kept)
#pragma unroll
    for (int j = 0; j < DG_ITEMS; j++) {
        u32 rbefore = 0, bbefore = 0;
        for (int jj = 0; jj <= j; jj++)
            for (int w = 0; w < DG_THREADS / 64; w++)
                if (jj < j || w < wv) { rbefore += wcnt[0][jj][w]; bbefore += wcnt[1][jj][w]; }
        const u32 sl = (u32)j * DG_THREADS + tid;
        if (ds.kind[j] == 1 && ds.gs[j] == sl) {
            u32 mn = 0xffffffffu, mx = 0;
            for (u32 m = 0; m < ds.sz[j]; m++) { const u32 q = pos[sl + m]; mn = q < mn ? q : mn; mx = q > mx ? q : mx; }
            const u64 r = (u32)off + rbefore + (u32)__popcll(rm[j] & lanemask_lt());
            if (pairs && ds.sz[j] == 2) {
                // a group of two travels whole: (larger position << 32 | smaller position, head) -- its members need not be fetched again
                rkeys[r] = ((u64)mx << 32) | mn;
                rvals[r] = ds.h[j];
            } else {
                rkeys[r] = ((u64)((pairs ? 0x80000000u : 0u) | ds.h[j]) << 32) | mn;        // the group's head = the SA slot of its first member
                rvals[r] = ds.sz[j];
            }
        }
        if (ds.kind[j] == 2) {
            const u64 o = a_small + (off >> 32) + bbefore + (u32)__popcll(bm[j] & lanemask_lt());
            st_idx[o] = ds.idx[j];
            st_head[o] = ds.h[j];
        }
    }
}
// record forms (go_write_kernel): pairs == false: (head = SA slot of the first member << 32 | smallest position, size); pairs == true:
// bit 63 set: the same with the flag; bit 63 clear: a group of two, (larger position << 32 | smaller position, head)
struct GoSizeIn {
    const u64 *rk; const u32 *rv; bool pairs;
    __device__ __forceinline__ u32 operator()(u64 j) const { return (pairs && !(rk[j] >> 63)) ? 2u : rv[j]; }
};
// members of the sorted groups to their places: a pair comes out of its record; the others are read from the suffix array itself -- a
// group is the slot range [head, head + size) there, and all its members carry that head -- a lane copying its own group when it is
// short, the wave together the longer ones (one scattered read per group)
__global__ __launch_bounds__(256) void go_expand_kernel(const u64 *__restrict__ rkeys, const u32 *__restrict__ rvals, const u32 *__restrict__ doff, u64 groups,
                                                        const u32 *__restrict__ SA, u32 *__restrict__ st_idx, u32 *__restrict__ st_head,
                                                        bool pairs)
{
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    const int lane = lane_id();
    u32 e = 0, sz = 0, d = 0;
    if (j < groups) {
        const u64 k = rkeys[j];
        const u32 v = rvals[j];
        d = doff[j];
        if (pairs && !(k >> 63)) {
            st_idx[d] = (u32)k; st_idx[d + 1] = (u32)(k >> 32);
            st_head[d] = v; st_head[d + 1] = v;
        } else { e = (u32)(k >> 32) & (pairs ? 0x7fffffffu : 0xffffffffu); sz = v; }
    }
    {
        // (a short group's members: four loads issued together, from the group's first slot where it has fewer -- not one behind a test each)
        const bool few = sz && sz <= 4;
        u32 pi[4];
#pragma unroll
        for (u32 t = 0; t < 4; t++) pi[t] = SA[(u64)e + (few && t < sz ? t : 0u)];
        if (few) {
#pragma unroll
            for (u32 t = 0; t < 4; t++) if (t < sz) { st_idx[d + t] = pi[t]; st_head[d + t] = e; }
        }
    }
    u64 longm = __ballot(sz > 4);
    while (longm) {
        const int r = __ffsll((unsigned long long)longm) - 1;
        longm &= longm - 1;
        const u32 re = shfl_t(e, r), rs = shfl_t(sz, r), rd = shfl_t(d, r);
        for (u32 t = (u32)lane; t < rs; t += 64) {
            const u32 pp = SA[(u64)re + t];
            st_idx[rd + t] = pp; st_head[rd + t] = re;
        }
    }
}

// ---- the big list ---------------------------------------------------------------------------------------------------------
struct BlIn {
    const u32 *head;
    __device__ __forceinline__ u32 operator()(u64 j) const { return (j == 0 || head[j] != head[j - 1]) ? 1u : 0u; }
};
template <bool CYCLIC>
struct BlOut {
    const u32 *head; const u32 *idx; int rb; const u32 *rank; u64 n; u64 h; const u32 *fstart; u64 k;
    u64 *bk; u32 *bv;
    u64 *k23, *k23_sort; u32 *j_sort;        // see DgBigOut
    __device__ __forceinline__ void operator()(u64 j, u32 before) const
    {
        const u32 st = (j == 0 || head[j] != head[j - 1]) ? 1u : 0u;
        const u64 ord = (u64)before + st - 1;
        const u64 p = idx[j];
        u64 r1, r2, r3;
        if (CYCLIC) {
            const u64 f = factor_of(fstart, k, p);
            const u64 s0 = fstart[f], L = factor_end(fstart, k, n, f) - s0;
            r1 = rank[cyclic_successor(p, s0, L, h)];
            r2 = rank[cyclic_successor(p, s0, L, 2 * h)]; r3 = rank[cyclic_successor(p, s0, L, 3 * h)];
        } else {
            const u64 q = p + h;
            r1 = q < n ? (u64)rank[q] + 1ull : 0ull;
            const u64 q2 = p + 2 * h, q3 = p + 3 * h;
            r2 = q2 < n ? (u64)rank[q2] + 1ull : 0ull;
            r3 = q3 < n ? (u64)rank[q3] + 1ull : 0ull;
        }
        bk[j] = (ord << rb) | r1;
        bv[j] = (u32)p;
        const u64 v = (r2 << rb) | r3;
        k23[j] = v; k23_sort[j] = v; j_sort[j] = (u32)j;
    }
};
// after the sorts, in sorted order.  bl_flags_kernel looks at every element and its predecessor once -- first of its group (the ordinal
// changes), first of its new subgroup (any of the three ranks changes) -- and fetches the element's position; what follows reads
// the flag bytes and positions in sequence.  (The regrouping scan used to do the comparisons itself, in both of its sweeps: three
// gathers through the second sort's permutation per element and sweep.)
#define BLF_GROUP 1u
#define BLF_SUB   2u
__global__ __launch_bounds__(256) void bl_flags_kernel(const u64 *__restrict__ bk, const u32 *__restrict__ src, const u64 *__restrict__ k23,
                                                       const u32 *__restrict__ bv, u64 m, int rb, u8 *__restrict__ flags, u32 *__restrict__ t_idx)
{
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    const bool valid = j < m;
    const u64 key = valid ? bk[j] : 0ull;
    const u32 s = valid ? src[j] : 0u;
    const u64 q = valid ? k23[s] : 0ull;
    if (valid) t_idx[j] = bv[s];
    u64 kprev = shfl_up_t(key, 1), qprev = shfl_up_t(q, 1);
    if (lane_id() == 0 && valid && j > 0) { kprev = bk[j - 1]; qprev = k23[src[j - 1]]; }
    if (!valid) return;
    const bool gstart = j == 0 || (kprev >> rb) != (key >> rb);
    const bool sstart = gstart || kprev != key || qprev != q;
    flags[j] = (u8)((gstart ? BLF_GROUP : 0u) | (sstart ? BLF_SUB : 0u));
}
// regrouping scan (max on both halves, see OpMax2): high word = 1 + index of the element's group start, low word = 1 + index of its
// subgroup start
struct BlFlagIn {
    const u8 *flags;
    __device__ __forceinline__ u64 operator()(u64 j) const
    {
        const u32 f = flags[j];
        return ((u64)((f & BLF_GROUP) ? (u32)j + 1u : 0u) << 32) | (u64)((f & BLF_SUB) ? (u32)j + 1u : 0u);
    }
};
// new heads, final bytes, new ranks (every gather of the round is done by now); and, for the split that follows, every element's
// subgroup start and -- written by the subgroup's last element -- the subgroup's size
struct BlRegroupOut {
    const u8 *flags; const u32 *oldhead; u64 m;
    const u32 *t_idx; u32 *t_head; u32 *rank; PrevSym prev; u8 *out; unsigned long long *result;
    u32 *rstart; u32 *rsize;
    __device__ __forceinline__ void operator()(u64 j, u64 v) const       // inclusive (max, max) scan value
    {
        const u32 gidx = (u32)(v >> 32) - 1u, sidx = (u32)v - 1u;
        const u32 newhead = oldhead[j] + (sidx - gidx);        // sorting keeps every group on its own slots, all holding its old head
        const u32 p = t_idx[j];
        t_head[j] = newhead;
        if (sidx != gidx) rank[p] = newhead;
        const bool last_of_sub = j + 1 == m || (flags[j + 1] & BLF_SUB);
        if (out && sidx == (u32)j && last_of_sub) out[newhead] = prev(p);
        rstart[j] = sidx;
        if (last_of_sub) rsize[sidx] = (u32)j - sidx + 1u;
        const u64 splitm = __ballot(sidx != gidx);
        if (splitm && lane_id() == __ffsll((unsigned long long)__ballot(true)) - 1 &&
            __hip_atomic_load(&result[CHS_SPLIT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
            __hip_atomic_store(&result[CHS_SPLIT], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
// class of every element of the (regrouped) big list: 0 alone (finished), 1 in a group of 2 .. CH_GROUP_MAX (leaves for a chunk),
// 2 stays.  Group sizes from the run lengths of equal heads: an inclusive max-scan gives every element its run's first index, the
// run's last element writes the length there.
struct BlRunIn {
    const u32 *head;
    __device__ __forceinline__ u32 operator()(u64 i) const { return (i == 0 || head[i] != head[i - 1]) ? (u32)i + 1u : 0u; }
};
struct BlRunOut {
    const u32 *head; u64 m; u32 *rstart; u32 *rsize;
    __device__ __forceinline__ void operator()(u64 i, u32 v) const
    {
        const u32 s = v - 1u;
        rstart[i] = s;
        if (i + 1 == m || head[i + 1] != head[i]) rsize[s] = (u32)i - s + 1u;
    }
};
__device__ __forceinline__ u32 bl_class(const u32 *__restrict__ rstart, const u32 *__restrict__ rsize, u64 i)
{
    const u32 sz = rsize[rstart[i]];
    return sz > CH_GROUP_MAX ? 2u : (sz >= 2 ? 1u : 0u);
}
struct BlSplitIn {
    const u32 *rstart; const u32 *rsize;
    __device__ __forceinline__ u64 operator()(u64 i) const { const u32 c = bl_class(rstart, rsize, i); return (u64)(c == 1 ? 1u : 0u) | ((u64)(c == 2 ? 1u : 0u) << 32); }
};
struct BlSplitOut {
    const u32 *rstart; const u32 *rsize; const u32 *t_idx; const u32 *t_head; u64 m;
    u32 *x_idx, *x_head;          // where the leaving elements go (the chunk store's tail)
    u32 *s_idx, *s_head;          // the next big list
    unsigned long long *result;
    __device__ __forceinline__ void operator()(u64 i, u64 before) const
    {
        const u32 c = bl_class(rstart, rsize, i);
        if (c == 1) { const u32 o = (u32)before; x_idx[o] = t_idx[i]; x_head[o] = t_head[i]; }
        else if (c == 2) {
            const u32 o = (u32)(before >> 32); s_idx[o] = t_idx[i]; s_head[o] = t_head[i];
            // (the next round's group ordinals are below this count: it sizes the sort key)
            const u64 firsts = __ballot(rstart[i] == (u32)i);
            if (lane_id() == __ffsll((unsigned long long)firsts) - 1) atomicAdd(&result[CHS_BIGGROUPS], (unsigned long long)__popcll(firsts));
        }
        if (i + 1 == m) { result[CHS_EXIT] = (u64)(u32)before + (c == 1 ? 1u : 0u); result[CHS_STAY] = (before >> 32) + (c == 2 ? 1u : 0u); }
    }
};

// (BWTS_ROUND_TRACE only) which of the big list's groups hold one value of the rank at h / of all three ranks: such a group cannot split
__global__ void bl_diag_flag_kernel(const u64 *__restrict__ bk0, const u64 *__restrict__ k23, u64 m, int rb, u8 *__restrict__ f1, u8 *__restrict__ f23)
{
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0 || j >= m) return;
    const u64 a = bk0[j], b = bk0[j - 1];
    if ((a >> rb) != (b >> rb)) return;
    if (a != b) f1[a >> rb] = 1;
    if (k23[j] != k23[j - 1]) f23[a >> rb] = 1;
}
__global__ void bl_diag_count_kernel(const u64 *__restrict__ bk0, u64 m, int rb, const u8 *__restrict__ f1, const u8 *__restrict__ f23, unsigned long long *cnt)
{
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = j < m;
    const u64 o = in ? bk0[j] >> rb : 0;
    const u64 c1 = __ballot(in && !f1[o]), c3 = __ballot(in && !f1[o] && !f23[o]);
    if (lane_id() == 0) { if (c1) atomicAdd(&cnt[0], (unsigned long long)__popcll(c1)); if (c3) atomicAdd(&cnt[1], (unsigned long long)__popcll(c3)); }
    if (in && j + 1 == m) cnt[2] = o + 1;
}

// (BWTS_ROUND_TRACE only) elements of the regrouped big list by log2 of their group's size
__global__ void bl_diag_sizes_kernel(const u32 *__restrict__ rstart, const u32 *__restrict__ rsize, u64 m, unsigned long long *hist)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || rstart[i] != (u32)i) return;
    const u32 sz = rsize[i];
    atomicAdd(&hist[31 - __clz(sz)], (unsigned long long)sz);
    atomicAdd(&hist[32 + 31 - __clz(sz)], 1ull);
}
static void bl_diag_sizes(bwts_ctx *ctx, const u32 *rstart, const u32 *rsize, u64 m, const char *what)
{
    unsigned long long *d = nullptr, hh[64];
    if (hipMalloc((void **)&d, sizeof(hh)) != hipSuccess) return;
    (void)hipMemsetAsync(d, 0, sizeof(hh), ctx->stream);
    bl_diag_sizes_kernel<<<dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream>>>(rstart, rsize, m, d);
    (void)hipMemcpyAsync(hh, d, sizeof(hh), hipMemcpyDeviceToHost, ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    fprintf(stderr, "[chunks] %s: elements (groups) by log2 group size:", what);
    for (int b = 0; b < 32; b++) if (hh[b]) fprintf(stderr, " %d:%llu(%llu)", b, hh[b], hh[32 + b]);
    fprintf(stderr, "\n");
}

// (BWTS_ROUND_TRACE only) elements of the chunks by the size of their group: 2, 3-4, 5-16, 17-64, 65-256, 257-2048
__global__ __launch_bounds__(256) void chunk_diag_sizes_kernel(const u32 *__restrict__ head, const u32 *__restrict__ cstart, const u32 *__restrict__ ccount, unsigned long long *hist)
{
    const u32 c = blockIdx.x, cnt = ccount[c];
    const u64 base = cstart[c];
    for (u32 i = threadIdx.x; i < cnt; i += 256) {
        if (i && head[base + i] == head[base + i - 1]) continue;
        u32 e = i + 1;
        while (e < cnt && head[base + e] == head[base + i]) e++;
        const u32 sz = e - i;
        const int cls = sz <= 2 ? 0 : sz <= 4 ? 1 : sz <= 16 ? 2 : sz <= 64 ? 3 : sz <= 256 ? 4 : 5;
        atomicAdd(&hist[cls], (unsigned long long)sz);
    }
}
static void chunk_diag_sizes(bwts_ctx *ctx, const u32 *head, const u32 *cstart, const u32 *ccount, u32 nchunks, u32 round)
{
    unsigned long long *d = nullptr, hh[6];
    if (!nchunks || hipMalloc((void **)&d, sizeof(hh)) != hipSuccess) return;
    (void)hipMemsetAsync(d, 0, sizeof(hh), ctx->stream);
    chunk_diag_sizes_kernel<<<dim3(nchunks), dim3(256), 0, ctx->stream>>>(head, cstart, ccount, d);
    (void)hipMemcpyAsync(hh, d, sizeof(hh), hipMemcpyDeviceToHost, ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    fprintf(stderr, "[chunks] before round %u, chunk elements by group size: 2: %llu  3-4: %llu  5-16: %llu  17-64: %llu  65-256: %llu  257-2048: %llu\n", round, hh[0], hh[1], hh[2], hh[3], hh[4], hh[5]);
}

// ---- the chunk tables as plain arithmetic (declared in internal.h: the bwts_debug_chunk_plan test hook asks them too) ----
u32 chunk_nominal_size(u64 a, u32 target)
{
    // about `target` chunks (CH_CHUNK_TARGET = 16 K unless the test switch BWTS_CHUNK_TARGET says otherwise), between one and eight tiles each
    u64 s = (a / target + 1023) / 1024 * 1024;
    if (s < CH_TILE) s = CH_TILE;
    if (s > 8 * CH_TILE) s = 8 * CH_TILE;
    return (u32)s;
}
// Entries of cstart/ccount/mvcount/cwide/coff, fixed when their block is reserved.  They hold every run the driver can make:
//   * the store has tail <= a0 slots in use (the driver fails on c.tail + m_exit > a0), and every cut_chunks(lo, hi) adds
//     ceil((hi - lo) / S) chunks over slots of its own;
//   * S changes only at a compaction, which starts the tables over at 0 with tail = a_chunks; between two compactions nchunks never
//     falls, and S >= CH_TILE always.  So between compactions nchunks <= tail / S + cuts <= a0 / CH_TILE + cuts;
//   * the cuts between two compactions are at most one first cut or re-cut, one first split of the big list and one append per round,
//     and the rounds are capped (more than 80 fails): fewer than CH_CUT_SLACK.
// A capacity sized by the FIRST cut's S (a0 / S(a0) + 1024, what this was) does not: after a re-cut at a nominal size up to 8x
// smaller, a list that the big list still dominates appends more chunks than that held.  "chunk table full" on the byte planes of a
// smooth float32 field from 2^29 bytes on was this: a0 = 254 419 860 cut at S = 16 384, 16 552 entries; 5 887 411 elements left of
// 85 722 238 slots re-cut into 2875 chunks of 2048; then 11.2 M and 18.4 M elements left the big list in two rounds, 17 328 chunks.
// 17 bytes per entry: ~35 MB at a0 = 2^32, beside a store of more than 100 GB.
u64 chunk_table_capacity(u64 a0) { return a0 / CH_TILE + CH_CUT_SLACK; }
// A compaction re-cuts the a_chunks <= a0 elements left by their own nominal size S' >= CH_TILE: ceil(a_chunks / S') <= a0 / CH_TILE + 1
// chunks, which always fit.
ChunkRecut chunk_recut_plan(u64 a_chunks, u32 target)
{
    ChunkRecut r;
    r.S = chunk_nominal_size(a_chunks, target);
    r.nc = (a_chunks + r.S - 1) / r.S;
    return r;
}

// The big list: idx/head ping-pong (cur = the side that holds it), the regrouped copy, two pairs of sort buffers, the second key word.
struct BigList {
    u32 *idx[2], *head[2], *t_idx, *t_head, *bv[2], *sv1;
    u64 *bk[2], *k23, *sk1;
    u8 *flags;
    u64 m = 0, groups = 0;          // elements; groups: the ordinals of a round's sort key lie below it
    int cur = 0;
};
// What the stages of chunk_rounds share: the list store with its chunk tables, and the big list
struct ChunkRun {
    bool trace;                     // BWTS_ROUND_TRACE=1
    u32 rounds;
    int rb;
    PrevSym prev;
    u8 *out;
    u64 *slots;                     // CH_SLOTS result slots in d_small
    u32 *st_idx, *st_head, *alt_idx, *alt_head;     // the store, and its other pair of arrays (chunk_compact_kernel)
    u64 *mv;
    u32 *cstart, *ccount, *mvcount, *coff;          // (coff: the chunks' offsets in the dense list of a compaction)
    u8 *cwide;
    u32 S, nchunks = 0;             // nominal chunk size; chunks in the tables
    u32 target = CH_CHUNK_TARGET;   // chunks a cut aims at (test switch BWTS_CHUNK_TARGET)
    u64 maxchunks, tail = 0;        // chunk_table_capacity(); slots of the store in use: chunks leaving the big list are appended there
    bool wide_possible = false;     // some chunk may be flagged WIDE: the second instantiation is launched as well
    BigList b;
};

#define CH_TRY(call) do { const int rc__ = (call); if (rc__ != BWTS_OK) { if (c.trace) fprintf(stderr, "[chunks] line %d: rc %d\n", __LINE__, rc__); return rc__; } } while (0)
#define CH_HIP(call) do { const hipError_t e__ = (call); if (e__ != hipSuccess) { ctx->last_hip = (int)e__; if (c.trace) fprintf(stderr, "[chunks] line %d: hip error %d\n", __LINE__, (int)e__); return BWTS_E_HIP; } } while (0)
#define CH_FAIL(why) do { if (c.trace) fprintf(stderr, "[chunks] invariant: %s (round %u)\n", why, c.rounds); return BWTS_E_INTERNAL; } while (0)

// Every launch of chunk_init_kernel: list slots [lo, hi) of the store become chunks first_chunk, first_chunk + 1, ... of the nominal size
// (the first cut and the re-cut after a compaction start the tables over at 0; an append goes behind the last chunk).
// wide: the new chunks may hold groups of up to CH_GROUP_MAX members.
static int cut_chunks(bwts_ctx *ctx, ChunkRun &c, u64 lo, u64 hi, u32 first_chunk, bool wide)
{
    const u32 add = (u32)((hi - lo + c.S - 1) / c.S);
    if ((u64)first_chunk + add > c.maxchunks) CH_FAIL("chunk table full");
    chunk_init_kernel<<<dim3((add + 3) / 4), dim3(256), 0, ctx->stream>>>(c.st_head, lo, hi, c.S, first_chunk, add, c.cstart, c.ccount, c.mvcount, c.cwide, wide);
    if (wide) c.wide_possible = true;
    CH_HIP(hipGetLastError());
    c.nchunks = first_chunk + add;
    c.tail = hi;
    return BWTS_OK;
}

// The one-off order: group records sorted by the group's smallest position, members copied to their places in the store; the larger
// groups' members compacted behind them (see go_write_kernel).  ob: the order block of ob_bytes, cut here as group records.
// *a_small: elements of the smaller groups.
static int chunk_order(bwts_ctx *ctx, ChunkRun &c, u64 n, SortSpace &sp, const ActiveList &cur, u64 a0, u32 *SA, char *ob, size_t ob_bytes, u64 *a_small)
{
    const u64 tiles = (a0 + DG_OWN - 1) / DG_OWN;
    const bool pairs = n <= 0x80000000ull;                        // (positions and list indices below 2^31)
    const u64 gmax = a0 / 2 + 1;                                  // a group has at least two members
    // records and their sort buffers (2 x 8 + 3 x 4 bytes per group <= 14 bytes per element), tile counts behind
    u64 *rk[2], *tcount;
    u32 *rv[2], *doff;
    BlockLayout G;
    G.array(&rk[0], gmax); G.array(&rk[1], gmax); G.array(&rv[0], gmax); G.array(&rv[1], gmax); G.array(&doff, gmax); G.array(&tcount, tiles + 1);
    if (!G.place_within(ob, ob_bytes)) CH_FAIL("order block too small");
    {
        SpanGuard g(ctx, BWTS_K_RERANK, a0, 14 * a0);
        go_count_kernel<<<dim3((unsigned)tiles), dim3(DG_THREADS), 0, ctx->stream>>>(cur.idx, cur.head, a0, tcount);
        CH_HIP(hipMemsetAsync(tcount + tiles, 0, sizeof(u64), ctx->stream));
        ScanLoadArr<u64> tin{tcount};
        ScanStoreArr<u64> tout{tcount};
        CH_TRY((device_scan<false, u64>(ctx, tiles + 1, tin, tout, OpAdd(), (u64)0, sp.scan_temp)));
        CH_HIP(hipMemcpyAsync(c.slots + CHS_TOTAL, tcount + tiles, sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream));
        go_write_kernel<<<dim3((unsigned)tiles), dim3(DG_THREADS), 0, ctx->stream>>>(cur.idx, cur.head, a0, tcount, tiles, rk[0], rv[0], c.st_idx, c.st_head, pairs);
        CH_HIP(hipGetLastError());
    }
    CH_TRY(read_small(ctx, SM_CHSLOT, CH_SLOT_WORDS));
    const u64 tot = ctx->h_small[SM_CHSLOT + CHS_TOTAL];
    const u64 groups = (u32)tot, bigs = tot >> 32;
    if (bigs > a0 || groups > gmax) CH_FAIL("group records");
    *a_small = a0 - bigs;
    if (groups) {
        const SortPlan op = sort_plan(rk[0], rk[1], rv[0], rv[1], sp.tile_hist, sp.scan_temp);
        int ores = 0;
        const int pb = bitlen_u64(n - 1);
        CH_TRY(radix_sort_pairs(ctx, op, groups, pb < 1 ? 1 : pb, &ores));
        SpanGuard g(ctx, BWTS_K_RERANK, *a_small, 20 * *a_small);
        const unsigned gblocks = (unsigned)((groups + 255) / 256);
        GoSizeIn zin{rk[ores], rv[ores], pairs};
        ScanStoreArr<u32> zout{doff};
        CH_TRY((device_scan<false, u32>(ctx, groups, zin, zout, OpAdd(), 0u, sp.scan_temp)));
        go_expand_kernel<<<dim3(gblocks), dim3(256), 0, ctx->stream>>>(rk[ores], rv[ores], doff, groups, SA, c.st_idx, c.st_head, pairs);
        CH_HIP(hipGetLastError());
    }
    return BWTS_OK;
}

// The big list's buffers, in side arena 1 (the order sort's block, free again), and the list itself: the m elements that
// go_write_kernel left behind the smaller groups.  BWTS_E_NOMEM: no room (nothing was written).
static int big_list_setup(bwts_ctx *ctx, ChunkRun &c, u64 m, u64 a_small)
{
    BigList &b = c.b;
    char *bb = nullptr;
    BlockLayout L;
    for (int i = 0; i < 2; i++) { L.array(&b.idx[i], m); L.array(&b.head[i], m); }
    L.array(&b.t_idx, m); L.array(&b.t_head, m); L.array(&b.bv[0], m); L.array(&b.bv[1], m); L.array(&b.sv1, m);
    L.array(&b.bk[0], m); L.array(&b.bk[1], m); L.array(&b.k23, m); L.array(&b.sk1, m); L.array(&b.flags, m);
    const bool deny = [ctx] { const char *e = bwts_knob(ctx, "BWTS_BIGLIST_NOMEM"); return e && atoi(e) == 1; }();      // (test switch)
    const int rc = deny ? BWTS_E_NOMEM : aux_reserve_slot(ctx, 1, L.bytes(), &bb);
    if (rc == BWTS_E_NOMEM) return rc;
    CH_TRY(rc);
    L.place(bb);
    b.m = m;
    CH_HIP(hipMemcpyAsync(b.idx[0], c.st_idx + a_small, m * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
    CH_HIP(hipMemcpyAsync(b.head[0], c.st_head + a_small, m * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
    return BWTS_OK;
}

// The one-off order left every group of more than CH_CAP members in the big list; those of up to CH_GROUP_MAX go to chunks right
// away (unordered, like everything that leaves the big list later): their chunks are flagged WIDE and take the sorting instantiation of the round kernel
static int big_list_first_split(bwts_ctx *ctx, ChunkRun &c, SortSpace &sp, u64 a0, u64 *a_chunks)
{
    BigList &b = c.b;
    CH_HIP(hipMemsetAsync(c.slots, 0, CH_SLOT_WORDS * sizeof(u64), ctx->stream));
    {
        SpanGuard g(ctx, BWTS_K_RERANK, b.m, 28 * b.m);
        BlRunIn nin{b.head[0]};
        BlRunOut nout{b.head[0], b.m, b.bv[0], b.bv[1]};
        CH_TRY((device_scan<true, u32>(ctx, b.m, nin, nout, OpMax(), 0u, sp.scan_temp)));
        if (c.trace) bl_diag_sizes(ctx, b.bv[0], b.bv[1], b.m, "groups of more than 256 after round 0");
        BlSplitIn sin{b.bv[0], b.bv[1]};
        BlSplitOut sout{b.bv[0], b.bv[1], b.idx[0], b.head[0], b.m, c.st_idx + c.tail, c.st_head + c.tail, b.idx[1], b.head[1], (unsigned long long *)c.slots};
        CH_TRY((device_scan<false, u64>(ctx, b.m, sin, sout, OpAdd(), (u64)0, sp.scan_temp)));
    }
    CH_TRY(read_small(ctx, SM_CHSLOT, CH_SLOT_WORDS));
    const u64 m_exit = ctx->h_small[SM_CHSLOT + CHS_EXIT], m_stay = ctx->h_small[SM_CHSLOT + CHS_STAY];
    b.groups = ctx->h_small[SM_CHSLOT + CHS_BIGGROUPS];
    { u64 *rep = fwd_report_of(ctx); rep[FC_M_EXIT] = m_exit; rep[FC_M_STAY] = m_stay; rep[FC_GROUPS] = b.groups; }
    if (m_exit + m_stay != b.m || c.tail + m_exit > a0 || b.groups * (CH_GROUP_MAX + 1) > m_stay) CH_FAIL("first split of the big list");
    if (m_exit) {
        CH_TRY(cut_chunks(ctx, c, c.tail, c.tail + m_exit, c.nchunks, true));
        *a_chunks += m_exit;
    }
    b.cur = 1;
    b.m = m_stay;
    if (c.trace) fprintf(stderr, "[chunks] groups of up to %d members leave the big list at once: %llu elements, %llu stay\n", (int)CH_GROUP_MAX,
                         (unsigned long long)m_exit, (unsigned long long)m_stay);
    return BWTS_OK;
}

// A round of the big list, first half: its gathers read the same version of the ranks as the chunks', before the moves are applied
template <bool CYCLIC>
static int big_list_gather(bwts_ctx *ctx, ChunkRun &c, SortSpace &sp, u64 n, u64 h, const u32 *d_fstart, u64 k)
{
    BigList &b = c.b;
    SpanGuard g(ctx, BWTS_K_RERANK, b.m, 30 * b.m);
    BlIn fin{b.head[b.cur]};
    BlOut<CYCLIC> fout{b.head[b.cur], b.idx[b.cur], c.rb, sp.rank, n, h, d_fstart, k, b.bk[0], b.bv[0], b.k23, b.bk[1], b.bv[1]};
    CH_TRY((device_scan<false, u32>(ctx, b.m, fin, fout, OpAdd(), 0u, sp.scan_temp)));
    if (c.trace) {
        const u64 gcap = b.m / (CH_GROUP_MAX + 1) + 2;
        u8 *df = nullptr; unsigned long long hc[3] = {0, 0, 0};
        if (hipMalloc((void **)&df, 2 * gcap + 32) == hipSuccess) {
            (void)hipMemsetAsync(df, 0, 2 * gcap + 32, ctx->stream);
            unsigned long long *dc = (unsigned long long *)(df + ((2 * gcap + 7) & ~7ull));
            const unsigned gb = (unsigned)((b.m + 255) / 256);
            bl_diag_flag_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(b.bk[0], b.k23, b.m, c.rb, df, df + gcap);
            bl_diag_count_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(b.bk[0], b.m, c.rb, df, df + gcap, dc);
            (void)hipMemcpyAsync(hc, dc, sizeof(hc), hipMemcpyDeviceToHost, ctx->stream);
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipFree(df);
            fprintf(stderr, "[chunks] big list at h %llu: %llu elements in %llu groups; in groups with one rank at h: %llu, with one rank triple (cannot split): %llu\n",
                    (unsigned long long)h, (unsigned long long)b.m, hc[2], hc[0], hc[1]);
        }
    }
    return BWTS_OK;
}

// ... second half: the two-word sort, subgroup flags, regrouping (ranks, emission), and the split into what stays (the list's other
// side) and what leaves for the store's tail
static int big_list_sort_split(bwts_ctx *ctx, ChunkRun &c, SortSpace &sp, unsigned long long *res)
{
    BigList &b = c.b;
    const int big_bits = (b.groups > 1 ? bitlen_u64(b.groups - 1) : 1) + c.rb;          // ordinals < groups
    if (big_bits > 64) return BWTS_E_RANGE;
    const u64 *sorted_keys = nullptr;
    const u32 *src = nullptr;
    CH_TRY(two_word_sort(ctx, sp, b.bk, b.bv[1], b.sk1, b.sv1, b.m, c.rb, big_bits, &sorted_keys, &src));
    SpanGuard g(ctx, BWTS_K_RERANK, b.m, 60 * b.m);
    bl_flags_kernel<<<dim3((unsigned)((b.m + 255) / 256)), dim3(256), 0, ctx->stream>>>(sorted_keys, src, b.k23, b.bv[0], b.m, c.rb, b.flags, b.t_idx);
    CH_HIP(hipGetLastError());
    // (the sort buffers are free again: subgroup starts and sizes go there)
    BlFlagIn rin{b.flags};
    BlRegroupOut rout{b.flags, b.head[b.cur], b.m, b.t_idx, b.t_head, sp.rank, c.prev, c.out, res, b.bv[0], b.bv[1]};
    CH_TRY((device_scan<true, u64>(ctx, b.m, rin, rout, OpMax2(), (u64)0, sp.scan_temp)));
    if (c.trace) bl_diag_sizes(ctx, b.bv[0], b.bv[1], b.m, "big list regrouped");
    BlSplitIn sin{b.bv[0], b.bv[1]};
    BlSplitOut sout{b.bv[0], b.bv[1], b.t_idx, b.t_head, b.m, c.st_idx + c.tail, c.st_head + c.tail, b.idx[b.cur ^ 1], b.head[b.cur ^ 1], res};
    CH_TRY((device_scan<false, u64>(ctx, b.m, sin, sout, OpAdd(), (u64)0, sp.scan_temp)));
    return BWTS_OK;
}

// The chunks are two thirds empty: a dense list in the store's other pair of arrays, cut into new chunks (chunk_compact_kernel).
// The new chunks always fit the tables (chunk_table_capacity).
static int compact_chunks(bwts_ctx *ctx, ChunkRun &c, u64 a_chunks)
{
    const ChunkRecut re = chunk_recut_plan(a_chunks, c.target);
    fwd_report_of(ctx)[FC_COMPACTIONS]++;
    SpanGuard g(ctx, BWTS_K_ROUND, 0, 0);
    chunk_total_kernel<<<dim3(1), dim3(1024), 0, ctx->stream>>>(c.ccount, c.nchunks, (unsigned long long *)(c.slots + 3 * CH_SLOT_WORDS), c.coff);
    chunk_compact_kernel<<<dim3(c.nchunks), dim3(256), 0, ctx->stream>>>(c.st_idx, c.st_head, c.cstart, c.ccount, c.coff, c.alt_idx, c.alt_head);
    { u32 *t = c.st_idx; c.st_idx = c.alt_idx; c.alt_idx = t; t = c.st_head; c.st_head = c.alt_head; c.alt_head = t; }
    if (c.trace) fprintf(stderr, "[chunks] list compacted: %llu elements of %llu slots, %u chunks -> %u (nominal chunk %u)\n", (unsigned long long)a_chunks,
                         (unsigned long long)c.tail, c.nchunks, (u32)re.nc, re.S);
    c.S = re.S;
    fwd_report_of(ctx)[FC_S_RECUT] = re.S;
    return cut_chunks(ctx, c, 0, a_chunks, 0, c.wide_possible);
}

// After the last round: the suffix array when someone reads it, and with a stable partition the groups of equal infinite words
static int chunk_finish(bwts_ctx *ctx, ChunkRun &c, SortSpace &sp, u64 n, u32 *SA, bool need_sa, bool stable, u64 a_chunks)
{
    BigList &b = c.b;
    if (need_sa) CH_TRY(sa_from_ranks(ctx, sp.rank, n, SA));
    if (stable) {
        // (a round enqueued behind the stable one has split nothing either: the lists are what they were)
        SpanGuard g(ctx, BWTS_K_EMIT, a_chunks + b.m, 10 * (a_chunks + b.m));
        fwd_report_of(ctx)[FR_REST_CHUNKS] = c.nchunks ? a_chunks : 0;
        fwd_report_of(ctx)[FR_REST_BIG] = b.m;
        if (c.nchunks && a_chunks) {
            chunk_rest_records_kernel<<<dim3(c.nchunks), dim3(256), 0, ctx->stream>>>(c.st_idx, c.st_head, c.cstart, c.ccount, c.mv, c.mvcount);
            chunk_apply_records_kernel<1><<<dim3(c.nchunks), dim3(256), 0, ctx->stream>>>(c.mv, c.cstart, c.mvcount, RecordTargets{sp.rank, c.prev, c.out, need_sa ? SA : nullptr});
            CH_HIP(hipGetLastError());
        }
        if (b.m) {
            DgRestIn rin{b.head[b.cur]};
            DgRestOut rout{b.idx[b.cur], b.head[b.cur], c.prev, c.out, need_sa ? SA : nullptr};
            CH_TRY((device_scan<true, u32>(ctx, b.m, rin, rout, OpMax(), 0u, sp.scan_temp)));
        }
    }
    return BWTS_OK;
}

// Same contract as dense_rounds().  *handled = false: this form does not apply (short list, no room) and nothing was changed.
template <bool CYCLIC>
static int chunk_rounds(bwts_ctx *ctx, const u8 *d_T, u64 n, const Alphabet &al, const u32 *d_fstart, u64 k, SortSpace &sp,
                        ActiveList cur, u64 a0, u32 *SA, bool need_sa, u32 *rounds_io, bool *handled)
{
    *handled = false;
    u64 *rep = fwd_report_of(ctx);
    if (a0 > 0xffffffffull || a0 < CH_MIN_LIST) { rep[FR_NO_CHUNKS] = FR_NC_SHORT; return BWTS_OK; }
    ChunkRun c{[ctx] { const char *e = bwts_knob(ctx, "BWTS_ROUND_TRACE"); return e && atoi(e) == 1; }(), *rounds_io,
               CYCLIC ? bitlen_u64(n - 1) : bitlen_u64(n), PrevSym{sp.carry_src, d_T, n, d_fstart, k}, CYCLIC ? sp.carry_out : nullptr,
               ctx->d_small + SM_CHSLOT};
    BigList &b = c.b;
    if (const char *e = bwts_knob(ctx, "BWTS_CHUNK_TARGET")) { const int v = atoi(e); if (v >= 16 && v <= CH_CHUNK_TARGET) c.target = (u32)v; }      // (test switch)
    c.S = chunk_nominal_size(a0, c.target);
    c.maxchunks = chunk_table_capacity(a0);
    char *base = nullptr, *ob = nullptr;
    BlockLayout L;
    L.array(&c.st_idx, a0); L.array(&c.st_head, a0); L.array(&c.mv, a0);
    L.array(&c.cstart, c.maxchunks + 1); L.array(&c.ccount, c.maxchunks + 1); L.array(&c.mvcount, c.maxchunks + 1); L.array(&c.cwide, c.maxchunks + 1);
    L.array(&c.coff, c.maxchunks + 1); L.array(&c.alt_idx, a0); L.array(&c.alt_head, a0);
    int rc = aux_reserve(ctx, L.bytes(), &base);
    if (rc == BWTS_E_NOMEM) { rep[FR_NO_CHUNKS] = FR_NC_STORE; return BWTS_OK; }
    CH_TRY(rc);
    // the order block: what the order sort of dense_rounds takes, two key and two value buffers of the whole list
    const size_t ob_bytes = 2 * BlockLayout::padded<u64>(a0) + 2 * BlockLayout::padded<u32>(a0);
    rc = aux_reserve_slot(ctx, 1, ob_bytes, &ob);
    if (rc == BWTS_E_NOMEM) { rep[FR_NO_CHUNKS] = FR_NC_ORDER; return BWTS_OK; }
    CH_TRY(rc);
    rep[FR_NO_CHUNKS] = FR_NC_NA;
    *handled = true;
    L.place(base);

    u64 a_small = 0;
    CH_TRY(chunk_order(ctx, c, n, sp, cur, a0, SA, ob, ob_bytes, &a_small));
    if (c.trace) fprintf(stderr, "[chunks] list %llu: in chunks %llu (nominal chunk %u), big list %llu\n", (unsigned long long)a0,
                         (unsigned long long)a_small, c.S, (unsigned long long)(a0 - a_small));
    rep[FC_S] = c.S; rep[FC_MAXCHUNKS] = c.maxchunks; rep[FC_A_SMALL] = a_small; rep[FC_BIG0] = a0 - a_small;
    rep[FC_FSL] = CYCLIC && k <= CH_FS;
    if (a0 - a_small) {
        // (nothing outside this function's own buffers has been written so far: without room for the big list the tile form takes over,
        // as it does when the first two blocks do not fit)
        rc = big_list_setup(ctx, c, a0 - a_small, a_small);
        if (rc == BWTS_E_NOMEM) {
            if (c.trace) fprintf(stderr, "[chunks] no room for the big list (%llu elements): the tile form takes over\n", (unsigned long long)(a0 - a_small));
            *handled = false;
            rep[FR_NO_CHUNKS] = FR_NC_BIGLIST;
            memset(rep + FC_S, 0, (FWD_HEADER_WORDS - FC_S) * sizeof(u64));       // (the chunk words describe a chunk run: this is none)
            return BWTS_OK;
        }
        if (rc != BWTS_OK) return rc;
    }
    // ---- chunks over the smaller groups ----
    // (the larger groups' members, which go_write_kernel left at [a_small, a0), are in the big list's own buffers by now: the store
    // behind the smaller groups is free, chunks leaving the big list are appended there)
    c.tail = a_small;
    if (a_small) CH_TRY(cut_chunks(ctx, c, 0, a_small, 0, false));
    u64 a_chunks = a_small;                 // elements in chunks after the last evaluated round
    if (b.m) CH_TRY(big_list_first_split(ctx, c, sp, a0, &a_chunks));

    u64 h = (u64)al.hstep;
    bool finished = false, stable = false;
    while (!finished) {
#ifdef CH_PROFILE
        const int B = 1;
#else
        const int B = b.m ? 1 : 2;        // rounds per host round trip
#endif
        CH_HIP(hipMemsetAsync(c.slots, 0, CH_SLOTS * CH_SLOT_WORDS * sizeof(u64), ctx->stream));
        u64 hs[CH_SLOTS];
        for (int r = 0; r < B; r++) {
            unsigned long long *res = (unsigned long long *)(c.slots + r * CH_SLOT_WORDS);
            hs[r] = h;
            if (c.trace && c.nchunks) chunk_diag_sizes(ctx, c.st_head, c.cstart, c.ccount, c.nchunks, c.rounds + 1);
            if (c.nchunks) {
                SpanGuard g(ctx, BWTS_K_ROUND, 0, 0);          // (elements and bytes are added below, once the round's true size is known)
#define CH_LAUNCH(FS, WD) chunk_round_kernel<CYCLIC, 3, FS, WD><<<dim3(c.nchunks), dim3(CH_THREADS), 0, ctx->stream>>>(c.st_idx, c.st_head, c.cstart, c.ccount, c.cwide, c.mv, c.mvcount, \
                                                                                                  sp.rank, n, h, d_fstart, k, c.prev, c.out, res)
                const bool fsl = CYCLIC && k <= CH_FS;
                if (fsl) CH_LAUNCH(CYCLIC, false); else CH_LAUNCH(false, false);
                if (c.wide_possible) {
                    // (behind the other one: a chunk whose last large group has just split is taken over in the NEXT round)
                    if (fsl) CH_LAUNCH(CYCLIC, true); else CH_LAUNCH(false, true);
                }
#undef CH_LAUNCH
                CH_HIP(hipGetLastError());
            }
            if (b.m) CH_TRY((big_list_gather<CYCLIC>(ctx, c, sp, n, h, d_fstart, k)));
            if (c.nchunks) {
                SpanGuard g(ctx, BWTS_K_ROUND, 0, 0);
                chunk_apply_records_kernel<0><<<dim3(c.nchunks), dim3(256), 0, ctx->stream>>>(c.mv, c.cstart, c.mvcount, RecordTargets{sp.rank, c.prev, c.out, nullptr});
                chunk_total_kernel<<<dim3(1), dim3(1024), 0, ctx->stream>>>(c.ccount, c.nchunks, res, nullptr);
                CH_HIP(hipGetLastError());
            }
            if (b.m) CH_TRY(big_list_sort_split(ctx, c, sp, res));
            h = h > (1ull << 60) ? h : h << 2;        // the step is quadrupled per round
        }
        CH_TRY(read_small(ctx, SM_CHSLOT, CH_SLOTS * CH_SLOT_WORDS));
        for (int q = 0; q < B; q++) {
            const u64 *r = ctx->h_small + SM_CHSLOT + q * CH_SLOT_WORDS;
            // 32 algorithmic bytes per list element and round: position + head in, three successor ranks, position + head out, rank update
            if (c.nchunks) { ctx->tm.k[BWTS_K_ROUND].elems += a_chunks; ctx->tm.k[BWTS_K_ROUND].alg_bytes += 32 * a_chunks; }
            if (finished) { rep[FC_ENQUEUED_BEHIND_LAST] = 1; continue; }        // (a round enqueued behind the last one: it ran, over what was left, and changed nothing)
            c.rounds++;
            if (r[CHS_ERR]) {
                if (c.trace) fprintf(stderr, "[chunks] chunk %llu of %u: group [%d, %d) plen %llu len %llu rp %llu slot %llu\n", (unsigned long long)r[5] - 1, c.nchunks,
                                     (int)(r[6] >> 32), (int)(u32)r[6], (unsigned long long)(r[7] >> 48), (unsigned long long)((r[7] >> 32) & 0xffff),
                                     (unsigned long long)((r[7] >> 16) & 0xffff), (unsigned long long)(r[7] & 0xffff));
                CH_FAIL("a chunk met a group larger than it may hold");
            }
            const u64 in_chunks = c.nchunks ? r[CHS_TOTAL] : 0;
            u64 m_exit = 0, m_stay = 0;
            if (b.m) {
                m_exit = r[CHS_EXIT]; m_stay = r[CHS_STAY];
                b.groups = r[CHS_BIGGROUPS];
                if (m_exit + m_stay > b.m || c.tail + m_exit > a0 || b.groups * (CH_GROUP_MAX + 1) > m_stay) CH_FAIL("big list split counts");
            }
            if (in_chunks > a_chunks) CH_FAIL("chunks grew");
#ifdef CH_PROFILE
            if (c.trace && q == 0) {
                (void)hipMemcpy(ctx->h_small + SM_CHSLOT + 64, ctx->d_small + SM_CHSLOT + 64, 64 * 8 * sizeof(u64), hipMemcpyDeviceToHost);
                double ph[6] = {0, 0, 0, 0, 0, 0}, tot = 0;
                for (int w = 0; w < 64; w++) for (int i = 0; i < 6; i++) ph[i] += (double)ctx->h_small[SM_CHSLOT + 64 + 8 * w + i];
                for (int i = 0; i < 6; i++) tot += ph[i];
                fprintf(stderr, "[chunks] phase shares: load %.1f%% detect %.1f%% gather %.1f%% count %.1f%% emit/moves %.1f%% write %.1f%%  (cycles per element %.2f)\n", 100 * ph[0] / tot, 100 * ph[1] / tot,
                        100 * ph[2] / tot, 100 * ph[3] / tot, 100 * ph[4] / tot, 100 * ph[5] / tot, tot / (double)(a_chunks ? a_chunks : 1));
                (void)hipMemset(ctx->d_small + SM_CHSLOT + 64, 0, 64 * 8 * sizeof(u64));
            }
#endif
            if (c.trace) fprintf(stderr, "[chunks] round %u h %llu: chunks %llu -> %llu, big list %llu -> stays %llu, leaves %llu\n", c.rounds,
                                 (unsigned long long)hs[q], (unsigned long long)a_chunks, (unsigned long long)in_chunks, (unsigned long long)b.m, (unsigned long long)m_stay, (unsigned long long)m_exit);
            if (u64 *rr = fwd_report_round(ctx, c.rounds)) {
                rr[FRR_FORM] = FR_FORM_CHUNKS; rr[FRR_H] = hs[q]; rr[FRR_IN] = a_chunks + b.m; rr[FRR_OUT] = in_chunks + m_exit + (b.m ? m_stay : 0);
                rr[FRR_SPLITS] = r[CHS_SPLIT]; rr[FRR_CHUNKS_IN] = a_chunks; rr[FRR_CHUNKS_OUT] = in_chunks; rr[FRR_BIG_IN] = b.m;
                rr[FRR_BIG_STAYS] = m_stay; rr[FRR_BIG_LEAVES] = m_exit; rr[FRR_NCHUNKS] = c.nchunks; rr[FRR_CHUNK_S] = c.S;
            }
            if (m_exit) CH_TRY(cut_chunks(ctx, c, c.tail, c.tail + m_exit, c.nchunks, true));
            if (b.m) { b.cur ^= 1; b.m = m_stay; }
            a_chunks = in_chunks + m_exit;
            const u64 left = a_chunks + b.m;
            rep[FR_LEFT] = left;
            rep[FR_END] = left == 0 ? FR_END_EMPTY : CYCLIC && r[CHS_SPLIT] == 0 ? FR_END_STABLE : FR_END_NONE;
            if (CYCLIC && c.rounds - 1 < BWTS_MAX_ROUND_STATS) ctx->tm.round_active[c.rounds - 1] = left;
            if (left == 0) { finished = true; continue; }
            // no group split: the partition is stable under doubling -- what is left are groups of equal infinite words
            if (CYCLIC && r[CHS_SPLIT] == 0) {
                if (c.trace) fprintf(stderr, "[chunks] round %u: no group split, %llu elements left in groups of equal infinite words\n", c.rounds, (unsigned long long)left);
                finished = true; stable = true; continue;
            }
            if (!CYCLIC && hs[q] >= n) CH_FAIL("suffixes still tied at h >= n");      // suffixes are distinct; cannot happen
            if (c.rounds > 80) CH_FAIL("more than 80 rounds");
        }
        if (!finished && c.nchunks >= 64 && a_chunks > 0 && a_chunks * 3 < c.tail) CH_TRY(compact_chunks(ctx, c, a_chunks));
    }
    rep[FC_WIDE_POSSIBLE] = c.wide_possible;
    CH_TRY(chunk_finish(ctx, c, sp, n, SA, need_sa, stable, a_chunks));
    *rounds_io = c.rounds;
    return BWTS_OK;
}
#undef CH_FAIL
#undef CH_TRY
#undef CH_HIP
