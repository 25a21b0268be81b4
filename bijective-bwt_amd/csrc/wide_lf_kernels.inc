// wide_lf_kernels.inc -- the n > 2^32 inverse's kernels that read LF, included twice by wide_inverse.h: once for the full form, once
// for the compact one.  The includer defines
//   WI_KERNEL(name)   the kernel's name (name##_wide_kernel, name##_c40_kernel)
//   WI_LFW            the word LF is read as through lf_at (u64: one entry per word; u32: packed 40-bit entries)
//   WI_GL             log2 of the splitter spacing
//   WI_MARKW, WI_MARK(m, x), WI_UNMARKED(m, i)   the byte-map fallback's marks: their word, setting one, testing one

// walk_record_kernel of the main path with 64-bit elements and marks (see there for the scheme)
// MOM: no marks; the unreached elements come from per-range moments (inverse.hip, MARK_MOMENTS) over WMOM_BUCKETS ranges kept in
// dynamic LDS (80 KB: two workgroups per CU) -- the random byte write per step was what held this walk at half the main path's rate
template <bool MOM>
__global__ __launch_bounds__(256) void WI_KERNEL(walk_record)(const WI_LFW *__restrict__ LF, WI_MARKW *__restrict__ marks, u64 s, u64 node_cap, u32 slot,
                                                               const u64 *__restrict__ Cg, u8 *__restrict__ seg, WiNode *__restrict__ nodes,
                                                               unsigned long long *__restrict__ ticket, unsigned long long *__restrict__ vcount,
                                                               unsigned long long *__restrict__ overflow, int mom_shift, unsigned long long *__restrict__ mom)
{
    __shared__ u64 Ctab[257];
    extern __shared__ __attribute__((aligned(16))) unsigned long long wmom_sm[];        // MOM: sums, sums of squares, counts
    unsigned long long *msum = wmom_sm, *msq = wmom_sm + WMOM_BUCKETS;
    u32 *mcnt = (u32 *)(wmom_sm + 2 * WMOM_BUCKETS);
    if (MOM) for (u32 b = threadIdx.x; b < WMOM_BUCKETS; b += 256) { mcnt[b] = 0; msum[b] = 0; msq[b] = 0; }
    for (int i = threadIdx.x; i < 257; i += 256) Ctab[i] = Cg[i];
    __syncthreads();
    const u64 gmask = (1ull << WI_GL) - 1ull;
    bool have = false, done = false;
    u64 my = 0, x = 0, mn = 0;
    u32 len = 0, mnoff = 0;
    u32 sb[16];                  // 64 recorded symbols, stored as one 64-byte block (see walk_record_kernel)
#pragma unroll
    for (int q = 0; q < 16; q++) sb[q] = 0;
    u64 bnext = 0, bend = 0;
    bool exhausted = false;
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
            }
            if (!have && !done) {
                const u64 id = bnext + (u64)__popcll(need & lanemask_lt());
                if (id < bend) {
                    have = true; my = id; x = my << WI_GL; len = 0; mn = x; mnoff = 0;
#pragma unroll
                    for (int q = 0; q < 16; q++) sb[q] = 0;
                }
                else if (exhausted) done = true;
            }
            const u64 taken = bnext + (u64)__popcll(need);
            bnext = taken < bend ? taken : bend;
        }
        if (__ballot(have || !done) == 0) break;
        if (have) {
            const u64 y = lf_at(LF, x);
            if (MOM) {
                const u32 b = (u32)x & (WMOM_BUCKETS - 1u);                  // residue classes (see inverse.hip, MARK_MOMENTS)
                const unsigned long long o = x >> WMOM_LOG2;
                atomicAdd(&mcnt[b], 1u); atomicAdd(&msum[b], o); atomicAdd(&msq[b], o * o);
            } else WI_MARK(marks, x);
            {
                const u32 sh = symbol_of64(Ctab, y) << (8 * (len & 3u));
                const u32 w = (len >> 2) & 15u;
#pragma unroll
                for (int q = 0; q < 16; q++) sb[q] |= w == (u32)q ? sh : 0u;
            }
            if ((len & 63u) == 63u) {
                uint4 *d = (uint4 *)(seg + my * slot + (len & ~63u));
#pragma unroll
                for (int q = 0; q < 4; q++) d[q] = make_uint4(sb[4 * q], sb[4 * q + 1], sb[4 * q + 2], sb[4 * q + 3]);
#pragma unroll
                for (int q = 0; q < 16; q++) sb[q] = 0;
            }
            len++;
            x = y;
            const bool at_splitter = (x & gmask) == 0;
            if (at_splitter || len == slot) {
                if (len & 63u) {
                    uint4 *d = (uint4 *)(seg + my * slot + (len & ~63u));
                    const u32 rem = len & 63u;
#pragma unroll
                    for (int q = 0; q < 4; q++) if ((u32)q * 16u < rem) d[q] = make_uint4(sb[4 * q], sb[4 * q + 1], sb[4 * q + 2], sb[4 * q + 3]);
                }
                u64 next_node;
                if (at_splitter) { next_node = x >> WI_GL; have = false; }
                else {
                    next_node = s + atomicAdd(vcount, 1ull);
                    if (next_node >= node_cap) { atomicAdd(overflow, 1ull); next_node = node_cap - 1; }
                }
                WiNode nd; nd.nxt = (u32)next_node; nd.len = len; nd.mn = mn; nd.off = mnoff; nd.pad = 0;
                nodes[my] = nd;
                if (!at_splitter) {
                    my = next_node; len = 0; mn = x; mnoff = 0;
#pragma unroll
                    for (int q = 0; q < 16; q++) sb[q] = 0;
                }
            } else if (x < mn) { mn = x; mnoff = len; }
        }
    }
    if (MOM) {
        __syncthreads();                  // every wave leaves the loop (the pool runs dry for all of them)
        for (u32 b = threadIdx.x; b < WMOM_BUCKETS; b += 256) {
            const u32 c = mcnt[b];
            if (c) { atomicAdd(&mom[b], (unsigned long long)c); atomicAdd(&mom[WMOM_BUCKETS + b], msum[b]); atomicAdd(&mom[2 * WMOM_BUCKETS + b], msq[b]); }
        }
    }
}
// moments_solve_kernel / moments_budget_kernel / moments_chase_kernel of the main path (inverse.hip) with 64-bit elements and WMOM_BUCKETS ranges
__global__ __launch_bounds__(1024) void WI_KERNEL(moments_solve)(const unsigned long long *__restrict__ mom, u64 n, int shift, const WI_LFW *__restrict__ LF,
                                                                  u64 *__restrict__ uidx, u64 *__restrict__ ulf, u64 ucap, u32 *__restrict__ def_list,
                                                                  unsigned long long *__restrict__ counters)
{
    const u64 b = (u64)blockIdx.x * 1024 + threadIdx.x;
    if (b >= WMOM_BUCKETS || b >= n) return;
    const u64 size = (n - b + WMOM_BUCKETS - 1) >> WMOM_LOG2;
    const u64 cnt = mom[b];
    if (cnt > size) { atomicAdd(&counters[11], 1ull); return; }
    const u64 d = size - cnt;
    if (d == 0) return;
    const u64 sall = size * (size - 1) / 2;
    u64 f[3] = {size - 1, size, 2 * size - 1};
    { int two = 0, three = 0; for (int i = 0; i < 3; i++) { if (!two && f[i] % 2 == 0) { f[i] /= 2; two = 1; } } for (int i = 0; i < 3; i++) { if (!three && f[i] % 3 == 0) { f[i] /= 3; three = 1; } } }
    const u64 qall = f[0] * f[1] * f[2];                                     // mod 2^64, like the sums of squares it is compared with
    const u64 A = sall - mom[WMOM_BUCKETS + b], B = qall - mom[2 * WMOM_BUCKETS + b];
    if (d == 1) {
        if (A >= size || A * A != B) { atomicAdd(&counters[11], 1ull); return; }
        const unsigned long long at = atomicAdd(&counters[1], 1ull);
        if (at < ucap) { const u64 x = (A << WMOM_LOG2) | b; uidx[at] = x; ulf[at] = lf_at(LF, x); }
    } else if (d == 2) {
        const u64 D = 2 * B - A * A;
        u64 r = (u64)sqrt((double)D);
        while (r * r > D) r--;
        while ((r + 1) * (r + 1) <= D) r++;
        const u64 o1 = (A - r) / 2, o2 = (A + r) / 2;
        if (A >= 2 * size || r * r != D || r == 0 || ((A - r) & 1) || o2 >= size || o1 * o1 + o2 * o2 != B) { atomicAdd(&counters[11], 1ull); return; }
        const unsigned long long at = atomicAdd(&counters[1], 2ull);
        if (at < ucap) { const u64 x = (o1 << WMOM_LOG2) | b; uidx[at] = x; ulf[at] = lf_at(LF, x); }
        if (at + 1 < ucap) { const u64 x = (o2 << WMOM_LOG2) | b; uidx[at + 1] = x; ulf[at + 1] = lf_at(LF, x); }
    } else {
        const unsigned long long at = atomicAdd(&counters[10], 1ull);
        def_list[at] = (u32)b;
    }
}
__global__ __launch_bounds__(256) void WI_KERNEL(moments_chase)(const u32 *__restrict__ def_list, const unsigned long long *__restrict__ counters_in, u64 n, int shift,
                                                                 const WI_LFW *__restrict__ LF, u32 cap, u64 *__restrict__ uidx, u64 *__restrict__ ulf, u64 ucap,
                                                                 unsigned long long *__restrict__ counters)
{
    const u64 classes = counters_in[10];
    const u64 members = (n + WMOM_BUCKETS - 1) >> WMOM_LOG2;
    const u64 per = (members + 255) / 256;
    const u64 gmask = (1ull << WI_GL) - 1ull;
    (void)shift;
    for (u64 w = blockIdx.x; w < classes * per; w += gridDim.x) {
        const u64 x0 = (((w % per) * 256 + threadIdx.x) << WMOM_LOG2) | (u64)def_list[w / per];
        bool un = false;
        if (x0 < n) {
            if ((x0 & gmask) != 0) {
                u64 y = lf_at(LF, x0);
                u32 steps = 0;
                for (;;) {
                    if (y == x0) { un = true; break; }
                    if ((y & gmask) == 0) break;
                    if (++steps > cap) { atomicAdd(&counters[11], 1ull); break; }
                    y = lf_at(LF, y);
                }
            }
        }
        const u64 m = __ballot(un);
        if (m) {
            const int leader = __ffsll((unsigned long long)m) - 1;
            unsigned long long bse = 0;
            if (lane_id() == leader) bse = atomicAdd(&counters[1], (unsigned long long)__popcll(m));
            bse = shfl_t((u64)bse, leader);
            if (un) { const u64 at = bse + (u64)__popcll(m & lanemask_lt()); if (at < ucap) { uidx[at] = x0; ulf[at] = lf_at(LF, x0); } }
        }
    }
}
__global__ __launch_bounds__(256) void WI_KERNEL(collect_unvisited)(const WI_LFW *__restrict__ LF, const WI_MARKW *__restrict__ marks, u64 n,
                                                                     u64 *__restrict__ uidx, u64 *__restrict__ ulf, u64 cap, unsigned long long *__restrict__ count)
{
    for (u64 base = (u64)blockIdx.x * 256; base < n; base += (u64)gridDim.x * 256) {
        const u64 i = base + threadIdx.x;
        const bool un = i < n && WI_UNMARKED(marks, i);
        const u64 m = __ballot(un);
        if (m) {
            const int leader = __ffsll((unsigned long long)m) - 1;
            unsigned long long b = 0;
            if (lane_id() == leader) b = atomicAdd(count, (unsigned long long)__popcll(m));
            b = shfl_t((u64)b, leader);
            if (un) { const u64 at = b + (u64)__popcll(m & lanemask_lt()); if (at < cap) { uidx[at] = i; ulf[at] = lf_at(LF, i); } }
        }
    }
}
__global__ __launch_bounds__(256) void WI_KERNEL(tiny_place)(const WiCycle *__restrict__ cyc, u64 m, const u64 *__restrict__ end_of_cyc,
                                                              const WI_LFW *__restrict__ LF, const u64 *__restrict__ Cg, u8 *__restrict__ out)
{
    __shared__ u64 Ctab[257];
    for (int i = threadIdx.x; i < 257; i += 256) Ctab[i] = Cg[i];
    __syncthreads();
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const WiCycle c = cyc[i];
    if (c.leader != WI_NIL) return;
    u64 x = c.minelem, pos = end_of_cyc[i];
    for (u64 t = 0; t < c.len; t++) {
        const u64 y = lf_at(LF, x);
        out[pos--] = (u8)symbol_of64(Ctab, y);
        x = y;
    }
}
