// wide_inverse.h -- inverse transform of inputs beyond the 32-bit index range (n > 2^32).  Included by inverse.hip.
//
// Same plan as the main path (unbwts.c:31-86 -> stable LF map, splitter walk that records every segment's symbols, ranking
// of the reduced list, placement), with 64-bit element indices and without the main path's tuning: LF is a u64 array built
// segment by segment (the tile table's offsets are 32-bit), the unreached elements come from per-range moments (a byte map as the fallback), the reduced list
// (n / 256 nodes) is ranked by plain pointer jumping, and everything sized by node or cycle counts carries 64-bit positions.
// Memory at n = 12 GiB: LF 96 GiB + recorded segments 58 + nodes ~6 (+ marks 12 on the fallback).
//
// Compact form (taken when the full form's memory cannot be reserved, or forced by BWTS_WIDE_INV=compact): LF as packed 40-bit
// entries (5 n), segment records of one splitter spacing (slot = G) in a node pool sized by its hard bound, and splitters every
// 2^WC_G_LOG2 elements so that the node tables stay near 0.3 n, and marks as bits over the ranking tables on the fallback: about
// 7.35 n in all.
#define WI_G_LOG2 8
#define WC_G_LOG2 10
#define WI_NIL 0xffffffffu

__device__ __forceinline__ u32 symbol_of64(const u64 *Ctab, u64 y)
{
    u32 lo = 0, hi = 255;
#pragma unroll
    for (int it = 0; it < 8; it++) {
        const u32 mid = (lo + hi + 1) >> 1;
        if (Ctab[mid] <= y) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Every reader of LF in the wide form goes through lf_at(): the full form's u64 array, or the compact form's packed 40-bit entries.
// Entry x of the packed map is the 5 bytes at byte 5x (little endian), read with the two aligned dwords that hold them: one line
// fill per step as with the u64 array, except for the 1 in 32 entries that cross a 128-byte line.
// The kernels shared by both forms take the map as `const W *` and tell the two apart by the word type: u64 for the full form, u32
// (the dwords of the packed map) for the compact one.
__device__ __forceinline__ u64 lf_at(const u64 *LF, u64 x) { return LF[x]; }
__device__ __forceinline__ u64 lf_at(const u32 *LF40, u64 x)
{
    const u64 b = 5 * x;
    const u32 *p = LF40 + (b >> 2);
    const u32 k = (u32)b & 3u, lo = p[0], hi = p[1];
    return ((u64)((hi >> (8 * k)) & 0xffu) << 32) | __builtin_amdgcn_alignbyte(hi, lo, k);
}
// bytes of the packed map: 5 n, a dword of slack for the reader of the last entry, whole 16-byte stores of the builder's last wave
static inline size_t lf40_bytes(u64 n) { return align_up(5 * n + 16, 256); }

// LF[p0 + i] for one segment: the segment's scanned tile table gives the rank inside the segment (32-bit), base64[c] turns it
// into the global one: C[c] + occurrences of c in earlier segments - first slot of c in the segment's own table
// (emit(j, i, entry) receives item j of the lane: element i of the segment, valid where i < count)
template <typename Emit>
__device__ __forceinline__ void lf_rank_wide_body(const u8 *__restrict__ B, u64 count, const u32 *__restrict__ tile_off,
                                                  const u64 *__restrict__ base64, Emit emit)
{
    __shared__ u32 whist[LF_WAVES][256];
    __shared__ u64 sbase[256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const u64 wave_base = (u64)blockIdx.x * LF_TILE + (u64)w * (64 * LF_ITEMS);
    for (int i = tid; i < LF_WAVES * 256; i += LF_THREADS) ((u32 *)whist)[i] = 0;
    sbase[tid] = base64[tid];
    u32 sym[LF_ITEMS], rnk[LF_ITEMS];
#pragma unroll
    for (int j = 0; j < LF_ITEMS; j++) {
        const u64 i = wave_base + (u64)j * 64 + lane;
        sym[j] = i < count ? (u32)B[i] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LF_ITEMS; j++) {
        const bool valid = wave_base + (u64)j * 64 + lane < count;
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
    for (int j = 0; j < LF_ITEMS; j++) emit(j, wave_base + (u64)j * 64 + lane, sbase[sym[j]] + (u64)(whist[w][sym[j]] + rnk[j]));
}
__global__ __launch_bounds__(LF_THREADS) void lf_rank_wide_kernel(const u8 *__restrict__ B, u64 count, const u32 *__restrict__ tile_off,
                                                                  const u64 *__restrict__ base64, u64 *__restrict__ LF)
{
    lf_rank_wide_body(B, count, tile_off, base64, [&](int, u64 i, u64 e) { if (i < count) LF[i] = e; });
}
// the same into the packed map (LF points at the segment's first entry, 16-byte aligned: segments and waves start at multiples of
// 4096 and 1024 elements): a wave stages its 1024 entries in LDS and stores them as whole 16-byte words, never 5-byte pieces, so
// no two lanes write parts of one dword.  Past the segment's end only the slack behind the last entry is written.
__global__ __launch_bounds__(LF_THREADS) void lf_rank_c40_kernel(const u8 *__restrict__ B, u64 count, const u32 *__restrict__ tile_off,
                                                                 const u64 *__restrict__ base64, u8 *__restrict__ LF)
{
    constexpr u32 wave_bytes = 5 * 64 * LF_ITEMS;
    __shared__ __attribute__((aligned(16))) u8 stage[LF_WAVES][wave_bytes];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    lf_rank_wide_body(B, count, tile_off, base64, [&](int j, u64 i, u64 e) {
        if (i >= count) e = 0;
        u8 *d = &stage[w][5 * (j * 64 + lane)];
#pragma unroll
        for (int q = 0; q < 5; q++) d[q] = (u8)(e >> (8 * q));
    });
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const u64 wave_base = (u64)blockIdx.x * LF_TILE + (u64)w * (64 * LF_ITEMS);
    if (wave_base >= count) return;
    const u64 valid = 5 * (count - wave_base);
    uint4 *dst = (uint4 *)(LF + 5 * wave_base);
    const uint4 *src = (const uint4 *)stage[w];
    for (u32 q = lane; q < wave_bytes / 16; q += 64)
        if ((u64)q * 16 < valid) dst[q] = src[q];
}

// node record: where the walk went next, how many symbols it recorded, the smallest element it saw and where
struct WiNode { u32 nxt, len; u64 mn; u32 off, pad; };

// MOM (walk_record_*_kernel in wide_lf_kernels.inc): the unreached elements come from per-range moments over WMOM_BUCKETS ranges
#define WMOM_LOG2 12
#define WMOM_BUCKETS (1u << WMOM_LOG2)

// pointer jumping over the nodes: records (leader, hop, smallest element) and (sum of lengths, hop)
struct WiMin { u32 leader, hop; u64 mn; };
struct WiSum { u64 sum; u32 hop, pad; };
struct WiCycle { u64 minelem, len; u32 leader, pad; };

__global__ __launch_bounds__(256) void wi_init_kernel(u64 s, const WiNode *__restrict__ nodes, WiMin *__restrict__ rec)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v < s) { WiMin r; r.leader = (u32)v; r.hop = nodes[v].nxt; r.mn = nodes[v].mn; rec[v] = r; }
}
__global__ __launch_bounds__(256) void wi_jump_min_kernel(u64 s, const WiMin *__restrict__ in, WiMin *__restrict__ out)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v >= s) return;
    const WiMin a = in[v], b = in[a.hop];
    WiMin r; r.leader = a.leader < b.leader ? a.leader : b.leader; r.mn = a.mn < b.mn ? a.mn : b.mn; r.hop = b.hop;
    out[v] = r;
}
__global__ __launch_bounds__(256) void wi_cut_kernel(u64 s, const WiNode *__restrict__ nodes, const WiMin *__restrict__ rec, WiSum *__restrict__ sh)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v < s) { WiSum r; r.sum = nodes[v].len; r.hop = nodes[v].nxt == rec[v].leader ? WI_NIL : nodes[v].nxt; r.pad = 0; sh[v] = r; }
}
__global__ __launch_bounds__(256) void wi_jump_sum_kernel(u64 s, const WiSum *__restrict__ in, WiSum *__restrict__ out)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v >= s) return;
    const WiSum a = in[v];
    if (a.hop == WI_NIL) out[v] = a;
    else { const WiSum b = in[a.hop]; WiSum r; r.sum = a.sum + b.sum; r.hop = b.hop; r.pad = 0; out[v] = r; }
}
__global__ __launch_bounds__(256) void wi_finish_kernel(u64 s, const WiMin *__restrict__ rec, const WiSum *__restrict__ sh, const WiNode *__restrict__ nodes,
                                                        u64 *__restrict__ dist, u64 *__restrict__ min_dist, WiCycle *__restrict__ cyc,
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
        WiCycle c; c.minelem = r.mn; c.len = L; c.leader = r.leader; c.pad = 0;
        cyc[at] = c;
    }
}
// cycles without a splitter (tiny_cycle_scan_kernel of the main path)
template <typename W>
__device__ __forceinline__ void tiny_cycle_scan_wide_body(const u64 *__restrict__ uidx, const u64 *__restrict__ ulf, u64 nu, const W *__restrict__ LF, u32 cap,
                                                          WiCycle *__restrict__ cyc, unsigned long long *__restrict__ count,
                                                          unsigned long long *__restrict__ overflow)
{
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    bool ismin = false;
    u64 x = 0, len = 1;
    if (q < nu) {
        x = uidx[q];
        u64 y = ulf[q];
        ismin = true;
        while (y != x) {
            if (y < x) { ismin = false; break; }
            y = lf_at(LF, y);
            if (++len > cap) { atomicAdd(overflow, 1ull); ismin = false; break; }
        }
    }
    const u64 m = __ballot(ismin);
    if (m == 0) return;
    const int leader = __ffsll((unsigned long long)m) - 1;
    unsigned long long b = 0;
    if (lane_id() == leader) b = atomicAdd(count, (unsigned long long)__popcll(m));
    b = shfl_t((u64)b, leader);
    if (ismin) { WiCycle c; c.minelem = x; c.len = len; c.leader = WI_NIL; c.pad = 0; cyc[b + (u64)__popcll(m & lanemask_lt())] = c; }
}
__global__ __launch_bounds__(256) void tiny_cycle_scan_wide_kernel(const u64 *__restrict__ uidx, const u64 *__restrict__ ulf, u64 nu, const u64 *__restrict__ LF,
                                                                   u32 cap, WiCycle *__restrict__ cyc, unsigned long long *__restrict__ count,
                                                                   unsigned long long *__restrict__ overflow)
{
    tiny_cycle_scan_wide_body(uidx, ulf, nu, LF, cap, cyc, count, overflow);
}
__global__ __launch_bounds__(256) void tiny_cycle_scan_c40_kernel(const u64 *__restrict__ uidx, const u64 *__restrict__ ulf, u64 nu, const u32 *__restrict__ LF,
                                                                  u32 cap, WiCycle *__restrict__ cyc, unsigned long long *__restrict__ count,
                                                                  unsigned long long *__restrict__ overflow)
{
    tiny_cycle_scan_wide_body(uidx, ulf, nu, LF, cap, cyc, count, overflow);
}
__global__ __launch_bounds__(256) void wi_cycle_keys_kernel(const WiCycle *__restrict__ cyc, u64 m, u64 *__restrict__ keys, u32 *__restrict__ vals)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < m) { keys[i] = cyc[i].minelem; vals[i] = (u32)i; }
}
struct WiLenIn {
    const WiCycle *cyc; const u32 *order;
    __device__ __forceinline__ u64 operator()(u64 j) const { return cyc[order[j]].len; }
};
struct WiEndOut {
    const WiCycle *cyc; const u32 *order; u64 m; u64 last; u64 *end_by_leader; u64 *end_of_cyc; u64 *total;
    u64 *end_by_unit_leader;      // cycles ranked as unit nodes (leader tagged WI_UNIT_TAG), or null
    __device__ __forceinline__ void operator()(u64 j, u64 used) const
    {
        const u32 i = order[j];
        const WiCycle c = cyc[i];
        const u64 end = last - used;
        if (c.leader != WI_NIL) {
            if (c.leader & 0x80000000u) end_by_unit_leader[c.leader & 0x7fffffffu] = end;
            else end_by_leader[c.leader] = end;
        }
        end_of_cyc[i] = end;
        if (j + 1 == m) *total = used + c.len;
    }
};
// node -> text position of its first symbol, symbols until the walk passes the cycle's smallest element, cycle length
__global__ __launch_bounds__(256) void wi_place_kernel(u64 s, const WiMin *__restrict__ rec, const WiSum *__restrict__ sh, const u64 *__restrict__ dist,
                                                       const u64 *__restrict__ min_dist, const u64 *__restrict__ end_by_leader,
                                                       u64 *__restrict__ opos, u64 *__restrict__ wrap_at, u64 *__restrict__ cyc_len)
{
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v >= s) return;
    const u32 l = rec[v].leader;
    const u64 L = sh[l].sum, dm = min_dist[l], d = dist[v];
    const u64 t = d >= dm ? d - dm : d + L - dm;
    opos[v] = end_by_leader[l] - t;
    wrap_at[v] = L - t;
    cyc_len[v] = L;
}
__global__ __launch_bounds__(256) void place_segments_wide_kernel(const u8 *__restrict__ seg, u64 nodes_n, u32 slot, int tpn_log2, const WiNode *__restrict__ nodes,
                                                                  const u64 *__restrict__ opos, const u64 *__restrict__ wrap_at, const u64 *__restrict__ cyc_len,
                                                                  u8 *__restrict__ out)
{
    const u64 gid = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 v = gid >> tpn_log2;
    if (v >= nodes_n) return;
    const u32 sub = (u32)(gid & ((1ull << tpn_log2) - 1ull)), tpn = 1u << tpn_log2;
    const u32 len = nodes[v].len;
    const u64 o = opos[v], wr = wrap_at[v], L = cyc_len[v];
    const u8 *src = seg + v * slot;
    for (u32 c = sub * 16; c < len; c += tpn * 16) {
        if (c + 16 <= len && ((u64)c + 16 <= wr || (u64)c >= wr)) {
            const uint4 q = *(const uint4 *)(src + c);
            const u64 base = (u64)c >= wr ? o - c + L : o - c;
            Unaligned16 r;
            r.w[0] = __builtin_bswap32(q.w); r.w[1] = __builtin_bswap32(q.z);
            r.w[2] = __builtin_bswap32(q.y); r.w[3] = __builtin_bswap32(q.x);
            *(Unaligned16 *)(out + base - 15) = r;
        } else {
            const u32 e = c + 16 < len ? c + 16 : len;
            for (u32 i = c; i < e; i++) out[(u64)i >= wr ? o - i + L : o - i] = src[i];
        }
    }
}
// The kernels that read LF, once per form from one source (wide_lf_kernels.inc): the walk, the searches for unreached elements and
// the placement of cycles without a splitter.  The full form: u64 LF, splitters every 2^WI_G_LOG2 elements, a byte per mark.
#define WI_KERNEL(name) name##_wide_kernel
#define WI_LFW u64
#define WI_GL WI_G_LOG2
#define WI_MARKW u8
#define WI_MARK(m, x) m[x] = 1
#define WI_UNMARKED(m, i) m[i] == 0
#include "wide_lf_kernels.inc"
#undef WI_KERNEL
#undef WI_LFW
#undef WI_GL
#undef WI_MARKW
#undef WI_MARK
#undef WI_UNMARKED
// The compact form: packed 40-bit LF (dwords, see lf_at), splitters every 2^WC_G_LOG2 elements, a bit per mark (n / 8 bytes)
#define WI_KERNEL(name) name##_c40_kernel
#define WI_LFW u32
#define WI_GL WC_G_LOG2
#define WI_MARKW u32
#define WI_MARK(m, x) atomicOr(&m[x >> 5], 1u << ((u32)x & 31u))
#define WI_UNMARKED(m, i) ((m[i >> 5] >> ((u32)i & 31u)) & 1u) == 0
#include "wide_lf_kernels.inc"
#undef WI_KERNEL
#undef WI_LFW
#undef WI_GL
#undef WI_MARKW
#undef WI_MARK
#undef WI_UNMARKED

// ---- cycles without a splitter that are too long for one lane --------------------------------------------------------------
// (structured inputs: no regular splitter i * 2^WI_G_LOG2 on a cycle of tens of thousands of elements).  Every unreached
// element becomes a node of its own -- length 1, successor = the compact index of LF[x] -- and the node kernels above rank that
// list in parallel (O(nu log nu) work, about 110 bytes per unreached element, taken from the device for the call).
#define WI_UNIT_TAG 0x80000000u      // leader indices of these cycles are kept apart from the splitter nodes'
template <typename IDX>      // u64 here, u32 on the main path (inverse.hip)
__global__ __launch_bounds__(256) void wi_unit_index_kernel(const IDX *__restrict__ uidx, u64 nu, IDX *__restrict__ LF)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < nu) LF[uidx[i]] = (IDX)i;                // the entry's old value lives on in ulf[i]
}
template <typename IDX>
__global__ __launch_bounds__(256) void wi_unit_nodes_kernel(const IDX *__restrict__ uidx, const IDX *__restrict__ ulf, u64 nu, const IDX *__restrict__ LF,
                                                            WiNode *__restrict__ nodes)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < nu) { WiNode nd; nd.nxt = (u32)LF[ulf[i]]; nd.len = 1; nd.mn = uidx[i]; nd.off = 0; nd.pad = 0; nodes[i] = nd; }
}
// the same over the packed map.  Neighbouring entries share dwords, so an entry's 5 bytes are replaced by an atomic and + or on
// each of the two dwords that hold them (bytes k..3 of the first, 0..k of the second, k = 5x mod 4): other lanes' bytes stay as they are.
__global__ __launch_bounds__(256) void wi_unit_index_c40_kernel(const u64 *__restrict__ uidx, u64 nu, u32 *__restrict__ LF)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= nu) return;
    const u64 b = 5 * uidx[i];
    u32 *p = LF + (b >> 2);
    const u32 k = (u32)b & 3u, lo = (u32)i, hi = (u32)(i >> 32);
    const u32 m0 = 0xffffffffu << (8 * k), v0 = lo << (8 * k);
    const u32 m1 = k == 3 ? 0xffffffffu : (1u << (8 * k + 8)) - 1u, v1 = (k == 0 ? hi : __builtin_amdgcn_alignbyte(hi, lo, 4 - k)) & m1;
    atomicAnd(&p[0], ~m0); atomicOr(&p[0], v0);
    atomicAnd(&p[1], ~m1); atomicOr(&p[1], v1);
}
__global__ __launch_bounds__(256) void wi_unit_nodes_c40_kernel(const u64 *__restrict__ uidx, const u64 *__restrict__ ulf, u64 nu, const u32 *__restrict__ LF,
                                                                WiNode *__restrict__ nodes)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < nu) { WiNode nd; nd.nxt = (u32)lf_at(LF, ulf[i]); nd.len = 1; nd.mn = uidx[i]; nd.off = 0; nd.pad = 0; nodes[i] = nd; }
}
__global__ __launch_bounds__(256) void wi_unit_tag_kernel(WiCycle *__restrict__ cyc, u64 m)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < m) cyc[i].leader |= WI_UNIT_TAG;
}
// wi_place_kernel + place_segments_wide_kernel for nodes of one symbol
// FROM_INPUT (the narrow form's shared pass over segments, inverse.hip): the unit node's symbol is B[uidx[v]], not looked up from its LF value
template <typename IDX, bool FROM_INPUT>
__device__ __forceinline__ void wi_unit_place_body(u64 nu, const WiMin *rec, const WiSum *sh, const u64 *dist,
                                                   const u64 *min_dist, const IDX *end_by_leader,
                                                   const IDX *ulf, const u64 *Cg, const IDX *uidx, const u8 *Bsym,
                                                   u8 *out)
{
    __shared__ u64 Ctab[FROM_INPUT ? 1 : 257];
    if (!FROM_INPUT) for (int i = threadIdx.x; i < 257; i += 256) Ctab[i] = Cg[i];
    __syncthreads();
    const u64 v = (u64)blockIdx.x * 256 + threadIdx.x;
    if (v >= nu) return;
    const u32 l = rec[v].leader;
    const u64 L = sh[l].sum, dm = min_dist[l], d = dist[v];
    const u64 t = d >= dm ? d - dm : d + L - dm;
    out[(u64)end_by_leader[l] - t] = FROM_INPUT ? Bsym[uidx[v]] : (u8)symbol_of64(Ctab, (u64)ulf[v]);
}
template <typename IDX>
__global__ __launch_bounds__(256) void wi_unit_place_kernel(u64 nu, const WiMin *__restrict__ rec, const WiSum *__restrict__ sh, const u64 *__restrict__ dist,
                                                            const u64 *__restrict__ min_dist, const IDX *__restrict__ end_by_leader,
                                                            const IDX *__restrict__ ulf, const u64 *__restrict__ Cg, u8 *__restrict__ out)
{
    wi_unit_place_body<IDX, false>(nu, rec, sh, dist, min_dist, end_by_leader, ulf, Cg, nullptr, nullptr, out);
}
template <typename IDX>
__global__ __launch_bounds__(256) void wi_unit_place_seg_kernel(u64 nu, const WiMin *__restrict__ rec, const WiSum *__restrict__ sh, const u64 *__restrict__ dist,
                                                                const u64 *__restrict__ min_dist, const IDX *__restrict__ end_by_leader,
                                                                const IDX *__restrict__ uidx, const u8 *__restrict__ B, u8 *__restrict__ out)
{
    wi_unit_place_body<IDX, true>(nu, rec, sh, dist, min_dist, end_by_leader, nullptr, nullptr, uidx, B, out);
}
// device memory for one call (the rare paths): released when the call returns
struct ScopedDeviceBlock {
    bwts_ctx *ctx; char *p = nullptr;
    explicit ScopedDeviceBlock(bwts_ctx *c) : ctx(c) {}
    int take(size_t bytes)
    {
        if (hipMalloc((void **)&p, bytes) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return BWTS_E_NOMEM; }
        if (bytes > ctx->call_block_bytes) ctx->call_block_bytes = bytes;
        return BWTS_OK;
    }
    ~ScopedDeviceBlock() { if (p) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(p); } }
};
// The pointer jumping over a node list (the wide node list, and the unit nodes of both forms): its two ping-pong pairs, declared
// into the caller's layout, and which side of each holds the result
struct WiRanking {
    WiMin *mn[2] = {nullptr, nullptr}; WiSum *sum[2] = {nullptr, nullptr}; int cur = 0, sc = 0;
    void declare(BlockLayout &L, u64 count) { L.arrays(count, &mn[0], &mn[1], &sum[0], &sum[1]); }
    const WiMin *min_of() const { return mn[cur]; } const WiSum *sum_of() const { return sum[sc]; }
};
// wi_init -> R x wi_jump_min -> wi_cut -> R x wi_jump_sum, 2^R > count >= any cycle's node count.  The finish kernel is the caller's.
static void wi_rank_nodes(bwts_ctx *ctx, u64 count, const WiNode *nodes, WiRanking &k)
{
    const int gb = grid1(count), R = bit_length(count);
    wi_init_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(count, nodes, k.mn[0]);
    for (int r = 0; r < R; r++, k.cur ^= 1) wi_jump_min_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(count, k.mn[k.cur], k.mn[k.cur ^ 1]);
    wi_cut_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(count, nodes, k.mn[k.cur], k.sum[0]);
    for (int r = 0; r < R; r++, k.sc ^= 1) wi_jump_sum_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(count, k.sum[k.sc], k.sum[k.sc ^ 1]);
}
// Side block 0 of an attempt (InvRun, WideRun): room for `cap` unreached elements (uidx, ulf), and for the records and ends of cap +
// `more` cycles -- the cycles without a splitter (at most cap), in the wide form next to those of the node list
template <typename RUN, typename CYC, typename END> static int lay_out_unreached(bwts_ctx *ctx, RUN &r, u64 cap, u64 more, CYC **cyc, END **ends)
{
    char *ub = nullptr; BlockLayout L;
    L.arrays(cap, &r.uidx, &r.ulf); L.array(cyc, cap + more); L.array(ends, cap + more);
    BWTS_TRY(aux_reserve_slot(ctx, 0, L.bytes(), &ub));
    L.place(ub);
    r.ucap = cap;
    return BWTS_OK;
}
// one lane of the scan for cycles without a splitter follows at most so many elements: bounds the work of an adversarial LF (many long cycles that dodge every splitter)
static u32 one_lane_cap(u64 nu, u64 G) { const u64 cap = (1ull << 36) / nu; return (u32)(cap > 64 * G ? 64 * G : cap < 4 * G ? 4 * G : cap); }
// The unit-node route's tables, in a block taken from the device for the call (about 110 bytes per unreached element): the caller
// declares its own ends (and leaders) behind them -- u64 here, u32 on the main path
struct UnitRank {
    WiNode *nodes = nullptr; WiRanking rk; u64 *dist = nullptr, *min_dist = nullptr;
    void declare(BlockLayout &L, u64 nu) { L.array(&nodes, nu); rk.declare(L, nu); L.arrays(nu, &dist, &min_dist); }
};
// One attempt of the 64-bit form: its sizes, its arrays in the arena, and what one stage hands to the next
struct WideRun {
    u64 n, G, s, node_cap, segn, nseg; u32 slot; bool moments, compact;
    size_t lf_bytes, mark_bytes, overlay_bytes = 0;
    u64 *LF = nullptr; u32 *LF40 = nullptr;             // the map: full form, compact form
    u8 *marks = nullptr, *seg = nullptr; unsigned long long *mom = nullptr; u32 *def_list = nullptr, *tile_hist = nullptr; void *scan_temp = nullptr;
    WiNode *nodes = nullptr; WiRanking rk; WiCycle *ncyc = nullptr;
    u64 *dist = nullptr, *min_dist = nullptr, *end_by_leader = nullptr, *opos = nullptr, *wrap_at = nullptr, *cyc_len = nullptr, *dC = nullptr;
    u64 ucap = 0, *uidx = nullptr, *ulf = nullptr, *end_of_cyc = nullptr; WiCycle *cyc = nullptr;      // side block 0: the unreached elements; all cycles and their ends
    u64 s_all = 0, nu = 0, kc = 0, kt = 0; bool unit_rank = false;     // ... the unit-node route: its block, taken from the device for the call
    UnitRank unit; u64 *uend = nullptr; ScopedDeviceBlock ub;
    u64 rep_spill[INV_REPORT_WORDS], *rep;              // this attempt's record (the fields the wide form has)
    WideRun(bwts_ctx *ctx, u64 n_, bool moments_, bool compact_) : n(n_), moments(moments_), compact(compact_), ub(ctx)
    {
        G = 1ull << (compact ? WC_G_LOG2 : WI_G_LOG2); s = (n + G - 1) / G;
        // compact: one splitter spacing per record (BWTS_WIDE_SLOT, a multiple of 64, for tests), and the pool's hard bound -- every
        // overflow node follows a node that recorded a full slot, and the walk records each element at most once
        slot = (u32)(compact ? G : 4 * G);
        if (const char *e = compact ? bwts_knob(ctx, "BWTS_WIDE_SLOT") : nullptr) { const long v = atol(e); if (v >= 64 && v <= (1 << 20) && v % 64 == 0) slot = (u32)v; }
        node_cap = compact ? s + (n + slot - 1) / slot + 1024 : s + s / 8 + 1024;
        int seg_log2 = 31;
        if (const char *e = bwts_knob(ctx, "BWTS_WIDE_SEG_LOG2")) { const int v = atoi(e); if (v >= 12 && v <= 31) seg_log2 = v; }
        segn = 1ull << seg_log2; nseg = (n + segn - 1) / segn;
        lf_bytes = compact ? lf40_bytes(n) : BlockLayout::padded<u64>(n);
        // marks: bytes in the full form; bits in the compact one, laid over the ranking tables -- the walk sets them and every collection
        // (a second one where the first ran out of room) reads them before the ranking writes those tables: the fallback needs no more
        // memory than the moments
        mark_bytes = compact ? (n + 31) / 32 * 4 : n;
        rep = inv_report_open(ctx, rep_spill);
        rep[IR_G] = compact ? WC_G_LOG2 : WI_G_LOG2; rep[IR_MARK] = moments ? MARK_MOMENTS : MARK_BYTEMAP; rep[IR_S] = s; rep[IR_NODE_CAP] = node_cap; rep[IR_FORM] = compact ? IR_FORM_WIDE_COMPACT : IR_FORM_WIDE;
    }
    void declare(BlockLayout &L)
    {
        if (compact) L.raw(&LF40, lf_bytes); else L.raw(&LF, lf_bytes);
        L.raw(&marks, moments || compact ? 256 : align_up(mark_bytes, 256));      // no byte map kept: a token block (the kernels take a pointer)
        L.array(&mom, 3 * WMOM_BUCKETS); L.array(&def_list, WMOM_BUCKETS); L.array(&seg, node_cap * slot); L.array(&nodes, node_cap);
        const size_t ranking_from = L.bytes(); rk.declare(L, node_cap);
        L.arrays(node_cap, &dist, &min_dist, &end_by_leader, &opos, &wrap_at, &cyc_len); L.array(&ncyc, node_cap);
        overlay_bytes = L.bytes() - ranking_from;       // rk.mn[0] .. the end of ncyc: where the compact form's mark bits go
        L.raw(&tile_hist, radix_tile_hist_bytes(segn)); L.raw(&scan_temp, scan_temp_bytes(segn)); L.pad(INV_ARENA_SLACK);
    }
};
static int wide_reserve(bwts_ctx *ctx, WideRun &r)
{
    BWTS_TRY(arena_place(ctx, r));
    if (r.compact && !r.moments) {
        if (r.overlay_bytes < r.mark_bytes) return BWTS_E_INTERNAL;
        r.marks = (u8 *)r.rk.mn[0];
    }
    return BWTS_OK;
}
// symbol boundaries C (unbwts.c:34-43), 64-bit, and the stable LF map (unbwts.c:50-52), segment by segment
static int wide_build_lf(bwts_ctx *ctx, WideRun &r, const u8 *d_in)
{
    const u64 n = r.n;
    u64 *hC = ctx->h_small + 1024, *dBase = ctx->d_small + 1536, *hBase = ctx->h_small + 1536, *dHist = ctx->d_small + 2048, *hHist = ctx->h_small + 2048;
    BWTS_TRY(byte_histogram_device(ctx, d_in, n, dHist));
    BWTS_TRY(read_small(ctx, 2048, 256));
    {
        u64 run = 0;
        for (int c = 0; c < 256; c++) { hC[c] = run; run += hHist[c]; }
        hC[256] = n;
        if (run != n) return BWTS_E_INTERNAL;
    }
    HIPC(hipMemcpyAsync(r.dC, hC, 257 * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    u64 before[256] = {0};
    for (u64 sg = 0; sg < r.nseg; sg++) {
        const u64 p0 = sg * r.segn, c = n - p0 < r.segn ? n - p0 : r.segn;
        const u64 tiles = (c + LF_TILE - 1) / LF_TILE;
        SpanGuard g(ctx, BWTS_K_LF_BUILD, c, 10 * c);
        BWTS_TRY(byte_histogram_device(ctx, d_in + p0, c, dHist));
        BWTS_TRY(read_small(ctx, 2048, 256));
        {
            u64 run = 0;
            for (int q = 0; q < 256; q++) { hBase[q] = hC[q] + before[q] - run; run += hHist[q]; before[q] += hHist[q]; }
        }
        HIPC(hipMemcpyAsync(dBase, hBase, 256 * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
        lf_hist_kernel<<<dim3((unsigned)tiles), dim3(LF_THREADS), 0, ctx->stream>>>(d_in + p0, c, r.tile_hist);
        BWTS_TRY(radix_column_scan(ctx, r.tile_hist, tiles, r.scan_temp));
        if (r.compact) lf_rank_c40_kernel<<<dim3((unsigned)tiles), dim3(LF_THREADS), 0, ctx->stream>>>(d_in + p0, c, r.tile_hist, dBase, (u8 *)r.LF40 + 5 * p0);
        else lf_rank_wide_kernel<<<dim3((unsigned)tiles), dim3(LF_THREADS), 0, ctx->stream>>>(d_in + p0, c, r.tile_hist, dBase, r.LF + p0);
        HIPC(hipGetLastError());
        HIPC(hipStreamSynchronize(ctx->stream));            // hBase is rewritten by the next segment
    }
    return BWTS_OK;
}
template <typename K, typename LFW, typename MARKW> static int launch_wide_walk(bwts_ctx *ctx, const WideRun &r, K kernel, const LFW *LF, MARKW *marks)
{
    const u64 walkers = r.s < 524288 ? r.s : 524288;
    const size_t lds = r.moments ? (size_t)WMOM_BUCKETS * (8 + 8 + 4) : 0;
    if (r.moments) BWTS_TRY(ensure_dyn_lds(ctx, (const void *)kernel, lds));
    kernel<<<dim3((unsigned)((walkers + 255) / 256)), dim3(256), lds, ctx->stream>>>(LF, marks, r.s, r.node_cap, r.slot, r.dC, r.seg, r.nodes, inv_counter(ctx, IC_TICKET),
                                                                                     inv_counter(ctx, IC_VIRTUAL), inv_counter(ctx, IC_OVERFLOW), r.moments ? WMOM_LOG2 : 0,
                                                                                     r.moments ? r.mom : nullptr);
    return launched(ctx);
}
static int wide_walk(bwts_ctx *ctx, WideRun &r)
{
    HIPC(hipMemsetAsync(inv_counter(ctx, 0), 0, IC_WORDS * sizeof(u64), ctx->stream));
    if (r.moments) HIPC(hipMemsetAsync(r.mom, 0, 3 * WMOM_BUCKETS * sizeof(u64), ctx->stream));
    else HIPC(hipMemsetAsync(r.marks, 0, r.mark_bytes, ctx->stream));
    {
        SpanGuard sg(ctx, BWTS_K_WALK, r.n, 10 * r.n);
        if (r.compact && r.moments) BWTS_TRY(launch_wide_walk(ctx, r, walk_record_c40_kernel<true>, r.LF40, (u32 *)r.marks));
        else if (r.compact) BWTS_TRY(launch_wide_walk(ctx, r, walk_record_c40_kernel<false>, r.LF40, (u32 *)r.marks));
        else if (r.moments) BWTS_TRY(launch_wide_walk(ctx, r, walk_record_wide_kernel<true>, r.LF, r.marks));
        else BWTS_TRY(launch_wide_walk(ctx, r, walk_record_wide_kernel<false>, r.LF, r.marks));
    }
    BWTS_TRY(read_small(ctx, SMI_COUNTERS, IC_WORDS));
    r.rep[IR_VIRTUAL] = inv_count(ctx, IC_VIRTUAL);
    if (inv_count(ctx, IC_OVERFLOW)) return r.compact ? BWTS_E_INTERNAL : BWTS_E_NOMEM;     // node pool exhausted (adversarial LF): the compact form's pool cannot be
    r.s_all = r.s + inv_count(ctx, IC_VIRTUAL);
    return BWTS_OK;
}
static int wide_collect(bwts_ctx *ctx, WideRun &r)
{
    SpanGuard sg(ctx, BWTS_K_OTHER, r.n, r.n);
    const u64 n = r.n; unsigned long long *ctr = inv_counter(ctx, 0);
    if (r.moments) {
        HIPC(hipMemsetAsync(inv_counter(ctx, IC_LISTED_CLASSES), 0, 2 * sizeof(u64), ctx->stream));      // ... and IC_MOM_FALLBACK
        const u64 per_class = (n + WMOM_BUCKETS - 1) >> WMOM_LOG2;
        const u64 budget = (8ull << 20) > per_class ? (8ull << 20) : per_class;        // elements the search may look at (at least one class)
        if (r.compact) moments_solve_c40_kernel<<<dim3(WMOM_BUCKETS / 1024), dim3(1024), 0, ctx->stream>>>(r.mom, n, WMOM_LOG2, r.LF40, r.uidx, r.ulf, r.ucap, r.def_list, ctr);
        else moments_solve_wide_kernel<<<dim3(WMOM_BUCKETS / 1024), dim3(1024), 0, ctx->stream>>>(r.mom, n, WMOM_LOG2, r.LF, r.uidx, r.ulf, r.ucap, r.def_list, ctr);
        moments_budget_kernel<<<dim3(1), dim3(64), 0, ctx->stream>>>(ctr, per_class, budget);
        if (r.compact) moments_chase_c40_kernel<<<dim3(4096), dim3(256), 0, ctx->stream>>>(r.def_list, ctr, n, WMOM_LOG2, r.LF40, 1u << 16, r.uidx, r.ulf, r.ucap, ctr);
        else moments_chase_wide_kernel<<<dim3(4096), dim3(256), 0, ctx->stream>>>(r.def_list, ctr, n, WMOM_LOG2, r.LF, 1u << 16, r.uidx, r.ulf, r.ucap, ctr);
    } else {
        u64 blocks = (n + 255) / 256; if (blocks > 16384) blocks = 16384;
        unsigned long long *found = inv_counter(ctx, IC_UNREACHED);
        if (r.compact) collect_unvisited_c40_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(r.LF40, (const u32 *)r.marks, n, r.uidx, r.ulf, r.ucap, found);
        else collect_unvisited_wide_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(r.LF, r.marks, n, r.uidx, r.ulf, r.ucap, found);
    }
    return launched(ctx);
}
// collect, count, and collect again where the first room was too small -- before the ranking writes its tables: the compact form's mark bits lie over them
static int wide_collect_unreached(bwts_ctx *ctx, WideRun &r, bool *need_marks)
{
    const u64 ucap = ctx->unv_hint > (1ull << 20) ? ctx->unv_hint : (1ull << 20);
    BWTS_TRY(lay_out_unreached(ctx, r, ucap > r.n ? r.n : ucap, r.node_cap, &r.cyc, &r.end_of_cyc));
    BWTS_TRY(wide_collect(ctx, r));
    BWTS_TRY(read_small(ctx, SMI_COUNTERS, IC_WORDS));
    r.rep[IR_UCAP_FIRST] = r.ucap; r.rep[IR_NU] = inv_count(ctx, IC_UNREACHED);
    r.rep[IR_LISTED] = inv_count(ctx, IC_LISTED_CLASSES); r.rep[IR_MOM_FALLBACK] = inv_count(ctx, IC_MOM_FALLBACK);
    if (r.moments && inv_count(ctx, IC_MOM_FALLBACK)) { *need_marks = true; return BWTS_OK; }     // too many unreached elements for the moments: the byte map
    r.nu = inv_count(ctx, IC_UNREACHED);
    if (r.nu > r.n) return BWTS_E_INTERNAL;
    if (r.nu > r.ucap) {
        BWTS_TRY(lay_out_unreached(ctx, r, r.nu, r.node_cap, &r.cyc, &r.end_of_cyc));
        HIPC(hipMemsetAsync(inv_counter(ctx, IC_UNREACHED), 0, sizeof(u64), ctx->stream));
        BWTS_TRY(wide_collect(ctx, r));
        BWTS_TRY(read_small(ctx, SMI_COUNTERS, IC_WORDS));
        if (inv_count(ctx, IC_UNREACHED) != r.nu) return BWTS_E_INTERNAL;
        r.rep[IR_SECOND_COLLECT] = 1;
    }
    return BWTS_OK;
}
// pointer jumping over the nodes; cycle records of the node list
static int wide_rank_node_list(bwts_ctx *ctx, WideRun &r)
{
    {
        SpanGuard sg(ctx, BWTS_K_LISTRANK, r.s_all, 0);
        wi_rank_nodes(ctx, r.s_all, r.nodes, r.rk);
        wi_finish_kernel<<<dim3(grid1(r.s_all)), dim3(256), 0, ctx->stream>>>(r.s_all, r.rk.min_of(), r.rk.sum_of(), r.nodes, r.dist, r.min_dist, r.ncyc,
                                                                             inv_counter(ctx, IC_LIST_CYCLES));
        HIPC(hipGetLastError());
    }
    BWTS_TRY(read_small(ctx, SMI_COUNTERS, IC_WORDS));
    r.kc = inv_count(ctx, IC_LIST_CYCLES);
    r.rep[IR_KC] = r.kc;
    ctx->tm.unvisited = r.nu; ctx->unv_hint = (size_t)r.nu;
    return r.kc == 0 || r.kc > r.s_all ? BWTS_E_INTERNAL : BWTS_OK;
}
// cycles without a splitter: the one-lane scan, or the unit-node ranking
static int wide_free_cycles(bwts_ctx *ctx, WideRun &r)
{
    if (r.nu) {
        SpanGuard sg(ctx, BWTS_K_OTHER, r.nu, 16 * r.nu);
        const u32 cap = one_lane_cap(r.nu, r.G);
        unsigned long long *count = inv_counter(ctx, IC_FREE_CYCLES), *overflow = inv_counter(ctx, IC_OVERFLOW);
        if (r.compact) tiny_cycle_scan_c40_kernel<<<dim3(grid1(r.nu)), dim3(256), 0, ctx->stream>>>(r.uidx, r.ulf, r.nu, r.LF40, cap, r.cyc, count, overflow);
        else tiny_cycle_scan_wide_kernel<<<dim3(grid1(r.nu)), dim3(256), 0, ctx->stream>>>(r.uidx, r.ulf, r.nu, r.LF, cap, r.cyc, count, overflow);
        HIPC(hipGetLastError());
    }
    BWTS_TRY(read_small(ctx, SMI_COUNTERS, IC_WORDS));
    r.kt = inv_count(ctx, IC_FREE_CYCLES);
    if (r.kt > r.nu) return BWTS_E_INTERNAL;
    r.unit_rank = inv_count(ctx, IC_OVERFLOW) != 0;
    r.rep[IR_UNIT_RANK] = r.unit_rank; r.rep[IR_KT] = r.kt;
    if (!r.unit_rank) return BWTS_OK;
    // a cycle without a splitter too long for one lane: all unreached elements are ranked as nodes of one symbol instead
    SpanGuard sg(ctx, BWTS_K_LISTRANK, r.nu, 0);
    if (r.nu >= 0x7ffffff0ull) return BWTS_E_NOMEM;
    BlockLayout L; r.unit.declare(L, r.nu); L.array(&r.uend, r.nu);
    BWTS_TRY(r.ub.take(L.bytes()));
    L.place(r.ub.p);
    const int gb = grid1(r.nu);
    HIPC(hipMemsetAsync(inv_counter(ctx, IC_UNIT_CYCLES), 0, sizeof(u64), ctx->stream));
    if (r.compact) {
        wi_unit_index_c40_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.uidx, r.nu, r.LF40);
        wi_unit_nodes_c40_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.uidx, r.ulf, r.nu, r.LF40, r.unit.nodes);
    } else {
        wi_unit_index_kernel<u64><<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.uidx, r.nu, r.LF);
        wi_unit_nodes_kernel<u64><<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.uidx, r.ulf, r.nu, r.LF, r.unit.nodes);
    }
    wi_rank_nodes(ctx, r.nu, r.unit.nodes, r.unit.rk);
    wi_finish_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(r.nu, r.unit.rk.min_of(), r.unit.rk.sum_of(), r.unit.nodes, r.unit.dist, r.unit.min_dist, r.cyc,
                                                             inv_counter(ctx, IC_UNIT_CYCLES));
    HIPC(hipGetLastError());
    BWTS_TRY(read_small(ctx, SMI_COUNTERS + IC_UNIT_CYCLES, 1));
    r.kt = inv_count(ctx, IC_UNIT_CYCLES);          // these cycles take the place of the one-lane scan's
    r.rep[IR_KT] = r.kt;
    if (r.kt == 0 || r.kt > r.nu) return BWTS_E_INTERNAL;
    wi_unit_tag_kernel<<<dim3(grid1(r.kt)), dim3(256), 0, ctx->stream>>>(r.cyc, r.kt);
    return launched(ctx);
}
// all cycles by smallest element, the ends of their stretches of text, every node's place
static int wide_order_cycles(bwts_ctx *ctx, WideRun &r)
{
    const u64 kall = r.kc + r.kt;
    ctx->tm.factors = kall;
    SpanGuard sg(ctx, BWTS_K_LISTRANK, kall, 0);
    HIPC(hipMemcpyAsync(r.cyc + r.kt, r.ncyc, r.kc * sizeof(WiCycle), hipMemcpyDeviceToDevice, ctx->stream));
    SortPlan cp;
    BWTS_TRY(cycle_sort_plan(ctx, kall, &cp));
    wi_cycle_keys_kernel<<<dim3(grid1(kall)), dim3(256), 0, ctx->stream>>>(r.cyc, kall, cp.keys[0], cp.vals[0]);
    int res = 0, kbits = bit_length(r.n - 1);
    BWTS_TRY(radix_sort_pairs(ctx, cp, kall, kbits < 1 ? 1 : kbits, &res));
    WiLenIn lin{r.cyc, cp.vals[res]};
    WiEndOut lout{r.cyc, cp.vals[res], kall, r.n - 1, r.end_by_leader, r.end_of_cyc, ctx->d_small + SMI_COUNTERS + IC_LENGTH_SUM, r.uend};
    BWTS_TRY((device_scan<false, u64>(ctx, kall, lin, lout, OpAdd(), (u64)0, cp.scan_temp)));
    wi_place_kernel<<<dim3(grid1(r.s_all)), dim3(256), 0, ctx->stream>>>(r.s_all, r.rk.min_of(), r.rk.sum_of(), r.dist, r.min_dist, r.end_by_leader, r.opos, r.wrap_at, r.cyc_len);
    return launched(ctx);
}
static int wide_place(bwts_ctx *ctx, WideRun &r, u8 *d_out)
{
    {
        SpanGuard sg(ctx, BWTS_K_WALK_EMIT, r.n, 2 * r.n);
        // threads per node: 16 (the full form's records loop over 4 G); in the compact form one per 16 bytes of a slot, at most 64
        int tpn_log2 = WI_G_LOG2 - 4;
        if (r.compact) { tpn_log2 = 2; while (tpn_log2 < 6 && (16u << (tpn_log2 + 1)) <= r.slot) tpn_log2++; }
        const u64 threads = r.s_all << tpn_log2;
        place_segments_wide_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream>>>(r.seg, r.s_all, r.slot, tpn_log2, r.nodes, r.opos, r.wrap_at,
                                                                                                           r.cyc_len, d_out);
        if (r.unit_rank)
            wi_unit_place_kernel<u64><<<dim3(grid1(r.nu)), dim3(256), 0, ctx->stream>>>(r.nu, r.unit.rk.min_of(), r.unit.rk.sum_of(), r.unit.dist, r.unit.min_dist, r.uend, r.ulf,
                                                                                        r.dC, d_out);
        else if (r.kt && r.compact) tiny_place_c40_kernel<<<dim3(grid1(r.kt)), dim3(256), 0, ctx->stream>>>(r.cyc, r.kt, r.end_of_cyc, r.LF40, r.dC, d_out);
        else if (r.kt) tiny_place_wide_kernel<<<dim3(grid1(r.kt)), dim3(256), 0, ctx->stream>>>(r.cyc, r.kt, r.end_of_cyc, r.LF, r.dC, d_out);
        HIPC(hipGetLastError());
    }
    BWTS_TRY(read_small(ctx, SMI_COUNTERS + IC_LENGTH_SUM, 1));
    return inv_count(ctx, IC_LENGTH_SUM) == r.n ? BWTS_OK : BWTS_E_INTERNAL;
}
// One attempt of one form with one way of finding the unreached elements: the stages in order
static int inverse_wide_attempt(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, bool moments, bool compact, bool *need_marks)
{
    *need_marks = false;
    if (n > (1ull << 36)) return BWTS_E_RANGE;
    WideRun r(ctx, n, moments, compact);
    if (r.node_cap > 0xfffffff0ull) return BWTS_E_RANGE;
    BWTS_TRY(wide_reserve(ctx, r));
    BWTS_TRY(wide_build_lf(ctx, r, d_in));
    BWTS_TRY(wide_walk(ctx, r));
    BWTS_TRY(wide_collect_unreached(ctx, r, need_marks));
    if (*need_marks) { r.rep[IR_OUTCOME] = INV_NEED_LOG; return BWTS_OK; }       // the moments gave up: in this form the marks come next (bwts_test.h says so for outcome 3)
    BWTS_TRY(wide_rank_node_list(ctx, r));
    BWTS_TRY(wide_free_cycles(ctx, r));
    BWTS_TRY(wide_order_cycles(ctx, r));
    BWTS_TRY(wide_place(ctx, r, d_out));
    r.rep[IR_OUTCOME] = INV_DONE;
    return BWTS_OK;
}
static int inverse_wide_form(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, bool compact)
{
    // unreached elements from per-range moments; the byte map when too many are missing (or BWTS_INV_MARK=bytemap / BWTS_BYTEMARK=1)
    const char *me = bwts_knob(ctx, "BWTS_INV_MARK");
    bool moments = !((me && !strcmp(me, "bytemap")) || bwts_knob(ctx, "BWTS_BYTEMARK"));
    bool need_marks = false;
    if (moments) {
        BWTS_TRY(inverse_wide_attempt(ctx, d_in, n, d_out, true, compact, &need_marks));
        if (!need_marks) return BWTS_OK;
    }
    return inverse_wide_attempt(ctx, d_in, n, d_out, false, compact, &need_marks);
}
static int inverse_wide_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out)
{
    // the full form where its memory can be had (about 13 n: up to ~16 GiB on one MI355X), the compact form (about 7.5 n) beyond;
    // BWTS_WIDE_INV=full|compact forces one of them (tests)
    const char *f = bwts_knob(ctx, "BWTS_WIDE_INV");
    const bool only_full = f && !strcmp(f, "full"), only_compact = f && !strcmp(f, "compact");
    if (!only_compact) {
        const int rc = inverse_wide_form(ctx, d_in, n, d_out, false);
        if (rc != BWTS_E_NOMEM || only_full) return rc;
        // nothing of the failed attempt is live: its arena and side blocks go back before the compact form reserves its own
        BWTS_TRY(arena_release(ctx));
        BWTS_TRY(aux_release(ctx));
    }
    return inverse_wide_form(ctx, d_in, n, d_out, true);
}
