// estimate.hip -- the plane costs of every member under both filters (include/bwts_members.h, "The estimate"): what
// the order-0 coder would make of a member's byte planes as they are, and of the planes of its zigzagged differences, in one read of
// the input.  The definition is exact integer arithmetic and is stated in estimate_plan.h, which host and device share;
// tests/estimate_model.py is its executable form.
//
// A member is cut into units of 2^18 elements of w bytes, no unit across a member's start; a workgroup of 256 threads works on one unit
// and walks it in delta.hip's tiles: 4096 elements, every thread 16 consecutive ones, which it takes as w 16-byte loads
// (planes_load16: any alignment, nothing read outside the call's input).  The element in front of a thread's first comes from the lane
// below; the first lane of a wave reads it from memory, byte by byte, and a member's first element has 0 in front of it -- never its
// neighbour's last element.
// The 2 w histograms of a unit lie in LDS, each in several copies that the waves share out among themselves.  A plane that holds one
// value (the high bytes of small integers, every plane of a smooth field's differences) must not queue 256 threads on one counter: as in
// ec.hip's histogram, a thread adds a run's length when the run ends -- a thread's consecutive elements are the member's consecutive
// elements -- and a pending run is carried from tile to tile.
// Behind the walk every thread takes one symbol of every histogram: the copies' sum c, the term c lg(c), and a sum over the workgroup;
// cost and byte rounding follow, and one thread writes the unit's two sums.  The members' sums are a host loop over these values, which
// are read back anyway: no global atomic, and no workgroup waits for another.
// Working memory: 16 bytes per unit in the context's arena.
#include "internal.h"
#include "device_utils.h"
#include "load16.h"
#include "delta_words.h"
#include "estimate_plan.h"

// copies of a histogram: one per wave, at the largest width one per two waves, so that every width's histograms fit 32 KiB
#define ESTIMATE_COPIES(w) ((w) == 8 ? 2 : 4)
#define ESTIMATE_LDS_WORDS (2u * PLANES_MAX_W * ESTIMATE_COPIES(PLANES_MAX_W) * 256u)
static_assert(2u * 4u * ESTIMATE_COPIES(4) * 256u <= ESTIMATE_LDS_WORDS, "the histograms of every width fit those of the largest");

// ec.hip's ec_count: symbol c into the bins, a run's length when the run ends
__device__ __forceinline__ void estimate_count(u32 *bins, u32 &cur, u32 &cnt, u32 c)
{
    if (c == cur) { cnt++; return; }
    if (cnt) atomicAdd(&bins[cur], cnt);
    cur = c;
    cnt = 1;
}

// unit j of the member of len bytes at seg; h: ESTIMATE_LDS_WORDS words, sm: 4 words; the unit's two costs in bytes to out[0], out[1]
template <int W>
__device__ __forceinline__ void estimate_unit(const u8 *__restrict__ in, u64 n, u64 seg, u64 len, u64 j, u32 *h, u64 *sm, u64 *out)
{
    typedef typename DeltaWord<W>::T T;
    constexpr u32 C = ESTIMATE_COPIES(W);
    const u32 tid = threadIdx.x;
    for (u32 i = tid; i < 2u * W * C * 256u; i += 256) h[i] = 0;
    __syncthreads();
    // histogram k (plane k of the elements, plane k - W of the differences), copy c: 256 words at h + (k C + c) 256
    u32 *const bins = h + ((u32)wave_id() & (C - 1u)) * 256u;
    u32 cur[2 * W], cnt[2 * W];
#pragma unroll
    for (int k = 0; k < 2 * W; k++) { cur[k] = 0; cnt[k] = 0; }
    const u64 u0 = j << ESTIMATE_LOG_UNIT;
    const u32 elems = estimate_unit_elems(len, W, j);
    for (u32 t0 = 0; t0 < elems; t0 += PLANES_E) {
        const u32 at = t0 + 16u * tid;
        if (at >= elems) continue;
        const u8 *p = in + seg + (u0 + at) * W;
        u32 D[4 * W];
        delta_load16<W>(p, in, n, D);
        // the element in front of the thread's first: the last one of the lane below (whose `at` is smaller: it is here too, with all
        // its 16 elements); a wave's first lane reads it from memory, and the member's first element has 0 in front of it
        T prev = shfl_up_t(delta_get<W>(D, 15), 1);
        if (lane_id() == 0) {
            prev = 0;
            if (u0 + at) {
#pragma unroll
                for (int k = 0; k < W; k++) prev |= (T)(p - W)[k] << (8 * k);
            }
        }
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (at + (u32)i < elems) {
                const T a = delta_get<W>(D, i), z = delta_zig<W>((T)(a - prev) & delta_mask_t<W>());
#pragma unroll
                for (int k = 0; k < W; k++) {
                    estimate_count(bins + (u32)k * C * 256u, cur[k], cnt[k], (u32)(a >> (8 * k)) & 255u);
                    estimate_count(bins + (u32)(W + k) * C * 256u, cur[W + k], cnt[W + k], (u32)(z >> (8 * k)) & 255u);
                }
                prev = a;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 2 * W; k++)
        if (cnt[k]) atomicAdd(&bins[(u32)k * C * 256u + cur[k]], cnt[k]);
    __syncthreads();
    // every histogram holds `elems` entries; thread s takes symbol s
    u64 est[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 2 * W; k++) {
        u32 c = 0;
#pragma unroll
        for (u32 cc = 0; cc < C; cc++) c += h[((u32)k * C + cc) * 256u + tid];
        u64 terms;
        block_scan_exclusive<u64, OpAdd, 4>(estimate_term(c), OpAdd(), (u64)0, sm, &terms);
        est[k / W] += estimate_bytes(elems, terms);
    }
    if (tid == 0) { out[0] = est[0]; out[1] = est[1]; }
}

// The members of a call: first and w lie behind the context's table, first[count + 1] (estimate_cut) and then a width per member.
struct EstimateSegs {
    const u64 *off, *first, *w;
    u64 count, n;
};

// the member of unit u: the last one whose first unit is not behind u (a member without units shares its first with the next member
// that has one, which stands behind it)
__global__ __launch_bounds__(256) void estimate_kernel(const u8 *__restrict__ in, EstimateSegs S, u64 *__restrict__ costs)
{
    __shared__ u32 h[ESTIMATE_LDS_WORDS];
    __shared__ u64 sm[4];
    const u64 u = blockIdx.x, s = planes_tile_segment(S.first, S.count, u);
    const u64 seg = S.off[s], len = S.off[s + 1] - seg, j = u - S.first[s];
    u64 *out = costs + 2 * u;
    // (the width is the same for the whole workgroup: one branch, taken together)
    switch ((u32)S.w[s]) {
    case 1: estimate_unit<1>(in, S.n, seg, len, j, h, sm, out); break;
    case 2: estimate_unit<2>(in, S.n, seg, len, j, h, sm, out); break;
    case 4: estimate_unit<4>(in, S.n, seg, len, j, h, sm, out); break;
    default: estimate_unit<8>(in, S.n, seg, len, j, h, sm, out); break;
    }
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
// The estimates of the members of the context's table (one member too) that `take` names (null: all of them; the others get 0), to
// the host: est_none[s], est_delta[s].  widths: one per member, judged by the caller.
int estimate_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, const u32 *widths, const u8 *take, u64 *est_none, u64 *est_delta)
{
    const u64 count = ctx->seg_off.size() - 1;
    std::vector<u64> words((size_t)(2 * count + 1));
    const u64 units = estimate_cut(ctx->seg_off.data(), widths, take, count, words.data());
    for (u64 s = 0; s < count; s++) { words[(size_t)(count + 1 + s)] = widths[s]; est_none[s] = est_delta[s] = 0; }
    if (units == 0) return BWTS_OK;
    if (units >= (1ull << 31)) return BWTS_E_RANGE;
    u64 *d_words = nullptr, *costs = nullptr;
    BWTS_TRY(seg_upload_extra(ctx, words.data(), 2 * count + 1, &d_words));
    BlockLayout L;
    L.array(&costs, 2 * units);
    BWTS_TRY(arena_take(ctx, L));
    std::vector<u64> got((size_t)(2 * units));
    {
        SpanGuard sp(ctx, BWTS_K_OTHER, n, n);
        const EstimateSegs S = {d_seg_off(ctx), d_words, d_words + count + 1, count, n};
        estimate_kernel<<<dim3((unsigned)units), dim3(256), 0, ctx->stream>>>(d_in, S, costs);
        HIPC(hipGetLastError());
    }
    HIPC(hipMemcpyAsync(got.data(), costs, got.size() * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    for (u64 s = 0; s < count; s++)
        for (u64 u = words[(size_t)s]; u < words[(size_t)s + 1]; u++) { est_none[s] += got[(size_t)(2 * u)]; est_delta[s] += got[(size_t)(2 * u + 1)]; }
    return BWTS_OK;
}
