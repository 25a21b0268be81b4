// api_test.hip -- what include/bwts_test.h declares: the harness utilities (generate, device buffers, compare) and the bwts_debug_*
// hooks the test suite drives.  No product path calls into this file.
#include "internal.h"
#include "../../include/bwts_test.h"
#include "ec_plan.h"
#include "zrl_plan.h"
#include "planes_plan.h"
#include "pack_plan.h"
#include "members_plan.h"
#include "key_plan.h"

#include <stdlib.h>
#include <string.h>

extern "C" int bwts_generate_device(bwts_ctx *ctx, int kind, uint64_t seed, uint64_t n, void *d_out)
{
    if (!ctx || !d_out) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    return generate_device_impl(ctx, kind, seed, n, (u8 *)d_out);
}

extern "C" int bwts_device_alloc(bwts_ctx *ctx, uint64_t bytes, void **d_ptr)
{
    if (!ctx || !d_ptr) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    if (hipMalloc(d_ptr, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); return BWTS_E_NOMEM; }
    return BWTS_OK;
}

extern "C" int bwts_device_free(bwts_ctx *ctx, void *d_ptr)
{
    if (!ctx) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    HIPC(hipFree(d_ptr));
    return BWTS_OK;
}

extern "C" int bwts_copy_to_device(bwts_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes)
{
    if (!ctx || (bytes && (!d_dst || !h_src))) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    HIPC(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return BWTS_OK;
}

extern "C" int bwts_copy_to_host(bwts_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes)
{
    if (!ctx || (bytes && (!h_dst || !d_src))) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    HIPC(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return BWTS_OK;
}

extern "C" int bwts_device_equal(bwts_ctx *ctx, const void *d_a, const void *d_b, uint64_t bytes, int *equal)
{
    if (!ctx || !equal) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    return device_equal_impl(ctx, (const u8 *)d_a, (const u8 *)d_b, bytes, equal);
}

// ---- unit-test hooks ----
extern "C" int bwts_debug_sort_pairs(bwts_ctx *ctx, uint64_t *h_keys, uint32_t *h_vals, uint64_t m, int key_bits)
{
    if (!ctx || !h_keys || !h_vals) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    spans_reset(ctx);
    SortBufs sb;
    BlockLayout L;
    sb.declare(L, m);
    BWTS_TRY(arena_reserve(ctx, L.bytes()));
    char *base = (char *)arena_alloc(ctx, L.bytes());
    if (!base) return BWTS_E_NOMEM;
    L.place(base);
    const SortPlan plan = sb.plan();
    HIPC(hipMemcpyAsync(plan.keys[0], h_keys, m * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(plan.vals[0], h_vals, m * 4, hipMemcpyHostToDevice, ctx->stream));
    int res = 0;
    BWTS_TRY(radix_sort_pairs(ctx, plan, m, key_bits, &res));
    HIPC(hipMemcpyAsync(h_keys, plan.keys[res], m * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipMemcpyAsync(h_vals, plan.vals[res], m * 4, hipMemcpyDeviceToHost, ctx->stream));
    BWTS_TRY(spans_resolve(ctx));
    return BWTS_OK;
}

// the packed passes' ranking of one tile alone (radix.hip, rank_split): 8192 digits and validity bytes in, 8192 ranks out
extern "C" int bwts_debug_rank_steps(bwts_ctx *ctx, const uint8_t *digits, const uint8_t *valid, int atomic_items, uint32_t *ranks,
                                     uint32_t shipped[4])
{
    if (!ctx || !digits || !valid || !ranks || !shipped) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    const size_t tile = 8192;
    u8 *d_in = nullptr;
    if (hipMalloc((void **)&d_in, 2 * tile + tile * sizeof(u32)) != hipSuccess) { (void)hipGetLastError(); return BWTS_E_NOMEM; }
    u32 *d_ranks = (u32 *)(d_in + 2 * tile);
    int rc = BWTS_OK;
    if (hipMemcpyAsync(d_in, digits, tile, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(d_in + tile, valid, tile, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = BWTS_E_HIP;
    if (rc == BWTS_OK) rc = radix_debug_rank_steps(ctx, d_in, d_in + tile, atomic_items, d_ranks, shipped);
    if (rc == BWTS_OK && hipMemcpyAsync(ranks, d_ranks, tile * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = BWTS_E_HIP;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == BWTS_OK) rc = BWTS_E_HIP;
    (void)hipFree(d_in);
    return rc;
}

static int upload_text(bwts_ctx *ctx, const uint8_t *in, uint64_t n, u8 **d_T)
{
    void *p = nullptr;
    if (hipMalloc(&p, n) != hipSuccess) { (void)hipGetLastError(); return BWTS_E_NOMEM; }
    if (hipMemcpyAsync(p, in, n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) { (void)hipFree(p); return BWTS_E_HIP; }
    *d_T = (u8 *)p;
    return BWTS_OK;
}

// the chunk tables' arithmetic for a tied list of a0 elements of which a_chunks are left at a compaction, with cuts that aim at
// `target` chunks: no context, no device.  The re-cut always fits (chunk_table_capacity): the return value says so
extern "C" int bwts_debug_chunk_plan_target(uint64_t a0, uint64_t a_chunks, uint32_t target, uint64_t out[4])
{
    if (!out || target < 16 || target > CH_CHUNK_TARGET) return -1;
    const ChunkRecut re = chunk_recut_plan(a_chunks, target);
    out[0] = chunk_nominal_size(a0, target); out[1] = chunk_table_capacity(a0); out[2] = re.S; out[3] = re.nc;
    return re.nc <= out[1] ? 1 : 0;
}
extern "C" int bwts_debug_chunk_plan(uint64_t a0, uint64_t a_chunks, uint64_t out[4])
{
    return bwts_debug_chunk_plan_target(a0, a_chunks, CH_CHUNK_TARGET, out);
}

// the round-0 key layout of a sort from its byte histogram (key_plan.h): no context, no device
extern "C" int bwts_debug_key_plan(const uint64_t hist[256], uint64_t n, int reserve_pad, int key_symbols, int varlen, int key_bits,
                                   int kb_emp, const double *partners_of, uint64_t out[BWTS_KEY_PLAN_WORDS], uint8_t codes[256],
                                   uint64_t vtab[256])
{
    static_assert(BWTS_KEY_KNOB_ABSENT == KEY_KNOB_ABSENT, "the value bwts_test.h states");
    if (!hist || !out || !codes || !vtab || n == 0) return -1;
    u64 sum = 0;
    for (int c = 0; c < 256; c++) {
        if (hist[c] > n - sum) return -1;
        sum += hist[c];
    }
    if (sum != n) return -1;
    KeyKnobs knobs;
    knobs.key_symbols = key_symbols; knobs.varlen = varlen; knobs.key_bits = key_bits;
    KeySample sample;
    sample.kb_emp = kb_emp;
    if (partners_of) memcpy(sample.partners_of, partners_of, sizeof sample.partners_of);
    KeyPlan P;
    key_plan(hist, n, reserve_pad != 0, knobs, sample, &P);
    const Alphabet &al = P.al;
    u64 avg_bits;
    memcpy(&avg_bits, &P.avg, 8);
    const u64 words[BWTS_KEY_PLAN_WORDS] = {(u64)al.sigma, (u64)al.bits, (u64)al.pad_add, (u64)al.msym, (u64)al.key_bits, al.varlen ? 1u : 0u,
                                            (u64)al.hstep, (u64)al.patch_span, al.few_ties ? 1u : 0u, (u64)P.lmax, (u64)P.kb_iid,
                                            (u64)P.passes_fixed, (u64)P.passes_var, avg_bits, P.code_built ? 1u : 0u, (u64)P.kb};
    memcpy(out, words, sizeof words);
    memcpy(codes, P.codes, 256);
    memcpy(vtab, P.vtab, sizeof P.vtab);
    return 0;
}

// the move-to-front stage's cut of one input of n bytes: tile size, tiles per group, tiles, groups.  No context, no device
extern "C" int bwts_debug_mtf_plan(uint64_t n, uint64_t out[4])
{
    if (n == 0 || !out) return -1;
    bwts_mtf_plan(n, out);
    return 0;
}

// the entropy coder's cut of one input of n bytes: tile size, tiles per block, tiles, blocks, the bound.  No context, no device
extern "C" int bwts_debug_ec_plan(uint64_t n, uint64_t out[5])
{
    if (n == 0 || n > EC_MAX_N || !out) return -1;
    bwts_ec_plan(n, out);
    return 0;
}

// the checksum's cut of one input of n bytes: tile size, tiles per fold group, tiles, groups.  No context, no device
extern "C" int bwts_debug_crc_plan(uint64_t n, uint64_t out[4])
{
    if (n == 0 || n > CRC_MAX_N || !out) return -1;
    bwts_crc_plan(n, out);
    return 0;
}

// the zero-run stage's cut of one input of n bytes: tile size, tiles.  No context, no device
extern "C" int bwts_debug_zrl_plan(uint64_t n, uint64_t out[2])
{
    if (n == 0 || n > ZRL_MAX_N || !out) return -1;
    bwts_zrl_plan(n, out);
    return 0;
}

// the byte-plane split's cut of one input of n bytes at a width: tile bytes, tiles, elements, tail bytes.  No context, no device
extern "C" int bwts_debug_planes_plan(uint64_t n, uint32_t width, uint64_t out[4])
{
    if (n == 0 || n > PLANES_MAX_N || !planes_width_ok(width) || !out) return -1;
    bwts_planes_plan(n, width, out);
    return 0;
}

// what a range read of a frame would decode and move (ranges_plan in members_plan.h): the frame's header and directory alone are read.  No context, no device
extern "C" int bwts_debug_unpack_ranges_plan(const uint8_t *frame, uint64_t in_bytes, const uint64_t *ranges, uint64_t count, uint64_t out_cap,
                                             uint64_t out[8], uint64_t *lists, uint64_t cap_words)
{
    if (!frame || !out || (!lists && cap_words)) return -1;
    Frame F;
    u64 sum = 0;
    PackRangesPlan P;
    std::vector<PackRange> whole;
    const PackRange *rs = nullptr;
    BWTS_TRY(frame_ranges_plan(frame, in_bytes, (const PackRange *)ranges, nullptr, count, out_cap, &F, &sum, &whole, &rs, &P));
    const u64 runs = P.runs.size(), words = 5 * runs + 3 * count;
    const u64 head[8] = {(u64)P.blocks.size(), runs, P.covered_bytes, P.stream_bytes, P.coded_bytes, P.out_bytes, PIECES_T, words};
    memcpy(out, head, sizeof head);
    if (words > cap_words) return 0;
    for (const PackRun &r : P.runs) { *lists++ = r.first; *lists++ = r.blocks; }
    for (const PackPiece &s : P.streams) { *lists++ = s.src; *lists++ = s.dst; *lists++ = s.bytes; }
    for (const PackPiece &o : P.out) { *lists++ = o.src; *lists++ = o.dst; *lists++ = o.bytes; }
    return 0;
}

// what the most recent range read on this context did: no device, the record is host memory
extern "C" int bwts_debug_unpack_ranges_report(bwts_ctx *ctx, uint64_t out[8])
{
    if (!ctx || !out) return BWTS_E_ARG;
    memcpy(out, ctx->ranges_report, sizeof ctx->ranges_report);
    return BWTS_OK;
}

// the device time of every timed launch of the most recent call, in launch order (timing level 2: every launch has a span; the events
// stay with the context until the next call)
extern "C" int bwts_debug_last_spans(bwts_ctx *ctx, double *ms, uint64_t cap)
{
    if (!ctx || (!ms && cap)) return BWTS_E_ARG;
    int k = 0;
    for (const TimedSpan &sp : ctx->spans) {
        if ((u64)k >= cap) break;
        float t = 0.f;
        if (hipEventElapsedTime(&t, sp.a, sp.b) != hipSuccess) { (void)hipGetLastError(); t = -1.f; }
        ms[k++] = t;
    }
    return k;
}

// what a segmented inverse would do with segments of these lengths (the cost estimate's choice; test switches do not apply): no
// context, no device
extern "C" int bwts_debug_segments_plan(const uint64_t *lengths, uint64_t count, uint64_t out[8])
{
    if (!lengths || !out || count == 0) return -1;
    return inverse_segments_plan_words(lengths, count, out);
}

// what the most recent segmented inverse on this context did: no device, the record is host memory
extern "C" int bwts_debug_segments_report(bwts_ctx *ctx, uint64_t out[8])
{
    static_assert(SEG_REPORT_WORDS == 8, "the record layout bwts_test.h states");
    if (!ctx || !out) return BWTS_E_ARG;
    memcpy(out, ctx->seg_report, sizeof ctx->seg_report);
    return BWTS_OK;
}

// the narrow inverse's arena as plain arithmetic: no context, no device
extern "C" int bwts_debug_inverse_arena(uint64_t n, int g, int mark, uint64_t out[2])
{
    if (n == 0 || n > NARROW_N || g > 20 || mark < 0 || mark > 3) return -1;
    if (g < 0) g = inverse_splitter_log2(n);
    out[0] = inverse_attempt_bytes(n, g, mark); out[1] = inverse_arena_bytes(n);
    return g;
}

// the narrow forward's arena, likewise: the bytes its declared layout takes
extern "C" int bwts_debug_forward_arena(uint64_t n, uint64_t out[1])
{
    if (n == 0 || n > NARROW_N || !out) return -1;
    out[0] = forward_arena_bytes(n);
    return 0;
}

// the wide forward's arena (wide_path.h), likewise
extern "C" int bwts_debug_wide_forward_arena(uint64_t n, int mode, int seg_log2, uint64_t bucket_cap, uint64_t out[1])
{
    return forward_wide_arena_probe(n, mode, seg_log2, bucket_cap, out);
}

// what the attempts of the most recent inverse call on this context did: no device, the records are host memory
extern "C" int bwts_debug_inverse_report(bwts_ctx *ctx, uint64_t *out, uint64_t cap_words, uint64_t *attempts)
{
    if (!ctx || !attempts || (!out && cap_words)) return BWTS_E_ARG;
    *attempts = ctx->inv_attempts_made;
    int copied = 0;
    for (u32 a = 0; a < ctx->inv_attempts_made && a < INV_REPORT_MAX && (u64)(a + 1) * INV_REPORT_WORDS <= cap_words; a++, copied++)
        memcpy(out + (size_t)a * INV_REPORT_WORDS, ctx->inv_report[a], INV_REPORT_WORDS * sizeof(u64));
    return copied;
}

// what the doubling sorts of the most recent forward call on this context did: no device, the records are host memory
extern "C" int bwts_debug_forward_report(bwts_ctx *ctx, uint64_t *out, uint64_t cap_words, uint64_t *sorts)
{
    static_assert(FWD_HEADER_WORDS == BWTS_FWD_HEADER_WORDS && FWD_ROUND_WORDS == BWTS_FWD_ROUND_WORDS, "the record layout bwts_test.h states");
    if (!ctx || !sorts || (!out && cap_words)) return BWTS_E_ARG;
    *sorts = ctx->fwd_sorts_made;
    int copied = 0;
    for (u32 a = 0; a < ctx->fwd_sorts_made && a < FWD_REPORT_SORTS && (u64)(a + 1) * FWD_SORT_WORDS <= cap_words; a++, copied++)
        memcpy(out + (size_t)a * FWD_SORT_WORDS, ctx->fwd_report[a], FWD_SORT_WORDS * sizeof(u64));
    return copied;
}

extern "C" int bwts_debug_suffix_array(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint32_t *h_sa)
{
    if (!ctx || !in || !h_sa || n == 0) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    spans_reset(ctx);
    u8 *d_T = nullptr;
    BWTS_TRY(upload_text(ctx, in, n, &d_T));
    int rc = arena_reserve(ctx, forward_arena_bytes(n));
    u32 *sa = nullptr, *rank = nullptr, rounds = 0;
    if (rc == BWTS_OK) rc = suffix_sort_device(ctx, d_T, n, &sa, &rank, &rounds);
    if (rc == BWTS_OK && hipMemcpyAsync(h_sa, sa, n * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = BWTS_E_HIP;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == BWTS_OK) rc = BWTS_E_HIP;
    (void)hipFree(d_T);
    return rc;
}

extern "C" int bwts_debug_lyndon(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint64_t *h_starts, uint64_t cap, uint64_t *count)
{
    if (!ctx || !in || !h_starts || !count || n == 0) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    spans_reset(ctx);
    u8 *d_T = nullptr;
    BWTS_TRY(upload_text(ctx, in, n, &d_T));
    int rc = arena_reserve(ctx, forward_arena_bytes(n));
    u32 *fstart = nullptr, rounds = 0;
    u64 k = 0;
    if (rc == BWTS_OK) rc = lyndon_factors_device(ctx, d_T, n, &fstart, &k, &rounds);
    if (rc == BWTS_OK) {
        const u64 take = k < cap ? k : cap;
        u32 *tmp = (u32 *)malloc((size_t)(take ? take : 1) * 4);
        if (!tmp) rc = BWTS_E_NOMEM;
        else {
            // on the context's stream: it is non-blocking, so the null stream would not wait for the factor list's last copy
            if (hipMemcpyAsync(tmp, fstart, take * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                hipStreamSynchronize(ctx->stream) != hipSuccess) rc = BWTS_E_HIP;
            for (u64 i = 0; i < take; i++) h_starts[i] = tmp[i];
            free(tmp);
        }
        *count = k;
    }
    (void)hipFree(d_T);
    return rc;
}
