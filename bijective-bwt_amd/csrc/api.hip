// api.hip -- the C-ABI of include/bwts.h and its stage headers: knobs, timing spans, the context, the bracket around every device call,
// the transform table, the entry points, introspection.  (Device memory: ctx_memory.hip; caller memory: staging.hip; test hooks: api_test.hip.)
#include "internal.h"
#include "../../include/bwts_mtf.h"
#include "../../include/bwts_ec.h"
#include "../../include/bwts_zrl.h"
#include "../../include/bwts_planes.h"
#include "../../include/bwts_pack.h"
#include "ec_plan.h"
#include "zrl_plan.h"
#include "planes_plan.h"
#include "pack_plan.h"
#include "members_plan.h"
#include "estimate_plan.h"
#include "../../include/bwts_members.h"
#include "../../include/bwts_delta.h"

#include <algorithm>
#include <new>
#include <stdio.h>
#include <time.h>
#include <stdlib.h>
#include <string.h>

double wall_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return 1e3 * (double)ts.tv_sec + 1e-6 * (double)ts.tv_nsec;
}

void bwts_trace_error(const char *file, int line, int rc)
{
    static const bool on = [] { const char *e = getenv("BWTS_TRACE_ERRORS"); return e && e[0] == '1'; }();
    if (on) fprintf(stderr, "[bwts] %s:%d: rc %d\n", file, line, rc);
}

// ------------------------------------------------------------------------------------
// environment knobs
// ------------------------------------------------------------------------------------
// Read once per context.  Always: diagnostics and the staging tuning below.  Everything else selects alternate code paths that exist
// for the test suite (tests/test_gpu_parity.py::test_alternate_paths) and for A/B timing sessions: those are only looked at when
// BWTS_TEST_KNOBS=1 is set, so a process that merely inherits a stray BWTS_* variable runs the product paths.
static const char *const kPublicKnobs[] = {"BWTS_TIMINGS", "BWTS_TRACE_ERRORS", "BWTS_ROUND_TRACE", "BWTS_INV_TRACE", "BWTS_BATCH_TRACE",
                                           "BWTS_COPY_THREADS", "BWTS_H2D", "BWTS_D2H", "BWTS_D2H_SPLIT"};
extern char **environ;

static void read_knobs(bwts_ctx *ctx)
{
    const char *gate = getenv("BWTS_TEST_KNOBS");
    const bool all = gate && gate[0] == '1';
    for (char **e = environ; e && *e; e++) {
        if (strncmp(*e, "BWTS_", 5) != 0) continue;
        const char *eq = strchr(*e, '=');
        if (!eq) continue;
        std::string name(*e, (size_t)(eq - *e));
        bool pub = false;
        for (const char *k : kPublicKnobs) if (name == k) pub = true;
        if (pub || all) ctx->knobs.emplace_back(name, std::string(eq + 1));
    }
}

const char *bwts_knob(const bwts_ctx *ctx, const char *name)
{
    for (const auto &kv : ctx->knobs) if (kv.first == name) return kv.second.c_str();
    return nullptr;
}

void bwts_stage_mark(bwts_ctx *ctx, const char *name)
{
    static int on = -1;
    if (on < 0) { const char *e = getenv("BWTS_STAGE_TRACE"); on = (e && e[0] == '1') ? 1 : 0; }
    if (!on) return;
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    fprintf(stderr, "[bwts stage] %s %s\n", name, e == hipSuccess ? "ok" : "FAILED");
    fflush(stderr);
}

int ensure_dyn_lds(bwts_ctx *ctx, const void *kernel, size_t bytes)
{
    for (const void *k : ctx->lds_granted) if (k == kernel) return BWTS_OK;
    HIPC(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    ctx->lds_granted.push_back(kernel);
    return BWTS_OK;
}

// ------------------------------------------------------------------------------------
// timing spans
// ------------------------------------------------------------------------------------
static hipEvent_t take_event(bwts_ctx *ctx)
{
    if (ctx->ev_used == ctx->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        ctx->ev_pool.push_back(e);
    }
    return ctx->ev_pool[ctx->ev_used++];
}

void spans_reset(bwts_ctx *ctx)
{
    ctx->ev_used = 0;
    ctx->spans.clear();
    memset(&ctx->tm, 0, sizeof(ctx->tm));
}

int span_begin(bwts_ctx *ctx, int cls, u64 elems, u64 alg_bytes)
{
    ctx->tm.k[cls].launches++;
    ctx->tm.k[cls].elems += elems;
    ctx->tm.k[cls].alg_bytes += alg_bytes;
    if (ctx->timing < 2 && !(ctx->timing == 1 && (cls == BWTS_K_RADIX_SCATTER_MAIN || cls == BWTS_K_WALK || cls == BWTS_K_ROUND))) return -1;
    TimedSpan sp;
    sp.cls = cls;
    sp.a = take_event(ctx);
    sp.b = take_event(ctx);
    if (!sp.a || !sp.b) return -1;
    (void)hipEventRecord(sp.a, ctx->stream);
    ctx->spans.push_back(sp);
    return (int)ctx->spans.size() - 1;
}

void span_end(bwts_ctx *ctx, int span)
{
    if (span < 0 || (size_t)span >= ctx->spans.size()) return;
    (void)hipEventRecord(ctx->spans[span].b, ctx->stream);
}

int spans_resolve(bwts_ctx *ctx)
{
    HIPC(hipStreamSynchronize(ctx->stream));
    for (const TimedSpan &sp : ctx->spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) ctx->tm.k[sp.cls].ms += ms;
    }
    return BWTS_OK;
}

int read_small(bwts_ctx *ctx, int first, int count)
{
    HIPC(hipMemcpyAsync(ctx->h_small + first, ctx->d_small + first, (size_t)count * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    return BWTS_OK;
}

// ------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------
extern "C" int bwts_ctx_create(bwts_ctx **out, int device_id)
{
    if (!out) return BWTS_E_ARG;
    *out = nullptr;
    const double t_create = wall_ms();
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); return BWTS_E_NODEVICE; }
    if (device_id < 0 || device_id >= count) return BWTS_E_NODEVICE;
    bwts_ctx *ctx = new (std::nothrow) bwts_ctx();
    if (!ctx) return BWTS_E_NOMEM;
    ctx->device = device_id;
    read_knobs(ctx);
    { const char *e = bwts_knob(ctx, "BWTS_TIMINGS"); ctx->timing = (e && e[0] == '1') ? 2 : 0; }
    { const char *e = bwts_knob(ctx, "BWTS_GUARD"); const int mib = e ? atoi(e) : 0; ctx->guard = mib >= 1 && mib <= 256 ? ((size_t)mib << 20) : 0; }     // MiB per band
    if (hipSetDevice(device_id) != hipSuccess) { delete ctx; return BWTS_E_NODEVICE; }
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return BWTS_E_HIP; }
    void *p = nullptr;
    if (ctx_malloc(ctx, &p, 4096 * sizeof(u64), "small words") != hipSuccess) { bwts_ctx_destroy(ctx); return BWTS_E_NOMEM; }
    ctx->d_small = (u64 *)p;
    if (hipMemset(p, 0, 4096 * sizeof(u64)) != hipSuccess) { bwts_ctx_destroy(ctx); return BWTS_E_HIP; }     // (counters that kernels expect at zero)
    if (hipHostMalloc(&p, 4096 * sizeof(u64), hipHostMallocDefault) != hipSuccess) { bwts_ctx_destroy(ctx); return BWTS_E_NOMEM; }
    trace_alloc(ctx, "pinned +", "small words", p, 4096 * sizeof(u64));
    ctx->h_small = (u64 *)p;
    if (hipEventCreate(&ctx->ev_begin) != hipSuccess || hipEventCreate(&ctx->ev_end) != hipSuccess) { bwts_ctx_destroy(ctx); return BWTS_E_HIP; }
    ctx->host_ms[BWTS_H_INIT] = wall_ms() - t_create;
    *out = ctx;
    return BWTS_OK;
}

extern "C" void bwts_ctx_destroy(bwts_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->ev_begin) (void)hipEventDestroy(ctx->ev_begin);
    if (ctx->ev_end) (void)hipEventDestroy(ctx->ev_end);
    for (KeptBlock &b : ctx->kept) (void)kept_give_up(ctx, b);
    (void)tied_release(ctx);
    if (ctx->d_small) (void)ctx_free(ctx, ctx->d_small);
    seg_pinned_free(ctx);
    for (const auto &b : ctx->guard_freed) (void)hipFree(b.user - ctx->guard);
    ctx->guard_freed.clear();
    if (ctx->h_small) (void)hipHostFree(ctx->h_small);
    staging_destroy(ctx);
    for (const auto &b : ctx->host_blocks) (void)hipHostFree(b.first);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// A context keeps what its last calls allocated on the device (a 12 GiB input leaves ~100-200 GiB there) so that the next call starts at
// once; a caller who wants the memory back without giving up the context asks for it here.  Pinned staging and the small blocks (the
// small words, the segment table) stay.
extern "C" int bwts_ctx_release_memory(bwts_ctx *ctx)
{
    if (!ctx) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    HIPC(hipStreamSynchronize(ctx->stream));
    ctx->arena_off = 0;
    for (int i = 0; i < KB_COUNT; i++)
        if (i != KB_SEG_TABLE) BWTS_TRY(kept_give_up(ctx, ctx->kept[i]));
    return tied_release(ctx);
}

// ------------------------------------------------------------------------------------
// transforms
// ------------------------------------------------------------------------------------
// The eight transforms that map n bytes to n bytes (the rows: internal.h).  The transform and its inverse allocate ahead only up to
// 2^32 positions; the wide forms size their arenas themselves.
static const Transform kForward = {forward_device_impl, "forward", "forward: in", [](const bwts_ctx *, u64 n) { return n <= NARROW_N ? forward_arena_bytes(n) : 0; }};
static const Transform kInverse = {inverse_device_impl, "inverse", "inverse: in", [](const bwts_ctx *, u64 n) { return n <= NARROW_N ? inverse_arena_bytes(n) : 0; }};
static const Transform kForwardSegments = {forward_segments_impl, "forward", "forward: in", kForward.arena_hint};
static const Transform kInverseSegments = {inverse_segments_impl, "inverse", "inverse: in",
                                           [](const bwts_ctx *ctx, u64 n) { return n <= NARROW_N ? inverse_segments_arena_bytes(ctx, n) : 0; }};
// (move-to-front is one function: its four rows say which direction, and whether the context's table is meant)
static const Transform kMtfForward = {[](bwts_ctx *ctx, const u8 *in, u64 n, u8 *out) { return mtf_impl(ctx, in, n, out, false, SEG_SINGLE); }, "mtf forward", "mtf: in",
                                      [](const bwts_ctx *ctx, u64 n) { return mtf_arena_bytes(ctx, n, SEG_SINGLE); }};
static const Transform kMtfInverse = {[](bwts_ctx *ctx, const u8 *in, u64 n, u8 *out) { return mtf_impl(ctx, in, n, out, true, SEG_SINGLE); }, "mtf inverse", "mtf: in",
                                      kMtfForward.arena_hint};
static const Transform kMtfForwardSegments = {[](bwts_ctx *ctx, const u8 *in, u64 n, u8 *out) { return mtf_impl(ctx, in, n, out, false, seg_mode(ctx)); }, "mtf forward",
                                              "mtf: in", [](const bwts_ctx *ctx, u64 n) { return mtf_arena_bytes(ctx, n, seg_mode(ctx)); }};
static const Transform kMtfInverseSegments = {[](bwts_ctx *ctx, const u8 *in, u64 n, u8 *out) { return mtf_impl(ctx, in, n, out, true, seg_mode(ctx)); }, "mtf inverse",
                                              "mtf: in", kMtfForwardSegments.arena_hint};

// The bracket around every device call: code object loaded outside the timing, spans, guard check, total_ms, device_bytes.  What the
// body needs beyond the context travels in its closure.  n: the uncoded bytes, where the caller knows them already.
template <typename Body>
static int run_sized(bwts_ctx *ctx, u64 n, const char *what, Body body)
{
    HIPC(hipSetDevice(ctx->device));
    spans_reset(ctx);
    ctx->tm.n = n;
    ctx->call_block_bytes = 0;
    if (!ctx->launched) {
        // the library's code object is loaded at the first launch: pay (and account for) that outside the timed transform
        const double t0 = wall_ms();
        pcie_copy_kernel<<<dim3(1), dim3(256), 0, ctx->stream>>>(nullptr, nullptr, 0, nullptr, nullptr, 0);
        HIPC(hipStreamSynchronize(ctx->stream));
        ctx->host_ms[BWTS_H_MODULE] += wall_ms() - t0;
        ctx->launched = true;
    }
    HIPC(hipEventRecord(ctx->ev_begin, ctx->stream));
    int rc = body();
    if (ctx->guard) {
        (void)hipStreamSynchronize(ctx->stream);
        const int grc = guard_check(ctx, what);
        if (rc == BWTS_OK) rc = grc;
    }
    if (rc != BWTS_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIPC(hipEventRecord(ctx->ev_end, ctx->stream));
    BWTS_TRY(spans_resolve(ctx));
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
    ctx->tm.total_ms = ms;
    ctx->tm.device_bytes = ctx_device_bytes(ctx);
    return BWTS_OK;
}

int run_device(bwts_ctx *ctx, const Transform &t, const void *d_in, u64 n, void *d_out)
{
    if (!ctx || !d_in || !d_out || n == 0) return BWTS_E_ARG;
    return run_sized(ctx, n, t.name, [&] { return t.fn(ctx, (const u8 *)d_in, n, (u8 *)d_out); });
}

extern "C" int bwts_forward_device(bwts_ctx *ctx, const void *d_in, uint64_t n, void *d_out)
{
    return run_device(ctx, kForward, d_in, n, d_out);
}

extern "C" int bwts_inverse_device(bwts_ctx *ctx, const void *d_in, uint64_t n, void *d_out)
{
    return run_device(ctx, kInverse, d_in, n, d_out);
}

// ------------------------------------------------------------------------------------
// host-buffer entry points: every one is its argument checks and one host_round_trip (staging.hip)
// ------------------------------------------------------------------------------------
static int run_host(bwts_ctx *ctx, const Transform &t, const uint8_t *in, uint64_t n, uint8_t *out, bwts_sink_fn sink, void *user)
{
    if (!ctx || !in || (!out && !sink) || n == 0) return BWTS_E_ARG;
    u64 made = 0;
    const HostTrip trip = {in, n, n, out, &made, sink, user, &t};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *d_out, u64 *bytes) { *bytes = n; return run_device(ctx, t, d_in, n, d_out); });
}

extern "C" int bwts_forward_batch(bwts_ctx *ctx, int count, const uint8_t *const *ins, const uint64_t *ns, uint8_t *const *outs)
{
    return run_batch(ctx, kForward, count, ins, ns, outs);
}

extern "C" int bwts_inverse_batch(bwts_ctx *ctx, int count, const uint8_t *const *ins, const uint64_t *ns, uint8_t *const *outs)
{
    return run_batch(ctx, kInverse, count, ins, ns, outs);
}

extern "C" int bwts_forward(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out)
{
    return run_host(ctx, kForward, in, n, out, nullptr, nullptr);
}

extern "C" int bwts_inverse(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out)
{
    return run_host(ctx, kInverse, in, n, out, nullptr, nullptr);
}

extern "C" int bwts_forward_sink(bwts_ctx *ctx, const uint8_t *in, uint64_t n, bwts_sink_fn sink, void *user)
{
    if (!sink) return BWTS_E_ARG;
    return run_host(ctx, kForward, in, n, nullptr, sink, user);
}

extern "C" int bwts_inverse_sink(bwts_ctx *ctx, const uint8_t *in, uint64_t n, bwts_sink_fn sink, void *user)
{
    if (!sink) return BWTS_E_ARG;
    return run_host(ctx, kInverse, in, n, nullptr, sink, user);
}

static int run_segments_host(bwts_ctx *ctx, const Transform &t, const uint8_t *in, const uint64_t *lengths, uint64_t count, uint8_t *out)
{
    if (!ctx || !in || !out) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    return run_host(ctx, t, in, n, out, nullptr, nullptr);
}

static int run_segments_device(bwts_ctx *ctx, const Transform &t, const void *d_in, const uint64_t *lengths, uint64_t count, void *d_out)
{
    if (!ctx || !d_in || !d_out) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    if (ranges_overlap(d_in, n, d_out, n)) return BWTS_E_ARG;
    return run_device(ctx, t, d_in, n, d_out);
}

extern "C" int bwts_forward_segments(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, uint64_t count, uint8_t *out)
{
    return run_segments_host(ctx, kForwardSegments, in, lengths, count, out);
}

extern "C" int bwts_inverse_segments(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, uint64_t count, uint8_t *out)
{
    return run_segments_host(ctx, kInverseSegments, in, lengths, count, out);
}

extern "C" int bwts_forward_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, void *d_out)
{
    return run_segments_device(ctx, kForwardSegments, d_in, lengths, count, d_out);
}

extern "C" int bwts_inverse_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, void *d_out)
{
    return run_segments_device(ctx, kInverseSegments, d_in, lengths, count, d_out);
}

// ------------------------------------------------------------------------------------
// move-to-front behind the transform (include/bwts_mtf.h): the same four plumbing routes, the kernels in mtf.hip
// ------------------------------------------------------------------------------------
extern "C" int bwts_mtf_forward_device(bwts_ctx *ctx, const void *d_in, uint64_t n, void *d_out)
{
    return run_device(ctx, kMtfForward, d_in, n, d_out);
}

extern "C" int bwts_mtf_inverse_device(bwts_ctx *ctx, const void *d_in, uint64_t n, void *d_out)
{
    return run_device(ctx, kMtfInverse, d_in, n, d_out);
}

extern "C" int bwts_mtf_forward(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out)
{
    return run_host(ctx, kMtfForward, in, n, out, nullptr, nullptr);
}

extern "C" int bwts_mtf_inverse(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out)
{
    return run_host(ctx, kMtfInverse, in, n, out, nullptr, nullptr);
}

extern "C" int bwts_mtf_forward_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, void *d_out)
{
    return run_segments_device(ctx, kMtfForwardSegments, d_in, lengths, count, d_out);
}

extern "C" int bwts_mtf_inverse_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, void *d_out)
{
    return run_segments_device(ctx, kMtfInverseSegments, d_in, lengths, count, d_out);
}

extern "C" int bwts_mtf_forward_segments(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, uint64_t count, uint8_t *out)
{
    return run_segments_host(ctx, kMtfForwardSegments, in, lengths, count, out);
}

extern "C" int bwts_mtf_inverse_segments(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, uint64_t count, uint8_t *out)
{
    return run_segments_host(ctx, kMtfInverseSegments, in, lengths, count, out);
}

// ------------------------------------------------------------------------------------
// entropy coding behind move-to-front (include/bwts_ec.h): calls whose output is not as long as their input, the kernels in ec.hip
// ------------------------------------------------------------------------------------
extern "C" uint64_t bwts_ec_bound(uint64_t n)
{
    return n == 0 || n > EC_MAX_N ? 0 : ec_bound_bytes(n);
}

extern "C" int bwts_ec_bound_segments(const uint64_t *lengths, uint64_t count, uint64_t *bound)
{
    if (!lengths || !bound || count == 0) return BWTS_E_ARG;
    u64 sum = 0, total = 0;
    for (u64 s = 0; s < count; s++) {
        if (lengths[s] == 0 || lengths[s] > ~0ull - sum) return BWTS_E_ARG;
        sum += lengths[s];
        if (sum > NARROW_N) return BWTS_E_RANGE;
        total += ec_bound_bytes(lengths[s]);
    }
    *bound = total;
    return BWTS_OK;
}

extern "C" int bwts_ec_decoded_size(const uint8_t header[16], uint64_t in_bytes, uint64_t *n)
{
    if (!header || !n) return BWTS_E_ARG;
    u64 v = 0;
    if (in_bytes < EC_HEADER_BYTES || (in_bytes & 15) || ec_header_parse(header, &v) != 0) return BWTS_E_FORMAT;
    if (v > EC_MAX_N) return BWTS_E_RANGE;
    if (in_bytes < ec_least_bytes(v) || in_bytes > ec_bound_bytes(v)) return BWTS_E_FORMAT;
    *n = v;
    return BWTS_OK;
}

extern "C" int bwts_ec_encode_device(bwts_ctx *ctx, const void *d_in, uint64_t n, void *d_out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !d_in || !d_out || !out_bytes || n == 0 || ((uintptr_t)d_out & 15)) return BWTS_E_ARG;
    if (n > EC_MAX_N) return BWTS_E_RANGE;
    if (ranges_overlap(d_in, n, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, n, "ec encode", [&] { return ec_encode_impl(ctx, (const u8 *)d_in, n, (u8 *)d_out, out_cap, SEG_SINGLE, out_bytes); });
}

extern "C" int bwts_ec_decode_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, void *d_out, uint64_t out_cap, uint64_t *n)
{
    if (!ctx || !d_in || !d_out || !n || in_bytes == 0 || ((uintptr_t)d_in & 15)) return BWTS_E_ARG;
    if (in_bytes > ec_bound_bytes(EC_MAX_N)) return BWTS_E_RANGE;
    if (ranges_overlap(d_in, in_bytes, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, 0, "ec decode", [&] { return ec_decode_impl(ctx, (const u8 *)d_in, in_bytes, (u8 *)d_out, out_cap, n, SEG_SINGLE, nullptr); });
}

extern "C" int bwts_ec_encode_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, void *d_out, uint64_t out_cap,
                                              uint64_t *stream_bytes)
{
    if (!ctx || !d_in || !d_out || !stream_bytes || ((uintptr_t)d_out & 15)) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    if (ranges_overlap(d_in, n, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, n, "ec encode", [&] { return ec_encode_impl(ctx, (const u8 *)d_in, n, (u8 *)d_out, out_cap, seg_mode(ctx), stream_bytes); });
}

extern "C" int bwts_ec_decode_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *stream_bytes, const uint64_t *lengths, uint64_t count,
                                              void *d_out)
{
    if (!ctx || !d_in || !d_out || !stream_bytes || ((uintptr_t)d_in & 15)) return BWTS_E_ARG;
    u64 n = 0, in_bytes = 0;
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    for (u64 s = 0; s < count; s++) {
        if (stream_bytes[s] > ec_bound_bytes(lengths[s])) return BWTS_E_FORMAT;       // (so the sum cannot overflow)
        in_bytes += stream_bytes[s];
    }
    if (ranges_overlap(d_in, in_bytes, d_out, n)) return BWTS_E_ARG;
    return run_sized(ctx, n, "ec decode", [&] { return ec_decode_impl(ctx, (const u8 *)d_in, n, (u8 *)d_out, n, nullptr, seg_mode(ctx), stream_bytes); });
}

// Host buffers: the checks that need no device, then one host_round_trip around the device form.
extern "C" int bwts_ec_encode(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !in || !out || !out_bytes || n == 0) return BWTS_E_ARG;
    if (n > EC_MAX_N) return BWTS_E_RANGE;
    const u64 cap = out_cap < ec_bound_bytes(n) ? out_cap : ec_bound_bytes(n);
    if (cap < ec_least_bytes(n)) return BWTS_E_SPACE;
    const HostTrip trip = {in, n, n > cap ? n : cap, out, out_bytes};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *d_out, u64 *bytes) { return bwts_ec_encode_device(ctx, d_in, n, d_out, cap, bytes); });
}

extern "C" int bwts_ec_decode(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n)
{
    if (!ctx || !in || !out || !n || in_bytes == 0) return BWTS_E_ARG;
    if (in_bytes > ec_bound_bytes(EC_MAX_N)) return BWTS_E_RANGE;
    u64 v = 0;
    BWTS_TRY(bwts_ec_decoded_size(in, in_bytes, &v));
    if (v > out_cap) return BWTS_E_SPACE;
    const HostTrip trip = {in, in_bytes, in_bytes > v ? in_bytes : v, out, n};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *d_out, u64 *got) { return bwts_ec_decode_device(ctx, d_in, in_bytes, d_out, v, got); });
}

// ------------------------------------------------------------------------------------
// zero-run coding between move-to-front and the entropy coder (include/bwts_zrl.h): the same routes as the coder's, the kernels in
// zrl.hip
// ------------------------------------------------------------------------------------
extern "C" uint64_t bwts_zrl_bound(uint64_t n)
{
    return n == 0 || n > ZRL_MAX_N ? 0 : n;
}

extern "C" int bwts_zrl_encode_device(bwts_ctx *ctx, const void *d_in, uint64_t n, void *d_out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !d_in || !d_out || !out_bytes || n == 0) return BWTS_E_ARG;
    if (n > ZRL_MAX_N) return BWTS_E_RANGE;
    if (ranges_overlap(d_in, n, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, n, "zrl encode", [&] { return zrl_encode_impl(ctx, (const u8 *)d_in, n, (u8 *)d_out, out_cap, SEG_SINGLE, out_bytes); });
}

extern "C" int bwts_zrl_decode_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, void *d_out, uint64_t n)
{
    if (!ctx || !d_in || !d_out || in_bytes == 0 || n == 0) return BWTS_E_ARG;
    if (n > ZRL_MAX_N) return BWTS_E_RANGE;
    if (in_bytes > n) return BWTS_E_FORMAT;
    if (ranges_overlap(d_in, in_bytes, d_out, n)) return BWTS_E_ARG;
    return run_sized(ctx, n, "zrl decode", [&] { return zrl_decode_impl(ctx, (const u8 *)d_in, in_bytes, (u8 *)d_out, n, SEG_SINGLE, nullptr); });
}

extern "C" int bwts_zrl_encode_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, void *d_out, uint64_t out_cap,
                                               uint64_t *out_lengths)
{
    if (!ctx || !d_in || !d_out || !out_lengths) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    if (ranges_overlap(d_in, n, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, n, "zrl encode", [&] { return zrl_encode_impl(ctx, (const u8 *)d_in, n, (u8 *)d_out, out_cap, seg_mode(ctx), out_lengths); });
}

extern "C" int bwts_zrl_decode_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *in_lengths, const uint64_t *lengths, uint64_t count,
                                               void *d_out)
{
    if (!ctx || !d_in || !d_out || !in_lengths) return BWTS_E_ARG;
    u64 n = 0, in_bytes = 0;
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    for (u64 s = 0; s < count; s++) {
        if (in_lengths[s] == 0) return BWTS_E_ARG;
        if (in_lengths[s] > lengths[s]) return BWTS_E_FORMAT;       // (so the sum cannot overflow)
        in_bytes += in_lengths[s];
    }
    if (ranges_overlap(d_in, in_bytes, d_out, n)) return BWTS_E_ARG;
    return run_sized(ctx, n, "zrl decode", [&] { return zrl_decode_impl(ctx, (const u8 *)d_in, in_bytes, (u8 *)d_out, n, seg_mode(ctx), in_lengths); });
}

extern "C" int bwts_zrl_encode(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !in || !out || !out_bytes || n == 0) return BWTS_E_ARG;
    if (n > ZRL_MAX_N) return BWTS_E_RANGE;
    if (out_cap == 0) return BWTS_E_SPACE;
    const u64 cap = out_cap < n ? out_cap : n;
    const HostTrip trip = {in, n, n, out, out_bytes};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *d_out, u64 *bytes) { return bwts_zrl_encode_device(ctx, d_in, n, d_out, cap, bytes); });
}

extern "C" int bwts_zrl_decode(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t n)
{
    if (!ctx || !in || !out || in_bytes == 0 || n == 0) return BWTS_E_ARG;
    if (n > ZRL_MAX_N) return BWTS_E_RANGE;
    if (in_bytes > n) return BWTS_E_FORMAT;
    u64 made = 0;
    const HostTrip trip = {in, in_bytes, n, out, &made};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *d_out, u64 *got) { *got = n; return bwts_zrl_decode_device(ctx, d_in, in_bytes, d_out, n); });
}

// ------------------------------------------------------------------------------------
// byte-plane split in front of the transform (include/bwts_planes.h): n bytes to n bytes at a width, the kernels in planes.hip
// ------------------------------------------------------------------------------------
static int planes_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t width, void *d_out, bool join)
{
    if (!ctx || !d_in || !d_out || n == 0 || !planes_width_ok(width)) return BWTS_E_ARG;
    if (n > PLANES_MAX_N) return BWTS_E_RANGE;
    if (ranges_overlap(d_in, n, d_out, n)) return BWTS_E_ARG;
    return run_sized(ctx, n, join ? "planes join" : "planes split", [&] { return planes_impl(ctx, (const u8 *)d_in, n, width, (u8 *)d_out, join, SEG_SINGLE); });
}

static int planes_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, uint32_t width, void *d_out, bool join)
{
    if (!ctx || !d_in || !d_out || !planes_width_ok(width)) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    if (ranges_overlap(d_in, n, d_out, n)) return BWTS_E_ARG;
    return run_sized(ctx, n, join ? "planes join" : "planes split", [&] { return planes_impl(ctx, (const u8 *)d_in, n, width, (u8 *)d_out, join, seg_mode(ctx)); });
}

static int planes_host(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint32_t width, uint8_t *out, bool join)
{
    if (!ctx || !in || !out || n == 0 || !planes_width_ok(width)) return BWTS_E_ARG;
    if (n > PLANES_MAX_N) return BWTS_E_RANGE;
    u64 made = 0;
    const HostTrip trip = {in, n, n, out, &made};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *d_out, u64 *got) { *got = n; return planes_device(ctx, d_in, n, width, d_out, join); });
}

extern "C" int bwts_planes_split_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t width, void *d_out)
{
    return planes_device(ctx, d_in, n, width, d_out, false);
}

extern "C" int bwts_planes_join_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t width, void *d_out)
{
    return planes_device(ctx, d_in, n, width, d_out, true);
}

extern "C" int bwts_planes_split_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, uint32_t width, void *d_out)
{
    return planes_segments_device(ctx, d_in, lengths, count, width, d_out, false);
}

extern "C" int bwts_planes_join_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, uint32_t width, void *d_out)
{
    return planes_segments_device(ctx, d_in, lengths, count, width, d_out, true);
}

extern "C" int bwts_planes_split(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint32_t width, uint8_t *out)
{
    return planes_host(ctx, in, n, width, out, false);
}

extern "C" int bwts_planes_join(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint32_t width, uint8_t *out)
{
    return planes_host(ctx, in, n, width, out, true);
}

// ------------------------------------------------------------------------------------
// delta filter in front of the byte-plane split (include/bwts_delta.h): n bytes to n bytes at a width, the kernels in delta.hip
// ------------------------------------------------------------------------------------
static int delta_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t width, void *d_out, bool decode)
{
    if (!ctx || !d_in || !d_out || n == 0 || !delta_width_ok(width)) return BWTS_E_ARG;
    if (n > DELTA_MAX_N) return BWTS_E_RANGE;
    if (ranges_overlap(d_in, n, d_out, n)) return BWTS_E_ARG;
    return run_sized(ctx, n, decode ? "delta decode" : "delta encode", [&] { return delta_impl(ctx, (const u8 *)d_in, n, width, (u8 *)d_out, decode); });
}

static int delta_segments_f_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters, uint64_t count,
                                   void *d_out, bool decode)
{
    if (!ctx || !d_in || !d_out || !widths || !filters) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    for (u64 s = 0; s < count; s++)
        if (!delta_width_ok(widths[s]) || !delta_filter_ok(filters[s])) return BWTS_E_ARG;
    if (ranges_overlap(d_in, n, d_out, n)) return BWTS_E_ARG;
    return run_sized(ctx, n, decode ? "delta decode" : "delta encode", [&] { return delta_f_impl(ctx, (const u8 *)d_in, n, widths, filters, (u8 *)d_out, decode); });
}

static int delta_host(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint32_t width, uint8_t *out, bool decode)
{
    if (!ctx || !in || !out || n == 0 || !delta_width_ok(width)) return BWTS_E_ARG;
    if (n > DELTA_MAX_N) return BWTS_E_RANGE;
    u64 made = 0;
    const HostTrip trip = {in, n, n, out, &made};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *d_out, u64 *got) { *got = n; return delta_device(ctx, d_in, n, width, d_out, decode); });
}

extern "C" int bwts_delta_encode_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t width, void *d_out)
{
    return delta_device(ctx, d_in, n, width, d_out, false);
}

extern "C" int bwts_delta_decode_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t width, void *d_out)
{
    return delta_device(ctx, d_in, n, width, d_out, true);
}

extern "C" int bwts_delta_encode_segments_f_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters,
                                                   uint64_t count, void *d_out)
{
    return delta_segments_f_device(ctx, d_in, lengths, widths, filters, count, d_out, false);
}

extern "C" int bwts_delta_decode_segments_f_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters,
                                                   uint64_t count, void *d_out)
{
    return delta_segments_f_device(ctx, d_in, lengths, widths, filters, count, d_out, true);
}

extern "C" int bwts_delta_encode(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint32_t width, uint8_t *out)
{
    return delta_host(ctx, in, n, width, out, false);
}

extern "C" int bwts_delta_decode(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint32_t width, uint8_t *out)
{
    return delta_host(ctx, in, n, width, out, true);
}

// ------------------------------------------------------------------------------------
// checksum and the packed frame (include/bwts_pack.h): the chain of the three stages as one call, the kernel in crc.hip, the drivers
// in pack.hip
// ------------------------------------------------------------------------------------
extern "C" int bwts_crc32_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t *crc)
{
    if (!ctx || !d_in || !crc || n == 0) return BWTS_E_ARG;
    if (n > CRC_MAX_N) return BWTS_E_RANGE;
    return run_sized(ctx, n, "crc32", [&] { return crc_impl(ctx, (const u8 *)d_in, n, SEG_SINGLE, crc); });
}

extern "C" int bwts_crc32_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, uint32_t *crcs)
{
    if (!ctx || !d_in || !crcs) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    return run_sized(ctx, n, "crc32", [&] { return crc_impl(ctx, (const u8 *)d_in, n, seg_mode(ctx), crcs); });
}

extern "C" uint64_t bwts_pack_bound_v(uint32_t version, uint64_t n, uint64_t block_bytes)
{
    const u64 B = pack_block_len(n, block_bytes);
    if (!B || !pack_version_asked_ok(version)) return 0;
    return pack_bound_bytes_of(version, n, B);
}

extern "C" uint64_t bwts_pack_planes_bound(uint32_t width, uint64_t n, uint64_t block_bytes)
{
    const u64 B = pack_block_len(n, block_bytes);
    return B && planes_width_ok(width) ? pack_bound_bytes_of(PACK_VERSION_3, n, B) : 0;
}

extern "C" uint64_t bwts_pack_bound(uint64_t n, uint64_t block_bytes)
{
    return bwts_pack_bound_v(PACK_VERSION, n, block_bytes);
}

extern "C" int bwts_unpack_size(const uint8_t *frame, uint64_t in_bytes, uint64_t *n, uint64_t *frame_bytes)
{
    if (!frame || !n || !frame_bytes) return BWTS_E_ARG;
    Frame F;
    BWTS_TRY(frame_head_check(frame, in_bytes, &F));
    BWTS_TRY(frame_dir_check(frame + PACK_HEADER_BYTES, F, in_bytes, false, frame_bytes));
    *n = F.n;
    return BWTS_OK;
}

// the device form of every version (width: 0 but for version 3)
static int pack_device_any(bwts_ctx *ctx, uint32_t version, uint32_t width, const void *d_in, uint64_t n, uint64_t block_bytes, void *d_out, uint64_t out_cap,
                           uint64_t *out_bytes)
{
    if (!ctx || !d_in || !d_out || !out_bytes || n == 0 || ((uintptr_t)d_out & 15)) return BWTS_E_ARG;
    if (n > PACK_MAX_N) return BWTS_E_RANGE;
    const u64 B = pack_block_len(n, block_bytes);
    if (B == 0 || ranges_overlap(d_in, n, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, n, "pack", [&] { return pack_device_impl(ctx, version, width, (const u8 *)d_in, n, B, (u8 *)d_out, out_cap, out_bytes); });
}

// the host form of every version
static int pack_host_any(bwts_ctx *ctx, uint32_t version, uint32_t width, const uint8_t *in, uint64_t n, uint64_t block_bytes, uint8_t *out, uint64_t out_cap,
                         uint64_t *out_bytes)
{
    if (!ctx || !in || !out || !out_bytes || n == 0) return BWTS_E_ARG;
    if (n > PACK_MAX_N) return BWTS_E_RANGE;
    const u64 B = pack_block_len(n, block_bytes);
    if (B == 0) return BWTS_E_ARG;
    const u64 bound = pack_bound_bytes_of(version, n, B);
    const u64 cap = out_cap < bound ? out_cap : bound;
    if (cap < pack_least_bytes_of(version, n, B)) return BWTS_E_SPACE;
    const HostTrip trip = {in, n, n > cap ? n : cap, out, out_bytes};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *d_out, u64 *bytes) { return pack_device_any(ctx, version, width, d_in, n, block_bytes, d_out, cap, bytes); });
}

extern "C" int bwts_pack_device_v(bwts_ctx *ctx, uint32_t version, const void *d_in, uint64_t n, uint64_t block_bytes, void *d_out, uint64_t out_cap,
                                  uint64_t *out_bytes)
{
    if (!pack_version_asked_ok(version)) return BWTS_E_ARG;
    return pack_device_any(ctx, version, 0, d_in, n, block_bytes, d_out, out_cap, out_bytes);
}

extern "C" int bwts_pack_planes_device(bwts_ctx *ctx, uint32_t width, const void *d_in, uint64_t n, uint64_t block_bytes, void *d_out, uint64_t out_cap,
                                       uint64_t *out_bytes)
{
    if (!planes_width_ok(width)) return BWTS_E_ARG;
    return pack_device_any(ctx, PACK_VERSION_3, width, d_in, n, block_bytes, d_out, out_cap, out_bytes);
}

extern "C" int bwts_pack_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint64_t block_bytes, void *d_out, uint64_t out_cap, uint64_t *out_bytes)
{
    return bwts_pack_device_v(ctx, PACK_VERSION, d_in, n, block_bytes, d_out, out_cap, out_bytes);
}

extern "C" int bwts_unpack_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, void *d_out, uint64_t out_cap, uint64_t *n)
{
    if (!ctx || !d_in || !d_out || !n || in_bytes == 0 || ((uintptr_t)d_in & 15)) return BWTS_E_ARG;
    if (ranges_overlap(d_in, in_bytes, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, 0, "unpack", [&] { return unpack_device_impl(ctx, (const u8 *)d_in, in_bytes, (u8 *)d_out, out_cap, n); });
}

extern "C" int bwts_pack_v(bwts_ctx *ctx, uint32_t version, const uint8_t *in, uint64_t n, uint64_t block_bytes, uint8_t *out, uint64_t out_cap,
                           uint64_t *out_bytes)
{
    if (!pack_version_asked_ok(version)) return BWTS_E_ARG;
    return pack_host_any(ctx, version, 0, in, n, block_bytes, out, out_cap, out_bytes);
}

extern "C" int bwts_pack_planes(bwts_ctx *ctx, uint32_t width, const uint8_t *in, uint64_t n, uint64_t block_bytes, uint8_t *out, uint64_t out_cap,
                                uint64_t *out_bytes)
{
    if (!planes_width_ok(width)) return BWTS_E_ARG;
    return pack_host_any(ctx, PACK_VERSION_3, width, in, n, block_bytes, out, out_cap, out_bytes);
}

extern "C" int bwts_pack(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint64_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes)
{
    return bwts_pack_v(ctx, PACK_VERSION, in, n, block_bytes, out, out_cap, out_bytes);
}

extern "C" int bwts_unpack(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n)
{
    if (!ctx || !in || !out || !n || in_bytes == 0) return BWTS_E_ARG;
    u64 v = 0, frame = 0;
    BWTS_TRY(bwts_unpack_size(in, in_bytes, &v, &frame));
    if (frame != in_bytes) return BWTS_E_FORMAT;
    if (v > out_cap) return BWTS_E_SPACE;
    const HostTrip trip = {in, in_bytes, in_bytes > v ? in_bytes : v, out, n};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *d_out, u64 *got) { return bwts_unpack_device(ctx, d_in, in_bytes, d_out, v, got); });
}

// ranges of a frame (include/bwts_pack.h, "Ranges"): the driver in pack.hip, the plan in members_plan.h
static_assert(sizeof(bwts_range) == sizeof(PackRange) && offsetof(bwts_range, bytes) == offsetof(PackRange, bytes), "bwts_range is pack_plan.h's PackRange");

extern "C" int bwts_unpack_ranges_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, const bwts_range *ranges, uint64_t count,
                                         void *d_out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !d_in || !d_out || !out_bytes || in_bytes == 0 || ((uintptr_t)d_in & 15)) return BWTS_E_ARG;
    if (ranges_overlap(d_in, in_bytes, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, 0, "unpack ranges", [&] {
        return unpack_ranges_device_impl(ctx, (const u8 *)d_in, in_bytes, false, (const PackRange *)ranges, count, (u8 *)d_out, out_cap, out_bytes);
    });
}

// The host form judges frame and ranges itself, in the device form's order, and sends header, directory and the covered blocks'
// streams alone, back to back: the device form finds them gathered.
// by_index: whole members of a member frame as the ranges (bwts_unpack_members); `ranges` is then not read.
static int unpack_ranges_host(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const PackRange *ranges, const uint64_t *indices, uint64_t count,
                              uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, bool by_index = false)
{
    Frame F;
    u64 sum = 0;
    PackRangesPlan P;
    std::vector<PackRange> whole;
    BWTS_TRY(frame_ranges_plan(in, in_bytes, ranges, by_index ? indices : nullptr, count, out_cap, &F, &sum, &whole, &ranges, &P));
    const u64 fixed = F.fixed;
    std::vector<u8> sent((size_t)(fixed + P.stream_bytes));
    memcpy(sent.data(), in, (size_t)fixed);
    for (const PackPiece &s : P.streams) memcpy(sent.data() + fixed + s.dst, in + s.src, (size_t)s.bytes);
    const HostTrip trip = {sent.data(), sent.size(), sent.size() > sum ? sent.size() : sum, out, out_bytes};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *d_out, u64 *got) {
        return run_sized(ctx, 0, "unpack ranges", [&] {
            return unpack_ranges_device_impl(ctx, d_in, in_bytes, true, ranges, count, d_out, sum, got, by_index ? indices : nullptr);
        });
    });
}

extern "C" int bwts_unpack_ranges(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const bwts_range *ranges, uint64_t count,
                                  uint8_t *out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !in || !out || !out_bytes || in_bytes == 0) return BWTS_E_ARG;
    return unpack_ranges_host(ctx, in, in_bytes, (const PackRange *)ranges, nullptr, count, out, out_cap, out_bytes);
}

// ------------------------------------------------------------------------------------
// the member frame (include/bwts_members.h): the drivers in pack.hip, the arithmetic in members_plan.h, the mixed-width kernels in
// planes.hip
// ------------------------------------------------------------------------------------
static int planes_segments_w_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, uint64_t count, void *d_out, bool join)
{
    if (!ctx || !d_in || !d_out || !widths) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    for (u64 s = 0; s < count; s++)
        if (!planes_width_w_ok(widths[s])) return BWTS_E_ARG;
    if (ranges_overlap(d_in, n, d_out, n)) return BWTS_E_ARG;
    return run_sized(ctx, n, join ? "planes join" : "planes split", [&] { return planes_w_impl(ctx, (const u8 *)d_in, n, widths, (u8 *)d_out, join); });
}

extern "C" int bwts_planes_split_segments_w_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, uint64_t count, void *d_out)
{
    return planes_segments_w_device(ctx, d_in, lengths, widths, count, d_out, false);
}

extern "C" int bwts_planes_join_segments_w_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, uint64_t count, void *d_out)
{
    return planes_segments_w_device(ctx, d_in, lengths, widths, count, d_out, true);
}

extern "C" uint64_t bwts_pack_members_bound(const uint64_t *lengths, uint64_t count)
{
    return members_bound_bytes(lengths, count);
}

extern "C" uint64_t bwts_pack_members_bound_m(const uint64_t *lengths, const uint32_t *widths, const uint32_t *methods, uint64_t count)
{
    return members_bound_bytes_m(lengths, widths, methods, count);
}

extern "C" int bwts_pack_members_m_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters,
                                          const uint32_t *methods, uint64_t count, void *d_out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !d_in || !d_out || !out_bytes || ((uintptr_t)d_out & 15)) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(members_args_check_m(lengths, widths, filters, methods, count, &n));
    if (ranges_overlap(d_in, n, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, n, "pack members", [&] {
        return pack_members_device_impl(ctx, (const u8 *)d_in, lengths, widths, filters, methods, count, n, (u8 *)d_out, out_cap, out_bytes);
    });
}

extern "C" int bwts_pack_members_m(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters,
                                   const uint32_t *methods, uint64_t count, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !in || !out || !out_bytes) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(members_args_check_m(lengths, widths, filters, methods, count, &n));
    // (without a method both are what they were: members_bound_bytes and members_least_bytes)
    const u64 bound = members_bound_bytes_m(lengths, widths, methods, count);
    const u64 cap = out_cap < bound ? out_cap : bound;
    if (cap < members_least_bytes_m(lengths, widths, methods, count)) return BWTS_E_SPACE;
    const HostTrip trip = {in, n, n > cap ? n : cap, out, out_bytes};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *d_out, u64 *bytes) {
        return bwts_pack_members_m_device(ctx, d_in, lengths, widths, filters, methods, count, d_out, cap, bytes);
    });
}

extern "C" int bwts_pack_members_f_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters, uint64_t count,
                                          void *d_out, uint64_t out_cap, uint64_t *out_bytes)
{
    return bwts_pack_members_m_device(ctx, d_in, lengths, widths, filters, nullptr, count, d_out, out_cap, out_bytes);
}

extern "C" int bwts_pack_members_f(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters, uint64_t count,
                                   uint8_t *out, uint64_t out_cap, uint64_t *out_bytes)
{
    return bwts_pack_members_m(ctx, in, lengths, widths, filters, nullptr, count, out, out_cap, out_bytes);
}

extern "C" int bwts_pack_members_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, uint64_t count, void *d_out,
                                        uint64_t out_cap, uint64_t *out_bytes)
{
    return bwts_pack_members_f_device(ctx, d_in, lengths, widths, nullptr, count, d_out, out_cap, out_bytes);
}

extern "C" int bwts_pack_members(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, const uint32_t *widths, uint64_t count, uint8_t *out,
                                 uint64_t out_cap, uint64_t *out_bytes)
{
    return bwts_pack_members_f(ctx, in, lengths, widths, nullptr, count, out, out_cap, out_bytes);
}

// the estimate and the pack that chooses (include/bwts_members.h, "The estimate", "AUTO"): the kernel in estimate.hip, the driver in pack.hip
static_assert(MEMBERS_AUTO == BWTS_FILTER_AUTO && MEMBERS_AUTO == BWTS_METHOD_AUTO, "members_plan.h names the header's AUTO");

extern "C" int bwts_members_estimate_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, uint64_t count,
                                            uint64_t *est_none, uint64_t *est_delta)
{
    if (!ctx || !d_in || !est_none || !est_delta) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(members_args_check(lengths, widths, count, &n));
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    std::vector<u32> ws((size_t)count, 1u);
    if (widths) ws.assign(widths, widths + count);
    return run_sized(ctx, n, "members estimate", [&] { return estimate_impl(ctx, (const u8 *)d_in, n, ws.data(), nullptr, est_none, est_delta); });
}

extern "C" int bwts_members_estimate(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, const uint32_t *widths, uint64_t count,
                                     uint64_t *est_none, uint64_t *est_delta)
{
    if (!ctx || !in || !est_none || !est_delta) return BWTS_E_ARG;
    u64 n = 0, made = 0;
    BWTS_TRY(members_args_check(lengths, widths, count, &n));
    u8 nothing = 0;
    const HostTrip trip = {in, n, n, &nothing, &made};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *, u64 *got) {
        *got = 0;
        return bwts_members_estimate_device(ctx, d_in, lengths, widths, count, est_none, est_delta);
    });
}

extern "C" uint64_t bwts_pack_members_bound_a(const uint64_t *lengths, const uint32_t *widths, const uint32_t *methods, uint64_t count)
{
    return members_bound_bytes_a(lengths, widths, methods, count);
}

extern "C" int bwts_pack_members_a_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters,
                                          const uint32_t *methods, uint64_t count, void *d_out, uint64_t out_cap, uint64_t *out_bytes,
                                          uint32_t *filters_out, uint32_t *methods_out)
{
    if (!ctx || !d_in || !d_out || !out_bytes || ((uintptr_t)d_out & 15)) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(members_args_check_a(lengths, widths, filters, methods, count, &n));
    if (ranges_overlap(d_in, n, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, n, "pack members", [&] {
        return pack_members_auto_device_impl(ctx, (const u8 *)d_in, lengths, widths, filters, methods, count, n, (u8 *)d_out, out_cap, out_bytes, filters_out,
                                             methods_out);
    });
}

extern "C" int bwts_pack_members_a(bwts_ctx *ctx, const uint8_t *in, const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters,
                                   const uint32_t *methods, uint64_t count, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes,
                                   uint32_t *filters_out, uint32_t *methods_out)
{
    if (!ctx || !in || !out || !out_bytes) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(members_args_check_a(lengths, widths, filters, methods, count, &n));
    // (the frame's size is known only when the choices are: the device form refuses what does not fit, before it writes)
    const u64 bound = members_bound_bytes_a(lengths, widths, methods, count);
    const u64 cap = out_cap < bound ? out_cap : bound;
    const HostTrip trip = {in, n, n > cap ? n : cap, out, out_bytes};
    return host_round_trip(ctx, trip, [&](const u8 *d_in, u8 *d_out, u64 *bytes) {
        return bwts_pack_members_a_device(ctx, d_in, lengths, widths, filters, methods, count, d_out, cap, bytes, filters_out, methods_out);
    });
}

extern "C" int bwts_frame_members_m(const uint8_t *frame, uint64_t in_bytes, uint64_t *lengths_out, uint32_t *widths_out, uint32_t *filters_out,
                                    uint32_t *methods_out, uint64_t cap, uint64_t *count)
{
    if (!frame || !count || in_bytes == 0) return BWTS_E_ARG;
    Frame F;
    u64 frame_bytes = 0;
    const int rc = frame_head_check(frame, in_bytes, &F);
    if (!F.members) return BWTS_E_FORMAT;       // (a "BWTZ" frame, whatever its own header check says, has no members)
    BWTS_TRY(rc);
    BWTS_TRY(frame_dir_check(frame + MEMBERS_HEADER_BYTES, F, in_bytes, true, &frame_bytes));
    if ((lengths_out || widths_out || filters_out || methods_out) && cap < F.count) return BWTS_E_SPACE;
    for (u64 k = 0; k < F.count; k++) {
        if (lengths_out) lengths_out[k] = F.len(k);
        if (widths_out) widths_out[k] = F.width[(size_t)k];
        if (filters_out) filters_out[k] = F.filter[(size_t)k];
        if (methods_out) methods_out[k] = F.direct(k) ? MEMBERS_METHOD_ORDER0 : MEMBERS_METHOD_CHAIN;
    }
    *count = F.count;
    return BWTS_OK;
}

extern "C" int bwts_frame_members_f(const uint8_t *frame, uint64_t in_bytes, uint64_t *lengths_out, uint32_t *widths_out, uint32_t *filters_out, uint64_t cap,
                                    uint64_t *count)
{
    return bwts_frame_members_m(frame, in_bytes, lengths_out, widths_out, filters_out, nullptr, cap, count);
}

extern "C" int bwts_frame_members(const uint8_t *frame, uint64_t in_bytes, uint64_t *lengths_out, uint32_t *widths_out, uint64_t cap, uint64_t *count)
{
    return bwts_frame_members_f(frame, in_bytes, lengths_out, widths_out, nullptr, cap, count);
}

extern "C" int bwts_unpack_members_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, const uint64_t *indices, uint64_t icount, void *d_out,
                                          uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !d_in || !d_out || !out_bytes || !indices || in_bytes == 0 || ((uintptr_t)d_in & 15)) return BWTS_E_ARG;
    if (ranges_overlap(d_in, in_bytes, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, 0, "unpack members", [&] {
        return unpack_ranges_device_impl(ctx, (const u8 *)d_in, in_bytes, false, nullptr, icount, (u8 *)d_out, out_cap, out_bytes, indices);
    });
}

extern "C" int bwts_unpack_members(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const uint64_t *indices, uint64_t icount, uint8_t *out,
                                   uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !in || !out || !out_bytes || !indices || in_bytes == 0) return BWTS_E_ARG;
    return unpack_ranges_host(ctx, in, in_bytes, nullptr, indices, icount, out, out_cap, out_bytes, true);
}

// ---- scattered members (include/bwts_members.h, "Pointers"): the copy kernel between scattered buffers as calls of its own, and
// ---- the member calls over tables of device pointers
// the scattered side of a call, ptrs[k] of lengths[k] >= 1 bytes, against its contiguous side [d_flat, d_flat + flat_bytes): no entry
// NULL, none that shares a byte with the contiguous side, and, where the scattered side is written, no two that share a byte
static int member_ptrs_check(const void *const *ptrs, const uint64_t *lengths, uint64_t count, const void *d_flat, u64 flat_bytes, bool written)
{
    if (!ptrs) return BWTS_E_ARG;
    for (u64 k = 0; k < count; k++)
        if (!ptrs[k]) return BWTS_E_ARG;
    std::vector<std::pair<u64, u64>> spans((size_t)count);
    for (u64 k = 0; k < count; k++) {
        if (ranges_overlap(d_flat, flat_bytes, ptrs[k], lengths[k])) return BWTS_E_ARG;
        spans[(size_t)k] = {(u64)(uintptr_t)ptrs[k], lengths[k]};
    }
    return !written || spans_disjoint(spans) ? BWTS_OK : BWTS_E_ARG;
}

// the members' pieces with the contiguous side at d_flat, members back to back
static std::vector<PackPiece> member_pieces(const void *const *ptrs, const uint64_t *lengths, uint64_t count, const void *d_flat, bool gather)
{
    std::vector<PackPiece> ps((size_t)count);
    u64 at = (u64)(uintptr_t)d_flat;
    for (u64 k = 0; k < count; k++) {
        const u64 m = (u64)(uintptr_t)ptrs[k];
        ps[(size_t)k] = gather ? PackPiece{m, at, lengths[k]} : PackPiece{at, m, lengths[k]};
        at += lengths[k];
    }
    return ps;
}

extern "C" int bwts_gather_device(bwts_ctx *ctx, const void *const *d_srcs, const uint64_t *lengths, uint64_t count, void *d_out)
{
    if (!ctx || !d_out) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(members_args_check(lengths, nullptr, count, &n));
    BWTS_TRY(member_ptrs_check(d_srcs, lengths, count, d_out, n, false));
    const std::vector<PackPiece> ps = member_pieces(d_srcs, lengths, count, d_out, true);
    return run_sized(ctx, n, "gather", [&] { return scatter_pieces_impl(ctx, ps.data(), count); });
}

extern "C" int bwts_scatter_device(bwts_ctx *ctx, const void *d_in, void *const *d_dsts, const uint64_t *lengths, uint64_t count)
{
    if (!ctx || !d_in) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(members_args_check(lengths, nullptr, count, &n));
    BWTS_TRY(member_ptrs_check(d_dsts, lengths, count, d_in, n, true));
    const std::vector<PackPiece> ps = member_pieces(d_dsts, lengths, count, d_in, false);
    return run_sized(ctx, n, "scatter", [&] { return scatter_pieces_impl(ctx, ps.data(), count); });
}

// A set that lies back to back already is the contiguous call's input as it is; any other is gathered into the block the context keeps
// for it, and packed from there.
extern "C" int bwts_pack_members_p_device(bwts_ctx *ctx, const void *const *d_members, const uint64_t *lengths, const uint32_t *widths,
                                          const uint32_t *filters, const uint32_t *methods, uint64_t count, void *d_out, uint64_t out_cap,
                                          uint64_t *out_bytes, uint32_t *filters_out, uint32_t *methods_out)
{
    if (!ctx || !d_out || !out_bytes || ((uintptr_t)d_out & 15)) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(members_args_check_a(lengths, widths, filters, methods, count, &n));
    BWTS_TRY(member_ptrs_check(d_members, lengths, count, d_out, out_cap, false));
    bool flat = true;
    for (u64 k = 0; k + 1 < count && flat; k++) flat = (const u8 *)d_members[k + 1] == (const u8 *)d_members[k] + lengths[k];
    return run_sized(ctx, n, "pack members", [&] {
        const u8 *d_in = (const u8 *)d_members[0];
        if (!flat) {
            BWTS_TRY(kept_grow(ctx, ctx->kept[KB_MEMBER_SET], n, 1 << 16, -1));
            u8 *set = (u8 *)ctx->kept[KB_MEMBER_SET].p;
            const std::vector<PackPiece> ps = member_pieces(d_members, lengths, count, set, true);
            BWTS_TRY(scatter_pieces_impl(ctx, ps.data(), count));
            d_in = set;
        }
        return pack_members_auto_device_impl(ctx, d_in, lengths, widths, filters, methods, count, n, (u8 *)d_out, out_cap, out_bytes, filters_out, methods_out);
    });
}

extern "C" int bwts_unpack_members_p_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, const uint64_t *indices, uint64_t icount,
                                            void *const *d_dsts, const uint64_t *dst_bytes)
{
    if (!ctx || !d_in || in_bytes == 0 || ((uintptr_t)d_in & 15)) return BWTS_E_ARG;
    const MemberDsts dsts = {d_dsts, dst_bytes};
    u64 made = 0;
    return run_sized(ctx, 0, "unpack members", [&] {
        return unpack_ranges_device_impl(ctx, (const u8 *)d_in, in_bytes, false, nullptr, icount, nullptr, ~0ull, &made, indices, &dsts);
    });
}

// copy_pieces_kernel alone (include/bwts_test.h; here for the call bracket): refuses, before anything is launched, what the driver's
// plan cannot make -- a piece that leaves either buffer, or two that share a destination byte
extern "C" int bwts_debug_copy_pieces(bwts_ctx *ctx, const void *d_src, uint64_t src_bytes, const uint64_t *pieces, uint64_t count, void *d_dst,
                                      uint64_t dst_bytes)
{
    if (!ctx || !d_src || !d_dst || !pieces || count == 0 || count > PACK_MAX_RANGES) return BWTS_E_ARG;
    std::vector<PackPiece> ps((size_t)count);
    std::vector<std::pair<u64, u64>> dsts((size_t)count);
    u64 total = 0;
    for (u64 i = 0; i < count; i++) {
        const PackPiece p = {pieces[3 * i], pieces[3 * i + 1], pieces[3 * i + 2]};
        if (p.bytes == 0 || p.bytes > src_bytes || p.src > src_bytes - p.bytes || p.bytes > dst_bytes || p.dst > dst_bytes - p.bytes) return BWTS_E_ARG;
        ps[(size_t)i] = p;
        dsts[(size_t)i] = {p.dst, p.bytes};
        total += p.bytes;
    }
    std::sort(dsts.begin(), dsts.end());
    for (u64 i = 1; i < count; i++)
        if (dsts[(size_t)i].first - dsts[(size_t)i - 1].first < dsts[(size_t)i - 1].second) return BWTS_E_ARG;
    return run_sized(ctx, total, "copy pieces", [&] { return copy_pieces_impl(ctx, (const u8 *)d_src, src_bytes, ps.data(), count, (u8 *)d_dst); });
}

extern "C" int bwts_host_alloc(bwts_ctx *ctx, uint64_t bytes, void **h_ptr)
{
    if (!ctx || !h_ptr) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return BWTS_E_NOMEM; }
    ctx->host_blocks.emplace_back((char *)p, (size_t)bytes);
    *h_ptr = p;
    return BWTS_OK;
}

extern "C" int bwts_host_free(bwts_ctx *ctx, void *h_ptr)
{
    if (!ctx) return BWTS_E_ARG;
    if (!h_ptr) return BWTS_OK;
    for (size_t i = 0; i < ctx->host_blocks.size(); i++) {
        if (ctx->host_blocks[i].first == (char *)h_ptr) {
            ctx->host_blocks.erase(ctx->host_blocks.begin() + (long)i);
            HIPC(hipSetDevice(ctx->device));
            HIPC(hipHostFree(h_ptr));
            return BWTS_OK;
        }
    }
    return BWTS_E_ARG;
}

extern "C" int bwts_set_timing(bwts_ctx *ctx, int level)
{
    if (!ctx || level < 0 || level > 2) return BWTS_E_ARG;
    ctx->timing = level;
    return BWTS_OK;
}

// ------------------------------------------------------------------------------------
// introspection
// ------------------------------------------------------------------------------------
extern "C" int bwts_last_timings(bwts_ctx *ctx, bwts_timings *t)
{
    if (!ctx || !t) return BWTS_E_ARG;
    *t = ctx->tm;
    for (int i = 0; i < BWTS_H_COUNT; i++) t->host_ms[i] = ctx->host_ms[i];
    return BWTS_OK;
}

extern "C" const char *bwts_kernel_class_name(int k)
{
    static const char *names[BWTS_K_COUNT] = {"histogram", "keybuild", "radix_hist", "radix_scan", "radix_scatter", "rerank",
                                              "lyndon", "emit", "lf_build", "walk", "listrank", "walk_emit", "other", "radix_scatter_main", "round"};
    return (k >= 0 && k < BWTS_K_COUNT) ? names[k] : "?";
}

extern "C" const char *bwts_host_cost_name(int h)
{
    static const char *names[BWTS_H_COUNT] = {"init", "module_load", "io_alloc", "staging_alloc", "arena_alloc"};
    return (h >= 0 && h < BWTS_H_COUNT) ? names[h] : "?";
}

extern "C" const char *bwts_strerror(int code)
{
    switch (code) {
    case BWTS_OK: return "ok";
    case BWTS_E_ARG: return "invalid argument (null pointer or empty input)";
    case BWTS_E_NODEVICE: return "no usable HIP device";
    case BWTS_E_NOMEM: return "out of device or pinned host memory";
    case BWTS_E_HIP: return "HIP runtime error";
    case BWTS_E_RANGE: return "input length beyond the engine's index range";
    case BWTS_E_INTERNAL: return "internal invariant violated";
    case BWTS_E_SINK: return "the caller's output sink reported an error";
    case BWTS_E_FORMAT: return "not a valid entropy-coded stream";
    case BWTS_E_SPACE: return "the result does not fit into the output buffer";
    case BWTS_E_CHECKSUM: return "checksum mismatch: the unpacked bytes are not the ones that were packed";
    default: return "unknown error";
    }
}

extern "C" int bwts_last_hip_error(bwts_ctx *ctx) { return ctx ? ctx->last_hip : 0; }
