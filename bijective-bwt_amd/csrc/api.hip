// api.hip -- the C-ABI of include/bwts.h: context, staging, timing, test hooks (the context's device memory: ctx_memory.hip).
#include "internal.h"
#include "../../include/bwts_test.h"
#include "../../include/bwts_mtf.h"
#include "../../include/bwts_ec.h"
#include "../../include/bwts_pack.h"
#include "ec_plan.h"
#include "pack_plan.h"

#include <algorithm>
#include <new>
#include <stdio.h>
#include <time.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif

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
    if (ctx->h_seg_off) (void)hipHostFree(ctx->h_seg_off);
    for (const auto &b : ctx->guard_freed) (void)hipFree(b.user - ctx->guard);
    ctx->guard_freed.clear();
    if (ctx->h_small) (void)hipHostFree(ctx->h_small);
    for (Stager &sg : ctx->stg) {
        if (sg.pool) { sg.pool->shutdown(); delete sg.pool; }
        for (int i = 0; i < STAGE_SLOTS; i++) {
            if (sg.pinned[i]) (void)hipHostFree(sg.pinned[i]);
            if (sg.slot_ev[i]) (void)hipEventDestroy(sg.slot_ev[i]);
            if (sg.slot_ev2[i]) (void)hipEventDestroy(sg.slot_ev2[i]);
        }
        if (sg.copy_stream) (void)hipStreamDestroy(sg.copy_stream);
        if (sg.own_stream && sg.stream) (void)hipStreamDestroy(sg.stream);
    }
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
typedef int (*device_impl_fn)(bwts_ctx *, const u8 *, u64, u8 *);
__global__ void pcie_copy_kernel(uint4 *__restrict__ dst, const uint4 *__restrict__ src, u64 vecs, u8 *__restrict__ dst_tail, const u8 *__restrict__ src_tail, u32 tail);

// The eight transforms that map n bytes to n bytes.  name: what a call is called in the guard report; in_label: its input in the
// allocation trace; arena_hint: what the host path reserves ahead of the call (0: the call's own reservation decides).  The transform
// and its inverse allocate ahead only up to 2^32 positions; the wide forms size their arenas themselves.
struct Transform {
    device_impl_fn fn;
    const char *name, *in_label;
    size_t (*arena_hint)(const bwts_ctx *ctx, u64 n);
};
#define NARROW_N 0x100000000ull
static const Transform kForward = {forward_device_impl, "forward", "forward: in", [](const bwts_ctx *, u64 n) { return n <= NARROW_N ? forward_arena_bytes(n) : 0; }};
static const Transform kInverse = {inverse_device_impl, "inverse", "inverse: in", [](const bwts_ctx *, u64 n) { return n <= NARROW_N ? inverse_arena_bytes(n) : 0; }};
static const Transform kForwardSegments = {forward_segments_impl, "forward", "forward: in", kForward.arena_hint};
static const Transform kInverseSegments = {inverse_segments_impl, "inverse", "inverse: in",
                                           [](const bwts_ctx *ctx, u64 n) { return n <= NARROW_N ? inverse_segments_arena_bytes(ctx, n) : 0; }};
static const Transform kMtfForward = {mtf_forward_impl, "mtf forward", "mtf: in", [](const bwts_ctx *ctx, u64 n) { return mtf_arena_bytes(ctx, n, false); }};
static const Transform kMtfInverse = {mtf_inverse_impl, "mtf inverse", "mtf: in", kMtfForward.arena_hint};
static const Transform kMtfForwardSegments = {mtf_forward_segments_impl, "mtf forward", "mtf: in", [](const bwts_ctx *ctx, u64 n) { return mtf_arena_bytes(ctx, n, true); }};
static const Transform kMtfInverseSegments = {mtf_inverse_segments_impl, "mtf inverse", "mtf: in", kMtfForwardSegments.arena_hint};

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

static int run_device(bwts_ctx *ctx, const Transform &t, const void *d_in, u64 n, void *d_out)
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
// host-buffer entry points (the path of the CLIs: mk_bwts_sa.c:41-60, unbwts.c:29-89)
// ------------------------------------------------------------------------------------
// Caller memory (typically an mmap of the input file, and a fresh malloc for the output) is not pinned, so it cannot be
// a DMA target.  It moves through a ring of STAGE_SLOTS pinned buffers: while the DMA engine works on one slot the copy
// workers fill (or drain) the next, and a slot is reused once ITS event has fired -- nothing waits for the whole stream.
// Memory from bwts_host_alloc() is pinned already and is transferred in one piece.
#define STAGE_CHUNK ((size_t)8 << 20)

void CopyPool::part(int i)
{
    if (touching) {                   // workers 1 .. parts-1 share the buffer; the caller takes no part
        // MADV_POPULATE_WRITE maps the pages writable WITHOUT changing what they hold (a store of zeros, the first form, clobbered
        // the caller's buffer although the call could still fail, and -- in a batch -- an input that the output aliases).  Where the
        // kernel refuses it (before Linux 5.14, or a mapping it cannot populate) nothing is pre-faulted: the copy out pays the faults.
        const int nw = parts - 1;
        const uintptr_t b = ((uintptr_t)dst + 4095) & ~(uintptr_t)4095, e = ((uintptr_t)dst + len) & ~(uintptr_t)4095;
        if (e <= b) return;
        const size_t pages = (e - b) >> 12, per = (pages + (size_t)nw - 1) / (size_t)nw;
        const size_t lo = per * (size_t)(i - 1) < pages ? per * (size_t)(i - 1) : pages;
        const size_t hi = lo + per < pages ? lo + per : pages;
        // (in pieces of 32 MiB: a worker that is told to stop gives up soon)
        for (size_t o = lo; o < hi && !touch_failed.load(std::memory_order_relaxed); o += 8192) {
            const size_t cnt = hi - o < 8192 ? hi - o : 8192;
            if (madvise((void *)(b + (o << 12)), cnt << 12, MADV_POPULATE_WRITE) != 0) touch_failed.store(true, std::memory_order_relaxed);
        }
        return;
    }
    // page-aligned cuts: two workers never fault on the same page of a fresh destination
    const size_t per = ((len / (size_t)parts) + 4095) & ~(size_t)4095;
    const size_t lo = per * (size_t)i < len ? per * (size_t)i : len;
    const size_t hi = i + 1 == parts ? len : (lo + per < len ? lo + per : len);
    if (hi > lo) memcpy(dst + lo, src + lo, hi - lo);
}

void CopyPool::start(int threads)
{
    parts = threads < 1 ? 1 : threads;
    for (int t = 1; t < parts; t++) {
        workers.emplace_back([this, t] {
            u64 seen = 0;
            for (;;) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv_work.wait(lk, [&] { return stop || generation != seen; });
                    if (stop) return;
                    seen = generation;
                }
                part(t);
                {
                    std::lock_guard<std::mutex> lk(mu);
                    if (--pending == 0) cv_done.notify_one();
                }
            }
        });
    }
}

void CopyPool::copy(void *d, const void *s_, size_t n)
{
    if (parts == 1 || n < ((size_t)1 << 20)) { memcpy(d, s_, n); return; }
    {
        std::lock_guard<std::mutex> lk(mu);
        dst = (char *)d; src = (const char *)s_; len = n;
        pending = parts - 1;
        generation++;
    }
    cv_work.notify_all();
    part(0);
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return pending == 0; });
}

void CopyPool::touch_async(void *d, size_t n)
{
    if (parts == 1 || n < ((size_t)4 << 20)) return;
    {
        std::lock_guard<std::mutex> lk(mu);
        dst = (char *)d; src = nullptr; len = n;
        touching = true;
        touch_failed.store(false, std::memory_order_relaxed);
        pending = parts - 1;
        generation++;
    }
    cv_work.notify_all();
}

void CopyPool::wait()
{
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return pending == 0; });
    touching = false;
}

void CopyPool::shutdown()
{
    {
        std::lock_guard<std::mutex> lk(mu);
        stop = true;
    }
    cv_work.notify_all();
    for (std::thread &t : workers) t.join();
    workers.clear();
}

// Copies between HBM and pinned host memory by a kernel instead of the DMA engines: the SDMA path moved 29-30 GB/s from the
// device to the host on the MI355X boxes used here, stores issued by compute units reach the PCIe link's rate.
__global__ __launch_bounds__(256) void pcie_copy_kernel(uint4 *__restrict__ dst, const uint4 *__restrict__ src, u64 vecs,
                                                        u8 *__restrict__ dst_tail, const u8 *__restrict__ src_tail, u32 tail)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < vecs; i += (u64)gridDim.x * 256) dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x < tail) dst_tail[threadIdx.x] = src_tail[threadIdx.x];
}

static int copy_mode(const bwts_ctx *ctx, const char *name)      // 0 = DMA engine (hipMemcpyAsync), 1 = copy kernel
{
    const char *e = bwts_knob(ctx, name);
    if (e && !strcmp(e, "dma")) return 0;
    if (e && !strcmp(e, "kernel")) return 1;
    return -1;
}

static int pcie_copy(bwts_ctx *ctx, hipStream_t stream, void *dst, const void *src, size_t len, bool use_kernel, hipMemcpyKind kind)
{
    if (!use_kernel || (((uintptr_t)dst | (uintptr_t)src) & 15)) {
        HIPC(hipMemcpyAsync(dst, src, len, kind, stream));
        return BWTS_OK;
    }
    const u64 vecs = len / 16;
    const u32 tail = (u32)(len % 16);
    u64 blocks = (vecs + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    pcie_copy_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>((uint4 *)dst, (const uint4 *)src, vecs, (u8 *)dst + vecs * 16,
                                                                            (const u8 *)src + vecs * 16, tail);
    HIPC(hipGetLastError());
    return BWTS_OK;
}

static int ensure_staging(bwts_ctx *ctx, Stager &sg)
{
    const double t0 = wall_ms();
    const bool first = !sg.pool;
    if (!sg.stream) {
        if (&sg == &ctx->stg[0]) sg.stream = ctx->stream;
        else { HIPC(hipStreamCreateWithFlags(&sg.stream, hipStreamNonBlocking)); sg.own_stream = true; }
    }
    for (int i = 0; i < STAGE_SLOTS; i++) {
        if (!sg.pinned[i]) {
            void *p = nullptr;
            if (hipHostMalloc(&p, STAGE_CHUNK, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return BWTS_E_NOMEM; }
            sg.pinned[i] = (char *)p;
            trace_alloc(ctx, "pinned +", "staging slot", p, STAGE_CHUNK);
        }
        if (!sg.slot_ev[i]) HIPC(hipEventCreateWithFlags(&sg.slot_ev[i], hipEventDisableTiming));
        if (!sg.slot_ev2[i]) HIPC(hipEventCreateWithFlags(&sg.slot_ev2[i], hipEventDisableTiming));
    }
    if (!sg.copy_stream) HIPC(hipStreamCreateWithFlags(&sg.copy_stream, hipStreamNonBlocking));
    if (!sg.pool) {
        int threads = 6;                                   // BWTS_COPY_THREADS: 1 = the calling thread alone
        if (const char *e = bwts_knob(ctx, "BWTS_COPY_THREADS")) { const int v = atoi(e); if (v >= 1 && v <= 64) threads = v; }
        const unsigned hw = std::thread::hardware_concurrency();
        if (hw && (unsigned)threads > hw) threads = (int)hw;
        sg.pool = new (std::nothrow) CopyPool();
        if (!sg.pool) return BWTS_E_NOMEM;
        sg.pool->start(threads);
    }
    if (first) ctx->host_ms[BWTS_H_STAGING_ALLOC] += wall_ms() - t0;
    return BWTS_OK;
}

static bool is_pinned_block(const bwts_ctx *ctx, const void *p, u64 n)
{
    for (const auto &b : ctx->host_blocks)
        if ((const char *)p >= b.first && (const char *)p + n <= b.first + b.second) return true;
    return false;
}

static int staged_h2d(bwts_ctx *ctx, Stager &sg, u8 *d_dst, const u8 *h_src, u64 n)
{
    const int mode = copy_mode(ctx, "BWTS_H2D");
    const bool by_kernel = mode == 1;
    BWTS_TRY(ensure_staging(ctx, sg));
    if (is_pinned_block(ctx, h_src, n)) {
        BWTS_TRY(pcie_copy(ctx, sg.stream, d_dst, h_src, n, by_kernel, hipMemcpyHostToDevice));
        HIPC(hipStreamSynchronize(sg.stream));
        return BWTS_OK;
    }
    u64 off = 0;
    for (u64 c = 0; off < n; c++) {
        const int slot = (int)(c % STAGE_SLOTS);
        const size_t len = n - off < STAGE_CHUNK ? (size_t)(n - off) : STAGE_CHUNK;
        if (c >= STAGE_SLOTS) HIPC(hipEventSynchronize(sg.slot_ev[slot]));       // the slot's previous DMA has read it
        sg.pool->copy(sg.pinned[slot], h_src + off, len);
        BWTS_TRY(pcie_copy(ctx, sg.stream, d_dst + off, sg.pinned[slot], len, by_kernel, hipMemcpyHostToDevice));
        HIPC(hipEventRecord(sg.slot_ev[slot], sg.stream));
        off += len;
    }
    HIPC(hipStreamSynchronize(sg.stream));
    return BWTS_OK;
}

// the result leaves in consecutive pieces: to h_dst (copy workers), or to the caller's sink straight from the staging slot
static int staged_d2h(bwts_ctx *ctx, Stager &sg, u8 *h_dst, const u8 *d_src, u64 n, bwts_sink_fn sink, void *user)
{
    const int mode = copy_mode(ctx, "BWTS_D2H");
    // default: the copy kernel for a single call (54 GB/s against the DMA engine's 29), the DMA engine inside a batch: there the
    // copy runs beside the next item's transform, whose kernels a copy kernel slows down by half (8 x 1 GiB: 18.0 GB/s with the
    // kernel, 24.4 GB/s with the engine -- the transform is the pipeline's slowest stage either way)
    const bool by_kernel = mode == 1 || (mode == -1 && &sg == &ctx->stg[0]);
    BWTS_TRY(ensure_staging(ctx, sg));
    if (!sink && is_pinned_block(ctx, h_dst, n)) {
        BWTS_TRY(pcie_copy(ctx, sg.stream, h_dst, d_src, n, by_kernel, hipMemcpyDeviceToHost));
        HIPC(hipStreamSynchronize(sg.stream));
        return BWTS_OK;
    }
    // a chunk's first part is moved by the copy kernel, the rest by the DMA engine on the second queue: the two paths
    // add up on the link (BWTS_D2H_SPLIT = percent moved by the kernel)
    const int kernel_pct = [ctx] { const char *e = bwts_knob(ctx, "BWTS_D2H_SPLIT"); int v = e ? atoi(e) : 100; return v < 0 ? 0 : v > 100 ? 100 : v; }();
    const u64 chunks = (n + STAGE_CHUNK - 1) / STAGE_CHUNK;
    auto issue = [&](u64 c) -> int {
        const u64 off = c * STAGE_CHUNK;
        const size_t len = n - off < STAGE_CHUNK ? (size_t)(n - off) : STAGE_CHUNK;
        const int slot = (int)(c % STAGE_SLOTS);
        size_t klen = by_kernel ? (len * (size_t)kernel_pct / 100) & ~(size_t)4095 : 0;
        if (by_kernel && kernel_pct == 100) klen = len;
        if (klen) BWTS_TRY(pcie_copy(ctx, sg.stream, sg.pinned[slot], d_src + off, klen, true, hipMemcpyDeviceToHost));
        HIPC(hipEventRecord(sg.slot_ev[slot], sg.stream));
        if (klen < len) HIPC(hipMemcpyAsync(sg.pinned[slot] + klen, d_src + off + klen, len - klen, hipMemcpyDeviceToHost, sg.copy_stream));
        HIPC(hipEventRecord(sg.slot_ev2[slot], sg.copy_stream));
        return BWTS_OK;
    };
    for (u64 c = 0; c < chunks && c < STAGE_SLOTS; c++) BWTS_TRY(issue(c));
    int rc = BWTS_OK;
    for (u64 c = 0; c < chunks; c++) {
        const u64 off = c * STAGE_CHUNK;
        const size_t len = n - off < STAGE_CHUNK ? (size_t)(n - off) : STAGE_CHUNK;
        const int slot = (int)(c % STAGE_SLOTS);
        if (hipEventSynchronize(sg.slot_ev[slot]) != hipSuccess || hipEventSynchronize(sg.slot_ev2[slot]) != hipSuccess) { rc = BWTS_E_HIP; break; }
        if (sink) { if (sink(user, (const uint8_t *)sg.pinned[slot], len) != 0) { rc = BWTS_E_SINK; break; } }
        else sg.pool->copy(h_dst + off, sg.pinned[slot], len);
        if (c + STAGE_SLOTS < chunks && (rc = issue(c + STAGE_SLOTS)) != BWTS_OK) break;
    }
    if (hipStreamSynchronize(sg.copy_stream) != hipSuccess && rc == BWTS_OK) rc = BWTS_E_HIP;
    if (hipStreamSynchronize(sg.stream) != hipSuccess && rc == BWTS_OK) rc = BWTS_E_HIP;
    return rc;
}


// device-side copies of the caller's input and output stay with the context (grown, never shrunk): d_io(ctx, 0), d_io(ctx, 1) inputs,
// d_io(ctx, 2), d_io(ctx, 3) outputs; the single calls use the first of each pair
static int ensure_io(bwts_ctx *ctx, u64 n, bool pairs)
{
    for (int i = 0; i < 4; i++)
        if (pairs || !(i & 1)) BWTS_TRY(kept_grow(ctx, ctx->kept[KB_IO + i], (size_t)n, 1 << 20, BWTS_H_IO_ALLOC));
    return BWTS_OK;
}

static int run_host(bwts_ctx *ctx, const Transform &t, const uint8_t *in, uint64_t n, uint8_t *out, bwts_sink_fn sink, void *user)
{
    if (!ctx || !in || (!out && !sink) || n == 0) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    BWTS_TRY(ensure_io(ctx, n, false));
    trace_alloc(ctx, "call    ", t.in_label, in, n);
    if (out) trace_alloc(ctx, "call    ", "out", out, n);
    Stager &sg = ctx->stg[0];
    // A context's first call allocates its arena, which can cost as long as the whole input copy where the driver clears what it
    // hands out: a helper thread does the hipMalloc -- and nothing else -- while this thread stages the input.  Rules (DESIGN.md
    // section 10: a GPU memory fault followed four arena re-reservations that an earlier form did wholly on the helper):
    //  * only a context that holds NO arena takes the helper (the one-shot CLI it was built for); a context that has to give up a
    //    smaller arena first does everything on this thread -- arena_release() drains the stream, then frees -- before staging starts;
    //  * the helper touches no context state: it allocates into a local, this thread installs the block after join().
    // BWTS_RESERVE_HELPER=1 (a test switch) sends EVERY growth through the helper, after the release on this thread.
    const size_t want = t.arena_hint(ctx, n);
    const KeptBlock &arena = ctx->kept[KB_ARENA];
    std::thread reserve;
    void *fresh = nullptr;
    double reserve_ms = 0;
    if (want > arena.cap) {
        const char *force = bwts_knob(ctx, "BWTS_RESERVE_HELPER");
        const bool helper = !ctx->guard && (force ? force[0] == '1' : (arena.p == nullptr && want >= ((size_t)256 << 20)));
        if (helper) {
            BWTS_TRY(arena_release(ctx));
            const size_t bytes = align_up(want, 1 << 20);
            const int device = ctx->device;
            reserve = std::thread([device, bytes, &fresh, &reserve_ms] {
                const double t0 = wall_ms();
                void *p = nullptr;
                if (hipSetDevice(device) == hipSuccess && hipMalloc(&p, bytes) == hipSuccess) fresh = p;
                else (void)hipGetLastError();
                reserve_ms = wall_ms() - t0;
            });
        }
    }
    double t0 = wall_ms();
    const int h2d_rc = staged_h2d(ctx, sg, d_io(ctx, 0), in, n);
    if (reserve.joinable()) {
        reserve.join();
        if (fresh) arena_install(ctx, fresh, align_up(want, 1 << 20), reserve_ms);     // (no block: the transform's own reservation reports it)
    }
    BWTS_TRY(h2d_rc);
    STAGE("host path: input on the device");
    const double h2d = wall_ms() - t0;
    // the caller's output buffer is usually fresh: its page faults are taken by the copy workers during the transform (contents
    // untouched: a call that fails leaves the buffer as it was, like the reference, which writes only after success: mk_bwts_sa.c:52-60)
    const bool touch = !sink && !is_pinned_block(ctx, out, n) && ensure_staging(ctx, sg) == BWTS_OK;
    if (touch) sg.pool->touch_async(out, n);
    const int rcd = run_device(ctx, t, d_io(ctx, 0), n, d_io(ctx, 2));
    if (touch) sg.pool->wait();
    BWTS_TRY(rcd);
    STAGE("host path: transform done");
    t0 = wall_ms();
    const int rc = staged_d2h(ctx, sg, out, d_io(ctx, 2), n, sink, user);
    ctx->tm.d2h_ms = wall_ms() - t0;
    ctx->tm.h2d_ms = h2d;
    return rc;
}

// ------------------------------------------------------------------------------------
// batches of independent inputs on one context (BASELINE config 5's data flow per GPU): a three-stage pipeline
// ------------------------------------------------------------------------------------
// While item k is transformed (the calling thread, the context's stream), item k+1 is staged to the device by one helper thread
// (stg[1], its own queue and copy workers) and item k-1 is drained to the caller's buffer by another (stg[2]).  Two device buffers
// per direction; an item's input buffer is free again when its transform is done, its output buffer when it has been drained.
// Every item goes through exactly the code of the single calls, so the bytes are the same.
struct BatchState {
    std::mutex mu;
    std::condition_variable cv;
    int staged = -1, transformed = -1, drained = -1;     // highest item index that has passed each stage
    int error = BWTS_OK;
};

static int run_batch(bwts_ctx *ctx, const Transform &t, int count, const uint8_t *const *ins, const uint64_t *ns, uint8_t *const *outs)
{
    if (!ctx || count < 0 || (count && (!ins || !ns || !outs))) return BWTS_E_ARG;
    u64 nmax = 0;
    for (int k = 0; k < count; k++) {
        if (!ins[k] || !outs[k] || ns[k] == 0) return BWTS_E_ARG;
        if (ns[k] > nmax) nmax = ns[k];
    }
    if (count == 0) return BWTS_OK;
    // An item's output may lie on its OWN input (in place, like `mk_bwts f f`: the input is on the device before a byte comes back) or on
    // an earlier item's.  It may not touch a LATER item's input: that item may not have been staged yet when this one is drained (single
    // calls in sequence would hand the later call the overwritten bytes; here it would be a race) -- refused.
    for (int k = 0; k < count; k++)
        for (int j = k + 1; j < count; j++)
            if (outs[k] < ins[j] + ns[j] && ins[j] < outs[k] + ns[k]) return BWTS_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    BWTS_TRY(ensure_io(ctx, nmax, true));
    BWTS_TRY(ensure_staging(ctx, ctx->stg[1]));
    BWTS_TRY(ensure_staging(ctx, ctx->stg[2]));
    BWTS_TRY(arena_reserve(ctx, std::max(t.arena_hint(ctx, nmax), ctx->kept[KB_ARENA].cap)));
    BatchState st;
    double busy[3] = {0, 0, 0};          // time the three stages spent working (BWTS_BATCH_TRACE=1 prints them)
    auto fail = [&st](int rc) { std::lock_guard<std::mutex> lk(st.mu); if (st.error == BWTS_OK) st.error = rc; st.cv.notify_all(); };
    const double t_begin = wall_ms();
    std::thread feeder([&] {
        if (hipSetDevice(ctx->device) != hipSuccess) { fail(BWTS_E_HIP); return; }
        for (int k = 0; k < count; k++) {
            {   // input buffer k % 2 is free once item k - 2 has been transformed
                std::unique_lock<std::mutex> lk(st.mu);
                st.cv.wait(lk, [&] { return st.error != BWTS_OK || st.transformed >= k - 2; });
                if (st.error != BWTS_OK) return;
            }
            const double t0 = wall_ms();
            const int rc = staged_h2d(ctx, ctx->stg[1], d_io(ctx, k & 1), ins[k], ns[k]);
            busy[0] += wall_ms() - t0;
            if (rc != BWTS_OK) { fail(rc); return; }
            { std::lock_guard<std::mutex> lk(st.mu); st.staged = k; }
            st.cv.notify_all();
        }
    });
    std::thread drainer([&] {
        if (hipSetDevice(ctx->device) != hipSuccess) { fail(BWTS_E_HIP); return; }
        for (int k = 0; k < count; k++) {
            // the caller's buffer is usually fresh: fault its pages in while the item is still being transformed (the pages' contents
            // stay as they are -- CopyPool::part -- so an output that lies on an input not yet staged does it no harm)
            const bool touch = !is_pinned_block(ctx, outs[k], ns[k]);
            if (touch) ctx->stg[2].pool->touch_async(outs[k], ns[k]);
            {
                std::unique_lock<std::mutex> lk(st.mu);
                st.cv.wait(lk, [&] { return st.error != BWTS_OK || st.transformed >= k; });
                if (touch) { lk.unlock(); ctx->stg[2].pool->wait(); lk.lock(); }
                if (st.error != BWTS_OK) return;
            }
            const double t0 = wall_ms();
            const int rc = staged_d2h(ctx, ctx->stg[2], outs[k], d_io(ctx, 2 + (k & 1)), ns[k], nullptr, nullptr);
            busy[2] += wall_ms() - t0;
            if (rc != BWTS_OK) { fail(rc); return; }
            { std::lock_guard<std::mutex> lk(st.mu); st.drained = k; }
            st.cv.notify_all();
        }
    });
    for (int k = 0; k < count; k++) {
        {   // input k on the device, output buffer k % 2 drained of item k - 2
            std::unique_lock<std::mutex> lk(st.mu);
            st.cv.wait(lk, [&] { return st.error != BWTS_OK || (st.staged >= k && st.drained >= k - 2); });
            if (st.error != BWTS_OK) break;
        }
        const double t0 = wall_ms();
        const int rc = run_device(ctx, t, d_io(ctx, k & 1), ns[k], d_io(ctx, 2 + (k & 1)));
        busy[1] += wall_ms() - t0;
        if (rc != BWTS_OK) { fail(rc); break; }
        { std::lock_guard<std::mutex> lk(st.mu); st.transformed = k; }
        st.cv.notify_all();
    }
    feeder.join();
    drainer.join();
    if (const char *e = bwts_knob(ctx, "BWTS_BATCH_TRACE"))
        if (e[0] == '1') fprintf(stderr, "[batch] %d items, wall %.1f ms; busy: copy in %.1f, transform %.1f, copy out %.1f ms\n", count, wall_ms() - t_begin, busy[0], busy[1], busy[2]);
    ctx->tm.h2d_ms = 0;
    ctx->tm.d2h_ms = wall_ms() - t_begin;        // (batch: wall time of the whole pipeline; total_ms is the last item's transform)
    return st.error;
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

// ------------------------------------------------------------------------------------
// independent segments in one device pass: the segment table goes to the context, the transform runs through the same host / device
// plumbing as a single input (staging, pre-faulting, a failed call leaves `out` as it was)
// ------------------------------------------------------------------------------------
int seg_table_set(bwts_ctx *ctx, const uint64_t *lengths, uint64_t count, u64 *total)
{
    if (!ctx || !lengths || count == 0) return BWTS_E_ARG;
    u64 sum = 0;
    for (u64 s = 0; s < count; s++) {
        if (lengths[s] == 0 || lengths[s] > ~0ull - sum) return BWTS_E_ARG;
        sum += lengths[s];
    }
    if (sum > 0x100000000ull) return BWTS_E_RANGE;
    HIPC(hipSetDevice(ctx->device));
    ctx->seg_off.resize(count + 1);
    ctx->seg_off[0] = 0;
    for (u64 s = 0; s < count; s++) ctx->seg_off[s + 1] = ctx->seg_off[s] + lengths[s];
    const size_t bytes = (count + 1) * sizeof(u64);
    const size_t room = 3 * bytes;       // the table, and behind it a second one of up to 2 count + 1 words (seg_upload_extra)
    BWTS_TRY(kept_grow(ctx, ctx->kept[KB_SEG_TABLE], room, 1 << 16, -1));
    // the table travels from a pinned block on the context's stream, ahead of the transform (the stream is idle between calls: the wait
    // only makes sure no earlier copy still reads the block)
    if (room > ctx->h_seg_cap) {
        HIPC(hipStreamSynchronize(ctx->stream));
        if (ctx->h_seg_off) { HIPC(hipHostFree(ctx->h_seg_off)); ctx->h_seg_off = nullptr; ctx->h_seg_cap = 0; }
        void *p = nullptr;
        const size_t cap = align_up(room, 1 << 16);
        if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return BWTS_E_NOMEM; }
        ctx->h_seg_off = (u64 *)p;
        ctx->h_seg_cap = cap;
    } else {
        HIPC(hipStreamSynchronize(ctx->stream));
    }
    memcpy(ctx->h_seg_off, ctx->seg_off.data(), bytes);
    HIPC(hipMemcpyAsync(d_seg_off(ctx), ctx->h_seg_off, bytes, hipMemcpyHostToDevice, ctx->stream));
    *total = sum;
    return BWTS_OK;
}

int seg_upload_extra(bwts_ctx *ctx, const u64 *words, u64 count, u64 **d_words)
{
    const u64 at = (u64)ctx->seg_off.size();
    if ((at + count) * sizeof(u64) > ctx->kept[KB_SEG_TABLE].cap || (at + count) * sizeof(u64) > ctx->h_seg_cap) return BWTS_E_INTERNAL;
    memcpy(ctx->h_seg_off + at, words, count * sizeof(u64));
    HIPC(hipMemcpyAsync(d_seg_off(ctx) + at, ctx->h_seg_off + at, count * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    *d_words = d_seg_off(ctx) + at;
    return BWTS_OK;
}

int seg_scratch_reserve(bwts_ctx *ctx, size_t bytes, u8 **out)
{
    BWTS_TRY(kept_grow(ctx, ctx->kept[KB_SEG_SCRATCH], bytes, 1 << 20, -1));
    *out = (u8 *)ctx->kept[KB_SEG_SCRATCH].p;
    return BWTS_OK;
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
    const char *a = (const char *)d_in, *b = (const char *)d_out;
    if (a < b + n && b < a + n) return BWTS_E_ARG;
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
static bool ranges_overlap(const void *a, u64 na, const void *b, u64 nb)
{
    // by subtraction: a length as large as 2^64 - 1 must not wrap the comparison
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x <= y ? y - x < na : x - y < nb;
}

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
        if (sum > 0x100000000ull) return BWTS_E_RANGE;
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
    return run_sized(ctx, n, "ec encode", [&] { return ec_encode_impl(ctx, (const u8 *)d_in, n, (u8 *)d_out, out_cap, out_bytes, nullptr); });
}

extern "C" int bwts_ec_decode_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, void *d_out, uint64_t out_cap, uint64_t *n)
{
    if (!ctx || !d_in || !d_out || !n || in_bytes == 0 || ((uintptr_t)d_in & 15)) return BWTS_E_ARG;
    if (in_bytes > ec_bound_bytes(EC_MAX_N)) return BWTS_E_RANGE;
    if (ranges_overlap(d_in, in_bytes, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, 0, "ec decode", [&] { return ec_decode_impl(ctx, (const u8 *)d_in, in_bytes, (u8 *)d_out, out_cap, n, nullptr); });
}

extern "C" int bwts_ec_encode_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, void *d_out, uint64_t out_cap,
                                              uint64_t *stream_bytes)
{
    if (!ctx || !d_in || !d_out || !stream_bytes || ((uintptr_t)d_out & 15)) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    if (ranges_overlap(d_in, n, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, n, "ec encode", [&] { return ec_encode_impl(ctx, (const u8 *)d_in, n, (u8 *)d_out, out_cap, nullptr, stream_bytes); });
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
    return run_sized(ctx, n, "ec decode", [&] { return ec_decode_impl(ctx, (const u8 *)d_in, n, (u8 *)d_out, n, nullptr, stream_bytes); });
}

// Host buffers, staged simply: the input goes to the device, the device form runs, what it made comes back.  Nothing is written to out
// before the device form has succeeded.
extern "C" int bwts_ec_encode(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !in || !out || !out_bytes || n == 0) return BWTS_E_ARG;
    if (n > EC_MAX_N) return BWTS_E_RANGE;
    const u64 cap = out_cap < ec_bound_bytes(n) ? out_cap : ec_bound_bytes(n);
    if (cap < ec_least_bytes(n)) return BWTS_E_SPACE;
    HIPC(hipSetDevice(ctx->device));
    BWTS_TRY(ensure_io(ctx, n > cap ? n : cap, false));
    Stager &sg = ctx->stg[0];
    double t0 = wall_ms();
    BWTS_TRY(staged_h2d(ctx, sg, d_io(ctx, 0), in, n));
    const double h2d = wall_ms() - t0;
    u64 bytes = 0;
    BWTS_TRY(bwts_ec_encode_device(ctx, d_io(ctx, 0), n, d_io(ctx, 2), cap, &bytes));
    t0 = wall_ms();
    BWTS_TRY(staged_d2h(ctx, sg, out, d_io(ctx, 2), bytes, nullptr, nullptr));
    ctx->tm.d2h_ms = wall_ms() - t0;
    ctx->tm.h2d_ms = h2d;
    *out_bytes = bytes;
    return BWTS_OK;
}

extern "C" int bwts_ec_decode(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n)
{
    if (!ctx || !in || !out || !n || in_bytes == 0) return BWTS_E_ARG;
    if (in_bytes > ec_bound_bytes(EC_MAX_N)) return BWTS_E_RANGE;
    u64 v = 0;
    BWTS_TRY(bwts_ec_decoded_size(in, in_bytes, &v));
    if (v > out_cap) return BWTS_E_SPACE;
    HIPC(hipSetDevice(ctx->device));
    BWTS_TRY(ensure_io(ctx, in_bytes > v ? in_bytes : v, false));
    Stager &sg = ctx->stg[0];
    double t0 = wall_ms();
    BWTS_TRY(staged_h2d(ctx, sg, d_io(ctx, 0), in, in_bytes));
    const double h2d = wall_ms() - t0;
    u64 got = 0;
    BWTS_TRY(bwts_ec_decode_device(ctx, d_io(ctx, 0), in_bytes, d_io(ctx, 2), v, &got));
    t0 = wall_ms();
    BWTS_TRY(staged_d2h(ctx, sg, out, d_io(ctx, 2), got, nullptr, nullptr));
    ctx->tm.d2h_ms = wall_ms() - t0;
    ctx->tm.h2d_ms = h2d;
    *n = got;
    return BWTS_OK;
}

// ------------------------------------------------------------------------------------
// checksum and the packed frame (include/bwts_pack.h): the chain of the three stages as one call, the kernel in crc.hip, the drivers
// in pack.hip
// ------------------------------------------------------------------------------------
extern "C" int bwts_crc32_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint32_t *crc)
{
    if (!ctx || !d_in || !crc || n == 0) return BWTS_E_ARG;
    if (n > CRC_MAX_N) return BWTS_E_RANGE;
    return run_sized(ctx, n, "crc32", [&] { return crc_impl(ctx, (const u8 *)d_in, n, false, crc); });
}

extern "C" int bwts_crc32_segments_device(bwts_ctx *ctx, const void *d_in, const uint64_t *lengths, uint64_t count, uint32_t *crcs)
{
    if (!ctx || !d_in || !crcs) return BWTS_E_ARG;
    u64 n = 0;
    BWTS_TRY(seg_table_set(ctx, lengths, count, &n));
    return run_sized(ctx, n, "crc32", [&] { return crc_impl(ctx, (const u8 *)d_in, n, true, crcs); });
}

extern "C" uint64_t bwts_pack_bound(uint64_t n, uint64_t block_bytes)
{
    const u64 B = pack_block_len(n, block_bytes);
    return B ? pack_bound_bytes(n, B) : 0;
}

extern "C" int bwts_unpack_size(const uint8_t *frame, uint64_t in_bytes, uint64_t *n, uint64_t *frame_bytes)
{
    if (!frame || !n || !frame_bytes) return BWTS_E_ARG;
    PackHeader H;
    BWTS_TRY(pack_header_check(frame, in_bytes, &H));
    BWTS_TRY(pack_directory_check(frame + PACK_HEADER_BYTES, H, in_bytes, false, frame_bytes));
    *n = H.n;
    return BWTS_OK;
}

extern "C" int bwts_pack_device(bwts_ctx *ctx, const void *d_in, uint64_t n, uint64_t block_bytes, void *d_out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !d_in || !d_out || !out_bytes || n == 0 || ((uintptr_t)d_out & 15)) return BWTS_E_ARG;
    if (n > PACK_MAX_N) return BWTS_E_RANGE;
    const u64 B = pack_block_len(n, block_bytes);
    if (B == 0 || ranges_overlap(d_in, n, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, n, "pack", [&] { return pack_device_impl(ctx, (const u8 *)d_in, n, B, (u8 *)d_out, out_cap, out_bytes); });
}

extern "C" int bwts_unpack_device(bwts_ctx *ctx, const void *d_in, uint64_t in_bytes, void *d_out, uint64_t out_cap, uint64_t *n)
{
    if (!ctx || !d_in || !d_out || !n || in_bytes == 0 || ((uintptr_t)d_in & 15)) return BWTS_E_ARG;
    if (ranges_overlap(d_in, in_bytes, d_out, out_cap)) return BWTS_E_ARG;
    return run_sized(ctx, 0, "unpack", [&] { return unpack_device_impl(ctx, (const u8 *)d_in, in_bytes, (u8 *)d_out, out_cap, n); });
}

// Host buffers, staged like the coder's: in goes to the device, the device form runs, what it made comes back.  Nothing is written
// to out before the device form has succeeded.
extern "C" int bwts_pack(bwts_ctx *ctx, const uint8_t *in, uint64_t n, uint64_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!ctx || !in || !out || !out_bytes || n == 0) return BWTS_E_ARG;
    if (n > PACK_MAX_N) return BWTS_E_RANGE;
    const u64 B = pack_block_len(n, block_bytes);
    if (B == 0) return BWTS_E_ARG;
    const u64 cap = out_cap < pack_bound_bytes(n, B) ? out_cap : pack_bound_bytes(n, B);
    if (cap < pack_least_bytes(n, B)) return BWTS_E_SPACE;
    HIPC(hipSetDevice(ctx->device));
    BWTS_TRY(ensure_io(ctx, n > cap ? n : cap, false));
    Stager &sg = ctx->stg[0];
    double t0 = wall_ms();
    BWTS_TRY(staged_h2d(ctx, sg, d_io(ctx, 0), in, n));
    const double h2d = wall_ms() - t0;
    u64 bytes = 0;
    BWTS_TRY(bwts_pack_device(ctx, d_io(ctx, 0), n, block_bytes, d_io(ctx, 2), cap, &bytes));
    t0 = wall_ms();
    BWTS_TRY(staged_d2h(ctx, sg, out, d_io(ctx, 2), bytes, nullptr, nullptr));
    ctx->tm.d2h_ms = wall_ms() - t0;
    ctx->tm.h2d_ms = h2d;
    *out_bytes = bytes;
    return BWTS_OK;
}

extern "C" int bwts_unpack(bwts_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n)
{
    if (!ctx || !in || !out || !n || in_bytes == 0) return BWTS_E_ARG;
    u64 v = 0, frame = 0;
    BWTS_TRY(bwts_unpack_size(in, in_bytes, &v, &frame));
    if (frame != in_bytes) return BWTS_E_FORMAT;
    if (v > out_cap) return BWTS_E_SPACE;
    HIPC(hipSetDevice(ctx->device));
    BWTS_TRY(ensure_io(ctx, in_bytes > v ? in_bytes : v, false));
    Stager &sg = ctx->stg[0];
    double t0 = wall_ms();
    BWTS_TRY(staged_h2d(ctx, sg, d_io(ctx, 0), in, in_bytes));
    const double h2d = wall_ms() - t0;
    u64 got = 0;
    BWTS_TRY(bwts_unpack_device(ctx, d_io(ctx, 0), in_bytes, d_io(ctx, 2), v, &got));
    t0 = wall_ms();
    BWTS_TRY(staged_d2h(ctx, sg, out, d_io(ctx, 2), got, nullptr, nullptr));
    ctx->tm.d2h_ms = wall_ms() - t0;
    ctx->tm.h2d_ms = h2d;
    *n = got;
    return BWTS_OK;
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

// ------------------------------------------------------------------------------------
// harness utilities
// ------------------------------------------------------------------------------------
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

// ------------------------------------------------------------------------------------
// unit-test hooks
// ------------------------------------------------------------------------------------
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

static int upload_text(bwts_ctx *ctx, const uint8_t *in, uint64_t n, u8 **d_T)
{
    void *p = nullptr;
    if (hipMalloc(&p, n) != hipSuccess) { (void)hipGetLastError(); return BWTS_E_NOMEM; }
    if (hipMemcpyAsync(p, in, n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) { (void)hipFree(p); return BWTS_E_HIP; }
    *d_T = (u8 *)p;
    return BWTS_OK;
}

// the chunk tables' arithmetic for a tied list of a0 elements of which a_chunks are left at a compaction: no context, no device
extern "C" int bwts_debug_chunk_plan(uint64_t a0, uint64_t a_chunks, uint64_t out[4])
{
    const ChunkRecut re = chunk_recut_plan(a0, a_chunks);
    out[0] = chunk_nominal_size(a0); out[1] = chunk_table_capacity(a0); out[2] = re.S; out[3] = re.nc;
    return re.allowed ? 1 : 0;
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
    if (n == 0 || n > 0x100000000ull || g > 20 || mark < 0 || mark > 3) return -1;
    if (g < 0) g = inverse_splitter_log2(n);
    out[0] = inverse_attempt_bytes(n, g, mark); out[1] = inverse_arena_bytes(n);
    return g;
}

// the narrow forward's arena, likewise: the bytes its declared layout takes
extern "C" int bwts_debug_forward_arena(uint64_t n, uint64_t out[1])
{
    if (n == 0 || n > 0x100000000ull || !out) return -1;
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
