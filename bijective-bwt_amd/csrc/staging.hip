// staging.hip -- everything between caller memory and HBM: the copy kernel, the ring of pinned slots, the one host round trip that
// every host-buffer entry point takes (the path of the CLIs: mk_bwts_sa.c:41-60, unbwts.c:29-89), the three-thread batch pipeline.
#include "internal.h"
#include "copy_pool.h"

#include <algorithm>
#include <new>
#include <stdio.h>
#include <stdlib.h>

// Caller memory (typically an mmap of the input file, and a fresh malloc for the output) is not pinned, so it cannot be
// a DMA target.  It moves through a ring of STAGE_SLOTS pinned buffers: while the DMA engine works on one slot the copy
// workers fill (or drain) the next, and a slot is reused once ITS event has fired -- nothing waits for the whole stream.
// Memory from bwts_host_alloc() is pinned already and is transferred in one piece.
#define STAGE_CHUNK ((size_t)8 << 20)

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

int host_round_trip(bwts_ctx *ctx, const HostTrip &trip, const std::function<int(const u8 *, u8 *, u64 *)> &device_form)
{
    const u64 n = trip.in_bytes;
    HIPC(hipSetDevice(ctx->device));
    BWTS_TRY(ensure_io(ctx, trip.io_bytes, false));
    if (trip.ahead) trace_alloc(ctx, "call    ", trip.ahead->in_label, trip.in, n);
    if (trip.ahead && trip.out) trace_alloc(ctx, "call    ", "out", trip.out, n);
    Stager &sg = ctx->stg[0];
    // A context's first call allocates its arena, which can cost as long as the whole input copy where the driver clears what it
    // hands out: a helper thread does the hipMalloc -- and nothing else -- while this thread stages the input.  Rules (DESIGN.md
    // section 10: a GPU memory fault followed four arena re-reservations that an earlier form did wholly on the helper):
    //  * only a context that holds NO arena takes the helper (the one-shot CLI it was built for); a context that has to give up a
    //    smaller arena first does everything on this thread -- arena_release() drains the stream, then frees -- before staging starts;
    //  * the helper touches no context state: it allocates into a local, this thread installs the block after join().
    // BWTS_RESERVE_HELPER=1 (a test switch) sends EVERY growth through the helper, after the release on this thread.
    const size_t want = trip.ahead ? trip.ahead->arena_hint(ctx, n) : 0;
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
    const int h2d_rc = staged_h2d(ctx, sg, d_io(ctx, 0), trip.in, n);
    if (reserve.joinable()) {
        reserve.join();
        if (fresh) arena_install(ctx, fresh, align_up(want, 1 << 20), reserve_ms);     // (no block: the transform's own reservation reports it)
    }
    BWTS_TRY(h2d_rc);
    STAGE("host path: input on the device");
    const double h2d = wall_ms() - t0;
    // the caller's output buffer is usually fresh: its page faults are taken by the copy workers during the transform (contents
    // untouched: a call that fails leaves the buffer as it was, like the reference, which writes only after success: mk_bwts_sa.c:52-60)
    const bool touch = trip.ahead && !trip.sink && !is_pinned_block(ctx, trip.out, n) && ensure_staging(ctx, sg) == BWTS_OK;
    if (touch) sg.pool->touch_async(trip.out, n);
    u64 made = 0;
    const int rcd = device_form(d_io(ctx, 0), d_io(ctx, 2), &made);
    if (touch) sg.pool->wait();
    BWTS_TRY(rcd);
    STAGE("host path: transform done");
    t0 = wall_ms();
    const int rc = staged_d2h(ctx, sg, trip.out, d_io(ctx, 2), made, trip.sink, trip.user);
    ctx->tm.d2h_ms = wall_ms() - t0;
    ctx->tm.h2d_ms = h2d;
    if (rc == BWTS_OK) *trip.out_bytes = made;
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

int run_batch(bwts_ctx *ctx, const Transform &t, int count, const uint8_t *const *ins, const uint64_t *ns, uint8_t *const *outs)
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
            if (ranges_overlap(outs[k], ns[k], ins[j], ns[j])) return BWTS_E_ARG;
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
            // stay as they are -- part() in copy_pool.h -- so an output that lies on an input not yet staged does it no harm)
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

void staging_destroy(bwts_ctx *ctx)
{
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
}
