// ctx_memory.hip -- every byte of device memory a context owns: guarded allocation, kept blocks, arena, side blocks, the segment table and its pinned copy.
#include "internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// BWTS_POISON=1 (a test switch): every block handed to a transform is filled with 0xA5 first, so that a kernel which reads memory
// nothing has written yet does so reproducibly -- whatever an earlier call or process left there -- instead of once in a blue moon
bool poison_on(const bwts_ctx *ctx) { const char *e = bwts_knob(ctx, "BWTS_POISON"); return e && e[0] == '1'; }

// device blocks of the context, with guard bands when BWTS_GUARD=1
#define GUARD_BYTE 0x5C
#define GUARD_FREED 0x5D
// BWTS_TRACE_ALLOC=1: every block the context takes or gives up, with its address range, on stderr -- the map a GPU memory fault's
// address is read against
void trace_alloc(const bwts_ctx *ctx, const char *what, const char *name, const void *p, size_t bytes)
{
    static int on = -1;
    if (on < 0) { const char *e = getenv("BWTS_TRACE_ALLOC"); on = (e && e[0] == '1') ? 1 : 0; }
    if (on) fprintf(stderr, "[bwts alloc] ctx %p %s %-16s [%p, %p) %zu bytes\n", (const void *)ctx, what, name, p, (const void *)((const char *)p + bytes), bytes);
}
hipError_t ctx_malloc(bwts_ctx *ctx, void **out, size_t bytes, const char *name)
{
    if (!ctx->guard) { const hipError_t e0 = hipMalloc(out, bytes); if (e0 == hipSuccess) trace_alloc(ctx, "device +", name, *out, bytes); return e0; }
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes + 2 * ctx->guard);
    if (e != hipSuccess) return e;
    e = hipMemset(p, GUARD_BYTE, ctx->guard);
    if (e == hipSuccess) e = hipMemset((char *)p + ctx->guard + bytes, GUARD_BYTE, ctx->guard);
    if (e != hipSuccess) { (void)hipFree(p); return e; }
    *out = (char *)p + ctx->guard;
    ctx->guard_blocks.push_back({(char *)*out, bytes, name});
    return hipSuccess;
}
hipError_t ctx_free(bwts_ctx *ctx, void *user)
{
    trace_alloc(ctx, "device -", "", user, 0);
    if (!ctx->guard) return hipFree(user);
    for (size_t i = 0; i < ctx->guard_blocks.size(); i++)
        if (ctx->guard_blocks[i].user == (char *)user) {
            const bwts_ctx::GuardBlock b = ctx->guard_blocks[i];
            ctx->guard_blocks.erase(ctx->guard_blocks.begin() + (long)i);
            // blocks of up to 64 MiB are not handed back: they stay mapped, filled with a pattern that guard_check() looks at
            if (b.bytes <= ((size_t)64 << 20) && hipDeviceSynchronize() == hipSuccess &&
                hipMemset((char *)user - ctx->guard, GUARD_FREED, b.bytes + 2 * ctx->guard) == hipSuccess) {
                ctx->guard_freed.push_back(b);
                return hipSuccess;
            }
            break;
        }
    return hipFree((char *)user - ctx->guard);
}
int guard_check(bwts_ctx *ctx, const char *what)
{
    if (!ctx->guard) return BWTS_OK;
    std::vector<unsigned char> h(ctx->guard);
    int bad = 0;
    for (const auto &b : ctx->guard_blocks)
        for (int side = 0; side < 2; side++) {
            const char *src = side == 0 ? b.user - ctx->guard : b.user + b.bytes;
            HIPC(hipMemcpy(h.data(), src, ctx->guard, hipMemcpyDeviceToHost));
            size_t first = ctx->guard, last = 0, count = 0;
            for (size_t i = 0; i < ctx->guard; i++)
                if (h[i] != GUARD_BYTE) { if (first == ctx->guard) first = i; last = i; count++; }
            if (count) {
                bad++;
                fprintf(stderr, "[bwts guard] %s: block '%s' (%zu bytes): %zu byte(s) written %s it, offsets %ld .. %ld relative to the block's %s; first bytes:", what,
                        b.name, b.bytes, count, side == 0 ? "IN FRONT OF" : "BEHIND", side == 0 ? (long)first - (long)ctx->guard : (long)first,
                        side == 0 ? (long)last - (long)ctx->guard : (long)last, side == 0 ? "start" : "end");
                for (size_t i = first; i < first + 16 && i < ctx->guard; i++) fprintf(stderr, " %02x", h[i]);
                fprintf(stderr, "\n");
                HIPC(hipMemset((void *)src, GUARD_BYTE, ctx->guard));
            }
        }
    for (const auto &b : ctx->guard_freed) {
        const size_t total = b.bytes + 2 * ctx->guard;
        std::vector<unsigned char> f(total);
        HIPC(hipMemcpy(f.data(), b.user - ctx->guard, total, hipMemcpyDeviceToHost));
        size_t first = total, last = 0, count = 0;
        for (size_t i = 0; i < total; i++)
            if (f[i] != GUARD_FREED) { if (first == total) first = i; last = i; count++; }
        if (count) {
            bad++;
            fprintf(stderr, "[bwts guard] %s: GIVEN-UP block '%s' (%zu bytes) was written after the context let go of it: %zu byte(s), offsets %ld .. %ld from its start; first bytes:",
                    what, b.name, b.bytes, count, (long)first - (long)ctx->guard, (long)last - (long)ctx->guard);
            for (size_t i = first; i < first + 16 && i < total; i++) fprintf(stderr, " %02x", f[i]);
            fprintf(stderr, "\n");
            HIPC(hipMemset(b.user - ctx->guard, GUARD_FREED, total));
        }
    }
    return bad ? BWTS_E_INTERNAL : BWTS_OK;
}

// ------------------------------------------------------------------------------------
// kept blocks
// ------------------------------------------------------------------------------------
// The one place that frees a block the context keeps.  A kept block changes hands on the thread that owns the context, and only with
// the context's stream drained: nothing that was enqueued can still use the block that is given up.  (a GPU
// memory fault followed frees that did not wait -- an arena re-reserved from a helper thread, a device input buffer replaced while the
// previous call's copy could still read it.)
int kept_give_up(bwts_ctx *ctx, KeptBlock &b)
{
    if (!b.p) return BWTS_OK;
    HIPC(hipStreamSynchronize(ctx->stream));
    HIPC(ctx_free(ctx, b.p));
    b.p = nullptr;
    b.cap = 0;
    return BWTS_OK;
}

// contents of a previous, smaller block are never live across this call
int kept_grow(bwts_ctx *ctx, KeptBlock &b, size_t bytes, size_t round, int host_cost)
{
    bytes = align_up(bytes, round);
    if (bytes <= b.cap) return BWTS_OK;
    const double t0 = wall_ms();
    BWTS_TRY(kept_give_up(ctx, b));
    void *p = nullptr;
    if (ctx_malloc(ctx, &p, bytes, b.name) != hipSuccess) { (void)hipGetLastError(); return BWTS_E_NOMEM; }
    b.p = (char *)p;
    b.cap = bytes;
    if (host_cost >= 0) ctx->host_ms[host_cost] += wall_ms() - t0;
    return BWTS_OK;
}

// the wide forward's tied-list blocks are plain hipMalloc blocks (no guard bands, not traced); they leave all at once
int tied_release(bwts_ctx *ctx)
{
    if (ctx->tied_blk.empty()) return BWTS_OK;
    HIPC(hipStreamSynchronize(ctx->stream));
    for (char *b : ctx->tied_blk) HIPC(hipFree(b));
    ctx->tied_blk.clear();
    return BWTS_OK;
}

size_t ctx_device_bytes(const bwts_ctx *ctx)
{
    size_t sum = ctx->call_block_bytes + ctx->tied_blk.size() * ((size_t)16 << ctx->tied_blk_lg);
    for (const KeptBlock &b : ctx->kept) sum += b.cap;
    return sum;
}

// ------------------------------------------------------------------------------------
// the segment table and its pinned copy (layout: seg_layout.h), the segment scratch
// ------------------------------------------------------------------------------------
int seg_table_set(bwts_ctx *ctx, const uint64_t *lengths, uint64_t count, u64 *total)
{
    if (!ctx || !lengths || count == 0) return BWTS_E_ARG;
    u64 sum = 0;
    for (u64 s = 0; s < count; s++) {
        if (lengths[s] == 0 || lengths[s] > ~0ull - sum) return BWTS_E_ARG;
        sum += lengths[s];
    }
    if (sum > NARROW_N) return BWTS_E_RANGE;
    HIPC(hipSetDevice(ctx->device));
    ctx->seg_off.resize(count + 1);
    ctx->seg_off[0] = 0;
    for (u64 s = 0; s < count; s++) ctx->seg_off[s + 1] = ctx->seg_off[s] + lengths[s];
    const size_t bytes = seg_offset_words(count) * sizeof(u64), room = seg_room_bytes(count);
    BWTS_TRY(kept_grow(ctx, ctx->kept[KB_SEG_TABLE], room, 1 << 16, -1));
    // the table travels from a pinned block on the context's stream, ahead of the transform (the stream is idle between calls: the wait
    // only makes sure no earlier copy still reads the block)
    HIPC(hipStreamSynchronize(ctx->stream));
    if (room > ctx->h_seg_cap) {
        if (ctx->h_seg_off) { HIPC(hipHostFree(ctx->h_seg_off)); ctx->h_seg_off = nullptr; ctx->h_seg_cap = 0; }
        void *p = nullptr;
        if (hipHostMalloc(&p, room, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return BWTS_E_NOMEM; }
        ctx->h_seg_off = (u64 *)p;
        ctx->h_seg_cap = room;
    }
    memcpy(ctx->h_seg_off, ctx->seg_off.data(), bytes);
    HIPC(hipMemcpyAsync(d_seg_off(ctx), ctx->h_seg_off, bytes, hipMemcpyHostToDevice, ctx->stream));
    *total = sum;
    return BWTS_OK;
}

void seg_pinned_free(bwts_ctx *ctx) { if (ctx->h_seg_off) (void)hipHostFree(ctx->h_seg_off); }      // (bwts_ctx_destroy)

// `words` u64 from word `at` of the pinned copy (a region of seg_layout.h), for the host to read or write
int seg_pinned_region(bwts_ctx *ctx, u64 at, u64 words, void **p)
{
    if ((at + words) * sizeof(u64) > ctx->h_seg_cap) return BWTS_E_INTERNAL;
    *p = ctx->h_seg_off + at;
    return BWTS_OK;
}

int seg_upload_extra(bwts_ctx *ctx, const u64 *words, u64 count, u64 **d_words)
{
    const u64 at = seg_upload_at(ctx->seg_off.size() - 1);
    void *h = nullptr;
    if ((at + count) * sizeof(u64) > ctx->kept[KB_SEG_TABLE].cap || seg_pinned_region(ctx, at, count, &h) != BWTS_OK) return BWTS_E_INTERNAL;
    memcpy(h, words, count * sizeof(u64));
    HIPC(hipMemcpyAsync(d_seg_off(ctx) + at, h, count * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    *d_words = d_seg_off(ctx) + at;
    return BWTS_OK;
}

int seg_scratch_reserve(bwts_ctx *ctx, size_t bytes, u8 **out)
{
    BWTS_TRY(kept_grow(ctx, ctx->kept[KB_SEG_SCRATCH], bytes, 1 << 20, -1));
    *out = (u8 *)ctx->kept[KB_SEG_SCRATCH].p;
    return BWTS_OK;
}

static int poison(bwts_ctx *ctx, const KeptBlock &b)
{
    if (b.p && poison_on(ctx)) HIPC(hipMemsetAsync(b.p, 0xA5, b.cap, ctx->stream));
    return BWTS_OK;
}

// ------------------------------------------------------------------------------------
// the arena and the side blocks
// ------------------------------------------------------------------------------------
int arena_release(bwts_ctx *ctx)
{
    ctx->arena_off = 0;
    return kept_give_up(ctx, ctx->kept[KB_ARENA]);
}

void arena_install(bwts_ctx *ctx, void *block, size_t bytes, double alloc_ms)
{
    trace_alloc(ctx, "device +", "arena", block, bytes);
    ctx->kept[KB_ARENA].p = (char *)block;
    ctx->kept[KB_ARENA].cap = bytes;
    ctx->arena_off = 0;
    ctx->host_ms[BWTS_H_ARENA_ALLOC] += alloc_ms;
}

int arena_reserve(bwts_ctx *ctx, size_t bytes)
{
    ctx->arena_off = 0;
    BWTS_TRY(kept_grow(ctx, ctx->kept[KB_ARENA], bytes, 1 << 20, BWTS_H_ARENA_ALLOC));
    return poison(ctx, ctx->kept[KB_ARENA]);
}

void arena_reset(bwts_ctx *ctx) { ctx->arena_off = 0; }

void *arena_alloc(bwts_ctx *ctx, size_t bytes)
{
    const KeptBlock &arena = ctx->kept[KB_ARENA];
    bytes = align_up(bytes ? bytes : 1, 256);
    if (ctx->arena_off + bytes > arena.cap) return nullptr;
    void *p = arena.p + ctx->arena_off;
    trace_alloc(ctx, "  arena:", "array", p, bytes);
    ctx->arena_off += bytes;
    return p;
}

// the one block a call holds in the arena: reserved by its declared size, taken whole, every declared array pointed into it
int arena_take(bwts_ctx *ctx, const BlockLayout &L)
{
    BWTS_TRY(arena_reserve(ctx, L.bytes()));
    char *base = (char *)arena_alloc(ctx, L.bytes());
    if (!base) return BWTS_E_NOMEM;
    L.place(base);
    return BWTS_OK;
}

int aux_reserve_slot(bwts_ctx *ctx, int slot, size_t bytes, char **base)
{
    KeptBlock &b = ctx->kept[KB_AUX + slot];
    BWTS_TRY(kept_grow(ctx, b, bytes, 1 << 20, BWTS_H_ARENA_ALLOC));
    *base = b.p;
    return poison(ctx, b);
}

int aux_release(bwts_ctx *ctx)
{
    for (int i = 0; i < BWTS_AUX_SLOTS; i++) BWTS_TRY(kept_give_up(ctx, ctx->kept[KB_AUX + i]));
    return BWTS_OK;
}
