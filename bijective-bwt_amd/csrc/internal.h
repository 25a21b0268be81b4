// internal.h -- host-side plumbing shared by the engine's translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <assert.h>
#include <algorithm>
#include <utility>
#include <string>
#include <vector>
#include <functional>

#include "../../include/bwts.h"
#include "seg_layout.h"
#include "stage_cut.h"

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint16_t u16;
typedef uint8_t  u8;

struct TimedSpan {
    int cls;
    hipEvent_t a, b;
};

struct CopyPool;                 // the copy workers of a staging ring (copy_pool.h)

#define INV_REPORT_MAX 8         // (the narrow inverse's fallback chain has at most five attempts, the wide one four)
#define INV_REPORT_WORDS 16
#define SEG_REPORT_WORDS 8
enum SegReportWord { SR_PLAN, SR_BIG, SR_RUNS, SR_OWN_SEGS, SR_OWN_BYTES, SR_SINGLE_SEGS, SR_SINGLE_BYTES, SR_ATTEMPTS };
// the forward's report (bwts_debug_forward_report; include/bwts_test.h names the words): a header, then one record per later round
#define FWD_REPORT_SORTS 2       // (the suffix sort of the general Lyndon path, then the cyclic sort)
#define FWD_HEADER_WORDS 48
#define FWD_ROUND_WORDS 12
#define FWD_SORT_WORDS (FWD_HEADER_WORDS + BWTS_MAX_ROUND_STATS * FWD_ROUND_WORDS)
#define STAGE_SLOTS 4
#define BWTS_AUX_SLOTS 5

// A device block that stays with the context: grown when a call needs more, never shrunk, given up by bwts_ctx_release_memory and
// bwts_ctx_destroy (ctx_memory.hip).  name: what the allocation trace and the guard report call it.
struct KeptBlock { char *p; size_t cap; const char *name; };
// every kept block of a context, in bwts_ctx::kept
enum { KB_ARENA, KB_AUX, KB_IO = KB_AUX + BWTS_AUX_SLOTS, KB_SEG_TABLE = KB_IO + 4, KB_SEG_SCRATCH, KB_PACK, KB_MEMBER_SET = KB_PACK + 3, KB_COUNT };

#define SM_RX_SYNC 4090          // d_small word holding the two 32-bit counters of radix_column_scan_fused_kernel (zero between launches)
#define SM_EC_TOTAL 4020         // entropy coder (ec.hip): d_small word for the bytes of all payloads of an encode
#define SM_EC_FLAG  4021         // ... d_small word for what a decode found wrong (0: nothing)
#define SM_EC_HEAD  4022         // ... h_small, two words: the header of a single stream
#define SM_CRC_OUT  4024         // checksum (crc.hip): h_small word for the value of a single input
#define SM_PACK_HEAD 4026        // packed frame (pack.hip): h_small, eight words: the header and a one-block directory (version 2: 32 bytes) on their way in or out
#define SM_ZRL_TOTAL 4034        // zero-run coding (zrl.hip): d_small word for the bytes of an encode, or the weights' sum of a decode
#define SM_ZRL_FLAG  4035        // ... d_small word, right behind it, for what a decode found wrong (0: nothing)

struct Stager {
    hipStream_t stream;             // the queue its copies (and copy kernels) are issued on
    bool own_stream;
    char *pinned[STAGE_SLOTS];
    hipEvent_t slot_ev[STAGE_SLOTS], slot_ev2[STAGE_SLOTS];
    hipStream_t copy_stream;        // second queue: part of a device-to-host chunk goes through the DMA engine while a kernel moves the rest
    CopyPool *pool;
};

struct bwts_ctx {
    int device;
    hipStream_t stream;
    size_t call_block_bytes = 0;        // device memory taken for one call only (rare paths), largest of the last call
    int last_hip;

    // KB_ARENA: the device arena: one allocation, bump-allocated per call (arena_off), grown between calls.
    // KB_AUX + i: side arenas sized on demand.  0, 1: forward: tied-set buffers; inverse: unreached-element lists, cycle sort.  2: factor
    // list of the general Lyndon path.  3: previous-symbol array + carried-byte buffers (rounds-0 sorts on wide keys).  4: dense rank array.
    // (What the headline path does not touch is not allocated: the driver clears device memory it hands out, ~27 ms per GiB.)
    // KB_IO + i: the host-buffer entry points' device-side in/out buffers (below).  KB_SEG_TABLE: the device copy of the segment table.
    // KB_SEG_SCRATCH: segmented forward: factor-start flags.  KB_PACK + 0, 1: pack / unpack: the bytes between two stages of the chain; + 2: a pack
    // that chooses methods: both candidates' streams.  KB_MEMBER_SET: a pack of scattered members (bwts_pack_members_p_device): the members
    // gathered back to back.
    KeptBlock kept[KB_COUNT] = {{nullptr, 0, "arena"},
                                {nullptr, 0, "side block 0"}, {nullptr, 0, "side block 1"}, {nullptr, 0, "side block 2"},
                                {nullptr, 0, "side block 3"}, {nullptr, 0, "side block 4"},
                                {nullptr, 0, "device input 0"}, {nullptr, 0, "device input 1"},
                                {nullptr, 0, "device output 0"}, {nullptr, 0, "device output 1"},
                                {nullptr, 0, "segment table"}, {nullptr, 0, "segment scratch"},
                                {nullptr, 0, "pack stage 0"}, {nullptr, 0, "pack stage 1"}, {nullptr, 0, "pack candidates"},
                                {nullptr, 0, "member set"}};
    size_t arena_off;
    size_t unv_hint;       // inverse: unreached elements seen by the previous call (sizes the first collection pass)
    // inverse: one record per attempt of the most recent call, from values its stages hold on the host anyway (a few stores per
    // attempt); bwts_debug_inverse_report is the only reader and include/bwts_test.h names the words
    u64 inv_report[INV_REPORT_MAX][INV_REPORT_WORDS];
    u32 inv_attempts_made = 0;          // attempts of that call (the records of those past INV_REPORT_MAX are dropped)
    // forward: one record per doubling sort of the most recent call, likewise from values the stages read back anyway;
    // bwts_debug_forward_report is the only reader
    u64 fwd_report[FWD_REPORT_SORTS][FWD_SORT_WORDS];
    u32 fwd_sorts_made = 0;             // sorts of that call (a third one and later overwrite the last record)
    // tied list of the forward transform beyond 2^32 positions (wide_path.h): blocks of 2^tied_blk_lg (position, head) pairs, taken as the
    // list grows and kept for the next call
    std::vector<char *> tied_blk;
    int tied_blk_lg = 0;
    // BWTS_GUARD=1 (a test switch): every block the context takes from the device gets `guard` bytes of a fixed pattern in front and
    // behind, checked after every transform: a kernel that writes outside its buffers is named, with the block and the offset
    size_t guard = 0;
    struct GuardBlock { char *user; size_t bytes; const char *name; };
    std::vector<GuardBlock> guard_blocks;
    std::vector<GuardBlock> guard_freed;         // ... and what the context has given up stays mapped, filled with a second pattern: a write through a stale pointer shows

    // small pinned host block for read-backs, and a device mirror
    u64 *h_small;          // 4096 u64
    u64 *d_small;          // 4096 u64

    // host-buffer entry points: staging (a ring of pinned slots with one event each, copy workers, a queue of its own), device-side
    // in/out buffers that stay with the context, and the pinned blocks handed out by bwts_host_alloc.  stg[0] serves the single
    // calls on the context's own stream; the batch entry points move the neighbouring items' data on stg[1] (in) and stg[2] (out)
    // while the current item is transformed, between two pairs of device buffers (d_io(ctx, 0..1) in, d_io(ctx, 2..3) out).
    Stager stg[3];
    std::vector<std::pair<char *, size_t>> host_blocks;

    // event pool + spans of the current call
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used;
    std::vector<TimedSpan> spans;
    hipEvent_t ev_begin, ev_end;
    int timing;            // HIP-event spans: 0 none (counters only), 1 dominant kernels, 2 all (bwts_set_timing / BWTS_TIMINGS=1)

    // kernels that were granted more than 64 KB of dynamic LDS on this context's device (the attribute is per device)
    std::vector<const void *> lds_granted;

    // environment knobs, read ONCE when the context is made (bwts_knob()): diagnostics and staging tuning always, the switches that
    // select alternate code paths -- what the test suite drives -- only when BWTS_TEST_KNOBS=1 is set
    std::vector<std::pair<std::string, std::string>> knobs;
    int fused_scan_cap;    // workgroups of radix_column_scan_fused_kernel that are certain to be resident together (0 = not yet asked)

    // segment table of the current segmented call: offsets on the host (count + 1); their device copy is d_seg_off(ctx)
    std::vector<u64> seg_off;
    u64 *h_seg_off = nullptr;           // pinned copy of the table and what lies behind it: ctx_memory.hip alone reads these two
    size_t h_seg_cap = 0;
    // inverse: what the most recent segmented inverse did (bwts_debug_segments_report; include/bwts_test.h names the words)
    u64 seg_report[SEG_REPORT_WORDS] = {0};
    bool crc_tables = false;            // the checksum's tables (crc.hip) have been made on this context's device
    // ranges of a frame: what the most recent call did (bwts_debug_unpack_ranges_report; include/bwts_test.h names the words)
    u64 ranges_report[8] = {0};

    bwts_timings tm;
    double host_ms[BWTS_H_COUNT];   // cumulative host-side costs (BWTS_H_*)
    bool launched;                  // a kernel of this context has run (the code object is loaded)
};

// BWTS_STAGE_TRACE=1 (diagnosis): the stream is drained after every stage of a transform and the stage is named on stderr, so that
// a GPU fault -- reported asynchronously -- is known to come from the stage after the last one named
void bwts_stage_mark(bwts_ctx *ctx, const char *name);
#define STAGE(name) bwts_stage_mark(ctx, name)

#define HIPC(call)                                                        \
    do {                                                                  \
        hipError_t e__ = (call);                                          \
        if (e__ != hipSuccess) { ctx->last_hip = (int)e__; return BWTS_E_HIP; } \
    } while (0)

// BWTS_TRACE_ERRORS=1: every failing call on the way up prints its place (a debugging aid; costs nothing until something fails)
void bwts_trace_error(const char *file, int line, int rc);
#define BWTS_TRY(call)                   \
    do {                                 \
        int rc__ = (call);               \
        if (rc__ != BWTS_OK) { bwts_trace_error(__FILE__, __LINE__, rc__); return rc__; } \
    } while (0)

const char *bwts_knob(const bwts_ctx *ctx, const char *name);    // value of an environment knob as the context saw it, or null

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
double wall_ms(void);
#define NARROW_N 0x100000000ull  // the narrow limit: up to this many positions an index is 32 bits wide (host code; kernels spell it out)
// do [a, a + na) and [b, b + nb) share a byte?  By subtraction: a length as large as 2^64 - 1 must not wrap the comparison
static inline bool ranges_overlap(const void *a, u64 na, const void *b, u64 nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x <= y ? y - x < na : x - y < nb;
}

// do no two of the spans (address, bytes >= 1) share a byte?  Sorts them.  An address space ends below 2^64: no sum wraps for spans that exist
static inline bool spans_disjoint(std::vector<std::pair<u64, u64>> &spans)
{
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); i++)
        if (spans[i].first - spans[i - 1].first < spans[i - 1].second) return false;
    return true;
}

// ---- the call bracket and the transform table (api.hip) ---------------------------
// One of the eight transforms that map n bytes to n bytes.  name: what a call is called in the guard report; in_label: its input in
// the allocation trace; arena_hint: what the host path reserves ahead of the call (0: the call's own reservation decides).
struct Transform {
    int (*fn)(bwts_ctx *, const u8 *, u64, u8 *);
    const char *name, *in_label;
    size_t (*arena_hint)(const bwts_ctx *ctx, u64 n);
};
int run_device(bwts_ctx *ctx, const Transform &t, const void *d_in, u64 n, void *d_out);    // the bracket around one row's device form
// the first launch of a context is this kernel with nothing to copy: it loads the library's code object outside the timing
__global__ void pcie_copy_kernel(uint4 *__restrict__ dst, const uint4 *__restrict__ src, u64 vecs, u8 *__restrict__ dst_tail, const u8 *__restrict__ src_tail, u32 tail);

// ---- between caller memory and HBM (staging.hip) -----------------------------------
// One host call: `in` to the device, the device form, what it made back to `out` (or to `sink`, piece by piece), the copy times
// booked in h2d_ms / d2h_ms.  Nothing reaches out, sink or *out_bytes unless the device form succeeded.
struct HostTrip {
    const u8 *in; u64 in_bytes;
    u64 io_bytes;                           // room in the device-side input and output buffer
    u8 *out; u64 *out_bytes;
    bwts_sink_fn sink = nullptr; void *user = nullptr;
    // the n -> n transforms only (out is in_bytes long): the arena reserved ahead of the call where the rules in staging.hip allow
    // it, the pages of a fresh `out` faulted in while the device works, and the call's two lines in the allocation trace
    const Transform *ahead = nullptr;
};
// device_form(d_in, d_out, &bytes): the public _device entry point, which says how many bytes it made
int host_round_trip(bwts_ctx *ctx, const HostTrip &trip, const std::function<int(const u8 *, u8 *, u64 *)> &device_form);
int run_batch(bwts_ctx *ctx, const Transform &t, int count, const uint8_t *const *ins, const uint64_t *ns, uint8_t *const *outs);
void staging_destroy(bwts_ctx *ctx);        // bwts_ctx_destroy: workers, pinned slots, events and queues of the three stagers

// ---- the context's device memory (ctx_memory.hip) -------------------------------
hipError_t ctx_malloc(bwts_ctx *ctx, void **out, size_t bytes, const char *name);   // with guard bands under BWTS_GUARD
hipError_t ctx_free(bwts_ctx *ctx, void *user);
int  guard_check(bwts_ctx *ctx, const char *what);      // after a transform: are all guard bands intact?
void trace_alloc(const bwts_ctx *ctx, const char *what, const char *name, const void *p, size_t bytes);   // BWTS_TRACE_ALLOC=1
bool poison_on(const bwts_ctx *ctx);
// room for `bytes`, rounded up to a multiple of `round`, in a kept block; host_cost: the BWTS_H_* the wall time of a growth is
// booked to, or -1.  A block that is large enough is left alone; one that is refused is left empty (BWTS_E_NOMEM).
int  kept_grow(bwts_ctx *ctx, KeptBlock &b, size_t bytes, size_t round, int host_cost);
int  kept_give_up(bwts_ctx *ctx, KeptBlock &b);         // drains the context's stream, then frees (calling thread only)
size_t ctx_device_bytes(const bwts_ctx *ctx);           // what the context holds on the device: bwts_timings::device_bytes
int  tied_release(bwts_ctx *ctx);                       // the wide forward's tied-list blocks (wide_path.h): drains, then frees
static inline u8 *d_io(const bwts_ctx *ctx, int i) { return (u8 *)ctx->kept[KB_IO + i].p; }
static inline u64 *d_seg_off(const bwts_ctx *ctx) { return (u64 *)ctx->kept[KB_SEG_TABLE].p; }
// the segment table, and the regions behind it in its pinned copy (seg_layout.h); a region the block has no room for: BWTS_E_INTERNAL
int  seg_table_set(bwts_ctx *ctx, const uint64_t *lengths, uint64_t count, u64 *total);     // the segment table of the calls that follow
int  seg_upload_extra(bwts_ctx *ctx, const u64 *words, u64 count, u64 **d_words);   // a second table, behind the segment table
int  seg_pinned_region(bwts_ctx *ctx, u64 at, u64 words, void **p);                 // a region behind the table, in the pinned copy, with its capacity check
void seg_pinned_free(bwts_ctx *ctx);
int  seg_scratch_reserve(bwts_ctx *ctx, size_t bytes, u8 **p);     // a device block that stays with the context, grown on demand

// ---- arena -------------------------------------------------------------------
int  arena_reserve(bwts_ctx *ctx, size_t bytes);        // (re)allocates when too small; resets
int  arena_release(bwts_ctx *ctx);                      // gives the arena up (calling thread only)
void arena_install(bwts_ctx *ctx, void *block, size_t bytes, double alloc_ms);
void arena_reset(bwts_ctx *ctx);
void *arena_alloc(bwts_ctx *ctx, size_t bytes);         // NULL when exhausted
struct BlockLayout;
int  arena_take(bwts_ctx *ctx, const BlockLayout &L);   // reserves a declared layout's bytes(), takes them whole and places the layout; BWTS_E_NOMEM
template <typename T> static inline T *arena_array(bwts_ctx *ctx, u64 count)
{
    return (T *)arena_alloc(ctx, (size_t)count * sizeof(T));
}

// opt-in for > 64 KB of dynamic LDS, once per kernel and context (a context is bound to one device)
int ensure_dyn_lds(bwts_ctx *ctx, const void *kernel, size_t bytes);

// ---- timing ------------------------------------------------------------------
int  span_begin(bwts_ctx *ctx, int cls, u64 elems, u64 alg_bytes);   // returns a span handle (spans may nest)
void span_end(bwts_ctx *ctx, int span);
void spans_reset(bwts_ctx *ctx);
int  spans_resolve(bwts_ctx *ctx);

struct SpanGuard {
    bwts_ctx *c;
    int h;
    SpanGuard(bwts_ctx *ctx, int cls, u64 elems, u64 alg_bytes) : c(ctx), h(span_begin(ctx, cls, elems, alg_bytes)) {}
    ~SpanGuard() { span_end(c, h); }
};

// ---- read-back of a few u64 words (synchronises the stream) --------------------
int read_small(bwts_ctx *ctx, int first, int count);    // d_small[first..) -> h_small[first..)

// ---- device-wide primitives (scan.hip) ------------------------------------------
size_t scan_temp_bytes(u64 n);
int exclusive_sum_u32(bwts_ctx *ctx, u32 *data, u64 n, void *temp);   // in place, wraps mod 2^32

// ---- LSD radix sort of (u64 key, u32 value) pairs (radix.hip) -------------------
struct SortPlan {
    u64  *keys[2];
    u32  *vals[2];
    u32  *tile_hist;      // 256 * tiles(m)
    void *scan_temp;
    // optional third stream: one byte per element travels with the pair (all three may be null)
    const u8 *sym_src = nullptr;     // byte of element i before the first pass
    u8 *sym_buf[2] = {nullptr, nullptr};
    u8 *sym_final = nullptr;         // where the last pass leaves the bytes
    bool vals_identity = false;      // vals[0] is not read: the first pass uses value = element index
    // keys[0] holds the keys split for the packed sort (radix_packed_applicable()): u32 low words at keys[0], and at
    // (u8 *)keys[0] + align_up(4 m, 256) the c stream: u16 (key bits 32..39 | carried byte << 8) for keys of more than 32
    // bits, else u8 (the carried byte).  sym_src is not read; needs sym_final and vals_identity.  The sorted keys come out split
    // too: u32 low words at keys[res], and for keys of more than 32 bits their bits 32..39 as u8 at (u8 *)keys[res] + align_up(4 m, 256).
    bool keys_split = false;
    // keys_split only, may be null: the first pass's [tile][digit] table (8192-element tiles, digit = key bits 0..7), counted
    // already, in a block of radix_tile_hist_bytes(m) that no pass writes but the first one's scan; that pass's histogram sweep is skipped
    u32 *first_hist = nullptr;
    // keys_split with five passes only: the last pass writes the byte stream and, instead of the sorted keys and the values, the group
    // flags of its output (radix.hip, radix_scatter_lean_last_kernel): headw, keepw of (m + 63) / 64 words each, which the caller has
    // filled with ones (up to m) and zeros; vals[res] at the tied slots only; *seam_giveup (zero before) set when the flags cannot be
    // trusted.  keys[res ^ 1] and vals[res ^ 1] stay as the fourth pass left them (radix_packed_last_pass), keys[res] is not written.
    bool lean_last = false;
    u64 *headw = nullptr, *keepw = nullptr, *seam_giveup = nullptr;
};
// a plain pair sort over two key and two value buffers (the optional fields stay as above)
static inline SortPlan sort_plan(u64 *k0, u64 *k1, u32 *v0, u32 *v1, u32 *tile_hist, void *scan_temp)
{
    SortPlan p;
    p.keys[0] = k0; p.keys[1] = k1; p.vals[0] = v0; p.vals[1] = v1; p.tile_hist = tile_hist; p.scan_temp = scan_temp;
    return p;
}
bool radix_packed_applicable(const bwts_ctx *ctx, u64 m, int key_bits);   // will radix_sort_pairs run its packed-stream passes for such a sort?
size_t radix_tile_hist_bytes(u64 m);
// Sorts on key bits [0, key_bits); returns in *result_buf which of keys[]/vals[] holds the output.
int radix_sort_pairs(bwts_ctx *ctx, const SortPlan &plan, u64 m, int key_bits, int *result_buf);
int radix_packed_last_pass(bwts_ctx *ctx, const SortPlan &plan, u64 m);   // the classic fifth pass behind a lean one that gave up
int radix_debug_rank_steps(bwts_ctx *ctx, const u8 *d_digits, const u8 *d_valid, int atomic_items, u32 *d_ranks, u32 shipped[4]);   // bwts_test.h
int radix_column_scan(bwts_ctx *ctx, u32 *tile_hist, u64 tiles, void *scan_temp);
int radix_sort_keys(bwts_ctx *ctx, u64 *keys[2], u32 *tile_hist, void *scan_temp, u64 m, int lo_bit, int bits, int *result_buf);

// ---- forward / inverse drivers ----------------------------------------------------
int forward_device_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out);
// independent segments (bwts_forward_segments / bwts_inverse_segments): the table set on the context by the entry point
// d_off: count + 1 device words, d_off[0] = 0, d_off[count] = n; flag: n bytes of factor-start flags (forward)
struct SegTable { const u64 *d_off; u64 count; u8 *flag; };
#define SEG_FWD_BIG (1ull << 21)     // forward: segments of this length or more are transformed alone
int forward_segments_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out);
int inverse_segments_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out);
size_t inverse_segments_arena_bytes(const bwts_ctx *ctx, u64 n);   // for the context's current segment table, by the plan the call will take
int inverse_segments_plan_words(const u64 *lengths, u64 count, u64 out[8]);   // bwts_debug_segments_plan: no context, no device
int inverse_device_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out);
size_t forward_arena_bytes(u64 n);
int forward_wide_arena_probe(u64 n, int mode, int seg_log2, u64 bucket_cap, u64 *bytes);   // wide_path.h, for bwts_debug_wide_forward_arena
// the inverse's arena as plain arithmetic (the bwts_debug_inverse_arena test hook asks them too): the splitter spacing the narrow
// form picks, what one attempt reserves (mark: 0 index log, 1 sentinel, 2 byte map, 3 moments), what the host path allocates ahead
int    inverse_splitter_log2(u64 n);
size_t inverse_attempt_bytes(u64 n, int g, int mark);
size_t inverse_arena_bytes(u64 n);

// ---- the stages behind the transform: which input a call works on, and its cut (stage_cut.h) ----
static inline SegMode seg_mode(const bwts_ctx *ctx) { return SegMode{ctx->seg_off.empty() ? 0 : (u64)ctx->seg_off.size() - 1}; }     // the context's table
static inline StageCut stage_cut_call(const bwts_ctx *ctx, SegMode segs, u64 n, u64 unit_a, u64 unit_b = 0)
{
    return stage_cut_call(ctx->seg_off, segs, n, unit_a, unit_b);
}

// ---- move-to-front (mtf.hip; include/bwts_mtf.h) ----
int mtf_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, bool inverse, SegMode segs);
size_t mtf_arena_bytes(const bwts_ctx *ctx, u64 n, SegMode segs);      // what a call reserves: 256 bytes per tile and a little per group
void bwts_mtf_plan(u64 n, u64 out[4]);                                  // tile size, tiles per group, tiles and groups of one input of n bytes

// ---- entropy coding behind move-to-front (ec.hip) -----------------------------------
// sizes: the stream's bytes, or one per segment; decode: the one stream of in_bytes, or stream_bytes[count] (in_bytes: the lengths' sum)
int ec_encode_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, u64 out_cap, SegMode segs, u64 *sizes);
int ec_decode_impl(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, u8 *d_out, u64 out_cap, u64 *n_out, SegMode segs, const u64 *stream_bytes);
void bwts_ec_plan(u64 n, u64 out[5]);                                   // tile size, tiles per block, tiles, blocks and the bound of one input

// ---- zero-run coding between move-to-front and the entropy coder (zrl.hip; include/bwts_zrl.h) ----
// sizes: the bytes the input becomes, or one per segment; decode: the one coded input of in_bytes, or in_lengths[count] (in_bytes: their sum)
int zrl_encode_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u8 *d_out, u64 out_cap, SegMode segs, u64 *sizes);
int zrl_decode_impl(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, u8 *d_out, u64 n, SegMode segs, const u64 *in_lengths);
void bwts_zrl_plan(u64 n, u64 out[2]);                                  // tile size and tiles of one input of n bytes

// ---- byte-plane split in front of the transform (planes.hip; include/bwts_planes.h) ----
int planes_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u32 w, u8 *d_out, bool join, SegMode segs);
int planes_w_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, const u32 *widths, u8 *d_out, bool join);     // the context's table, a width (1, 2, 4, 8) per segment
void bwts_planes_plan(u64 n, u32 w, u64 out[4]);                        // tile bytes, tiles, elements and tail bytes of one input of n bytes

// ---- delta filter in front of the byte-plane split (delta.hip; include/bwts_delta.h) ----
int delta_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u32 w, u8 *d_out, bool decode);                 // one input of n bytes at width 1, 2, 4 or 8
int delta_f_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, const u32 *widths, const u32 *filters, u8 *d_out, bool decode);   // the context's table, a width and a filter per segment

// ---- plane costs of the members of the context's table under both filters (estimate.hip; include/bwts_members.h) ----
// take: null for every member, or a byte per member (zero: left out, its estimates are 0)
int estimate_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, const u32 *widths, const u8 *take, u64 *est_none, u64 *est_delta);

// ---- checksum and the packed frame (crc.hip, pack.hip; include/bwts_pack.h) ------------
// one value for the input of n bytes, or one per segment, to the host
int crc_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, SegMode segs, u32 *crcs);
void bwts_crc_plan(u64 n, u64 out[4]);                                  // tile size, tiles per fold group, tiles and groups of one input
int pack_device_impl(bwts_ctx *ctx, u32 version, u32 width, const u8 *d_in, u64 n, u64 B, u8 *d_out, u64 out_cap, u64 *out_bytes);   // width: version 3 only
int unpack_device_impl(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, u8 *d_out, u64 out_cap, u64 *n_out);
// ranges of a frame (pack_plan.h names the three types).  packed: d_in holds header, directory and behind them the covered blocks'
// streams alone, back to back (the host form); in_bytes stays the whole frame's length
struct PackRange;
struct PackPiece;
struct MemberDsts;
// indices: not null for whole members of a member frame as the ranges (ranges is then not read; count indices)
int unpack_ranges_device_impl(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, bool packed, const PackRange *ranges, u64 count, u8 *d_out, u64 out_cap, u64 *out_bytes,
                              const u64 *indices = nullptr, const MemberDsts *ptrs = nullptr);
// the member frame (include/bwts_members.h); lengths, widths, filters (null: none) and methods (null: the whole chain) have passed
// members_args_check_m, n is the lengths' sum
int pack_members_device_impl(bwts_ctx *ctx, const u8 *d_in, const u64 *lengths, const u32 *widths, const u32 *filters, const u32 *methods, u64 count, u64 n,
                             u8 *d_out, u64 out_cap, u64 *out_bytes);
// the same with MEMBERS_AUTO among filters and methods, resolved by the rules of include/bwts_members.h ("AUTO"); arguments that have
// passed members_args_check_a; filters_out, methods_out: null, or room for the resolved values
int pack_members_auto_device_impl(bwts_ctx *ctx, const u8 *d_in, const u64 *lengths, const u32 *widths, const u32 *filters, const u32 *methods, u64 count, u64 n,
                                  u8 *d_out, u64 out_cap, u64 *out_bytes, u32 *filters_out, u32 *methods_out);
// pieces of one device buffer to another, at any alignment (pieces.hip); every piece inside both buffers, by the caller's check
int copy_pieces_impl(bwts_ctx *ctx, const u8 *d_src, u64 src_bytes, const PackPiece *pieces, u64 count, u8 *d_dst);
// the same between scattered buffers: src and dst of a piece are absolute device addresses, and every piece is a buffer of its own
int scatter_pieces_impl(bwts_ctx *ctx, const PackPiece *pieces, u64 count);
// the destinations of bwts_unpack_members_p_device: one per index, with its room
struct MemberDsts { void *const *dsts; const u64 *dst_bytes; };

// chunk tables of the forward's later rounds (chunk_rounds.h) as plain arithmetic: nominal chunk size of a list, the tables' capacity
// for a tied list of a0 (which holds every run: the derivation stands at chunk_table_capacity), and the re-cut of the a_chunks elements
// left at a compaction.  target: the chunks a cut aims at, CH_CHUNK_TARGET unless the test switch BWTS_CHUNK_TARGET (16 .. 16384) is set
#define CH_CHUNK_TARGET 16384
struct ChunkRecut { u32 S; u64 nc; };
u32 chunk_nominal_size(u64 a, u32 target);
u64 chunk_table_capacity(u64 a0);
ChunkRecut chunk_recut_plan(u64 a_chunks, u32 target);

// non-cyclic suffix sort: leaves the suffix array in *d_sa (arena memory) and ranks in *d_rank
int suffix_sort_device(bwts_ctx *ctx, const u8 *d_T, u64 n, u32 **d_sa, u32 **d_rank, u32 *rounds);
int lyndon_factors_device(bwts_ctx *ctx, const u8 *d_T, u64 n, u32 **d_fstart, u64 *k, u32 *rounds);
int byte_histogram_device(bwts_ctx *ctx, const u8 *d_T, u64 n, u64 *d_hist256);
int constant_input_probe(bwts_ctx *ctx, const u8 *d_in, u64 n, bool *constant);   // one byte value repeated?
int aux_reserve_slot(bwts_ctx *ctx, int slot, size_t bytes, char **base);   // side arenas, sized on demand
static inline int aux_reserve(bwts_ctx *ctx, size_t bytes, char **base) { return aux_reserve_slot(ctx, 0, bytes, base); }
int aux_release(bwts_ctx *ctx);      // gives every side arena back (their contents are dead)

// The arrays of one side block, declared once and in order, each rounded up to 256 bytes: bytes() is what to reserve, place()
// points every declared array into the block.  No allocator and no ownership: the pointers named must outlive place().
struct BlockLayout {
    struct Field { void *var; size_t off; void (*set)(void *var, char *p); };
    Field f[32];
    int count = 0;
    size_t total = 0;
    template <typename T> static size_t padded(u64 n) { return align_up((size_t)n * sizeof(T), 256); }
    template <typename T> void array(T **var, u64 n) { raw(var, padded<T>(n)); }
    template <typename... T> void arrays(u64 n, T **...vars) { (array(vars, n), ...); }      // several arrays of n elements each
    template <typename T> void raw(T **var, size_t bytes)         // a field of exactly `bytes` (sizes that come rounded already)
    {
        assert(count < (int)(sizeof f / sizeof f[0]));
        f[count++] = Field{var, total, [](void *v, char *p) { *(T **)v = (T *)p; }};
        total += bytes;
    }
    void pad(size_t bytes) { total += bytes; }
    size_t bytes() const { return total; }
    void place(char *base) const { for (int i = 0; i < count; i++) f[i].set(f[i].var, base + f[i].off); }
    // a second layout over a block of `cap` bytes that is reserved already: false, and nothing placed, when it does not fit
    bool place_within(char *base, size_t cap) const { if (bytes() > cap) return false; place(base); return true; }
};

// The buffers of a pair sort of up to m elements as one group of a layout: key and value ping-pong, the passes' [tile][digit] table
// (with its chunk table behind it) and the scans' partials
struct SortBufs {
    u64  *keys[2];
    u32  *vals[2], *tile_hist;
    void *scan_temp;
    void declare(BlockLayout &L, u64 m)
    {
        L.arrays(m, &keys[0], &keys[1]); L.arrays(m, &vals[0], &vals[1]);
        L.raw(&tile_hist, radix_tile_hist_bytes(m)); L.raw(&scan_temp, scan_temp_bytes(m));
    }
    SortPlan plan() const { return sort_plan(keys[0], keys[1], vals[0], vals[1], tile_hist, scan_temp); }
};

// ---- generators / utilities (gen.hip) ------------------------------------------------
int generate_device_impl(bwts_ctx *ctx, int kind, u64 seed, u64 n, u8 *d_out);
int device_equal_impl(bwts_ctx *ctx, const u8 *a, const u8 *b, u64 bytes, int *equal);
