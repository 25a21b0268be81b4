// pack.hip -- the chain as one call (include/bwts_pack.h): checksums, delta filter (member frame version 2), byte-plane split (frame
// version 3), transform, move-to-front, zero-run coding (frame versions 2 and 3) and entropy coder over the blocks of a frame, and the
// way back.  No kernel of its own: the stages are the ones behind the single calls, run one after the other inside
// one call bracket; the frame's arithmetic and the checks of an untrusted frame are in pack_plan.h.
//
// A frame of one block goes through the single-input stages, one of several blocks through the segment forms (the bytes are the
// same by the segment forms' contract).  The stages share the context's arena, and the segment forms the pinned staging of their
// tables: the stream is drained between two stages, so that no table copy of the stage before is still to come when the next stage
// writes its own (seg_layout.h: the regions, and who overlaps whom).  Header and directory travel through pinned memory too: the
// small block, and for several blocks the directory region behind the segment table (version 1; the 32-byte entries of version 2 do
// not fit that region and travel through a host block of the call's own).
// Versions 2 and 3 change the segment table on the way: the coder's segments are the blocks' zero-run coded bytes, every other
// stage's the blocks themselves.
// The bytes between two stages go to and fro between two blocks (pack) or between one block and d_out (unpack); where a version has
// a stage more, the directions swap, so that the last stage of an unpack always lands in d_out.
// A range read (unpack_ranges_device_impl, at the end) runs the same stages over the blocks its ranges touch, between the two blocks,
// and cuts the ranges out with pieces.hip's copy kernel.
#include "internal.h"
#include "members_plan.h"
#include "../../include/bwts_members.h"

#include <string.h>
#include <utility>

static_assert(PACK_OK == BWTS_OK && PACK_RANGE == BWTS_E_RANGE && PACK_FORMAT == BWTS_E_FORMAT && PACK_ARG == BWTS_E_ARG && PACK_SPACE == BWTS_E_SPACE,
              "pack_plan.h answers in the library's codes");

// the n-byte block between two stages
static int pack_stage(bwts_ctx *ctx, int i, u64 n, u8 **p)
{
    BWTS_TRY(kept_grow(ctx, ctx->kept[KB_PACK + i], n, 1 << 16, -1));
    *p = (u8 *)ctx->kept[KB_PACK + i].p;
    return BWTS_OK;
}

// the blocks of a frame as the segment table of the stages; one block: no table, the single-input stages
static int pack_blocks_set(bwts_ctx *ctx, u64 n, u64 B, u64 nblk)
{
    if (nblk == 1) return BWTS_OK;
    std::vector<u64> lengths((size_t)nblk, B);
    lengths[(size_t)nblk - 1] = pack_block_at(n, B, nblk - 1);
    u64 total = 0;
    BWTS_TRY(seg_table_set(ctx, lengths.data(), nblk, &total));
    return total == n ? BWTS_OK : BWTS_E_INTERNAL;
}

// room on the host for a directory of nblk entries: the small block behind the header, or for several blocks the directory region
// behind the segment table (pinned; version 1) or `own` (versions 2 and 3)
static int pack_dir_staging(bwts_ctx *ctx, u32 version, u64 nblk, std::vector<u8> &own, u8 **dir)
{
    if (nblk == 1) { *dir = (u8 *)(ctx->h_small + SM_PACK_HEAD) + PACK_HEADER_BYTES; return BWTS_OK; }
    if (version != PACK_VERSION) {
        own.resize((size_t)(PACK_ENTRY_BYTES_V2 * nblk));
        *dir = own.data();
        return BWTS_OK;
    }
    return seg_pinned_region(ctx, seg_dir_at(nblk), seg_dir_words(nblk), (void **)dir);
}

// the coder's segments of a version-2 frame of several blocks: the blocks' coded bytes
static int pack_coded_set(bwts_ctx *ctx, const std::vector<u64> &coded, u64 *total)
{
    if (coded.size() == 1) { *total = coded[0]; return BWTS_OK; }
    return seg_table_set(ctx, coded.data(), coded.size(), total);
}

int pack_device_impl(bwts_ctx *ctx, u32 version, u32 width, const u8 *d_in, u64 n, u64 B, u8 *d_out, u64 out_cap, u64 *out_bytes)
{
    const bool zrl = version != PACK_VERSION, planes = version == PACK_VERSION_3;
    const u64 nblk = pack_blocks(n, B), fixed = pack_fixed_bytes_v(version, nblk), entry = pack_entry_bytes(version);
    const bool seg = nblk > 1;
    if (out_cap < (zrl ? pack_least_bytes_v2(n, B) : pack_least_bytes(n, B))) return BWTS_E_SPACE;
    BWTS_TRY(pack_blocks_set(ctx, n, B, nblk));
    SegMode segs = seg ? seg_mode(ctx) : SEG_SINGLE;
    std::vector<u32> crcs((size_t)nblk);
    std::vector<u64> sizes((size_t)nblk), coded((size_t)nblk);
    BWTS_TRY(crc_impl(ctx, d_in, n, segs, crcs.data()));
    // a stage reads `from` and writes `to`; the two blocks swap behind it
    u8 *to = nullptr, *other = nullptr;
    BWTS_TRY(pack_stage(ctx, 0, n, &to));
    BWTS_TRY(pack_stage(ctx, 1, n, &other));
    const u8 *from = d_in;
    auto done = [&] { from = to; std::swap(to, other); return hipStreamSynchronize(ctx->stream); };
    if (planes) {
        // every block split on its own; the checksums above are the original bytes'
        BWTS_TRY(planes_impl(ctx, from, n, width, to, false, segs));
        HIPC(done());
    }
    BWTS_TRY(seg ? forward_segments_impl(ctx, from, n, to) : forward_device_impl(ctx, from, n, to));
    HIPC(done());
    BWTS_TRY(mtf_impl(ctx, from, n, to, false, segs));
    HIPC(done());
    u64 m = n;
    if (zrl) {
        // the ranks' coded bytes, one block's behind the other's: the coder's segments
        BWTS_TRY(zrl_encode_impl(ctx, from, n, to, n, segs, coded.data()));
        HIPC(done());
        BWTS_TRY(pack_coded_set(ctx, coded, &m));
        if (seg) segs = seg_mode(ctx);
    }
    // the streams go straight to their place; a frame that does not fit is refused by the coder before it writes anything
    BWTS_TRY(ec_encode_impl(ctx, from, m, d_out + fixed, out_cap - fixed, segs, sizes.data()));
    HIPC(hipStreamSynchronize(ctx->stream));
    u8 *head = (u8 *)(ctx->h_small + SM_PACK_HEAD), *dir = nullptr;
    std::vector<u8> own;
    BWTS_TRY(pack_dir_staging(ctx, version, nblk, own, &dir));
    u64 total = fixed;
    for (u64 k = 0; k < nblk; k++) {
        if (planes) pack_entry_write_v3(dir + entry * k, sizes[(size_t)k], crcs[(size_t)k], coded[(size_t)k], width);
        else if (zrl) pack_entry_write_v2(dir + entry * k, sizes[(size_t)k], crcs[(size_t)k], coded[(size_t)k]);
        else pack_entry_write(dir + entry * k, sizes[(size_t)k], crcs[(size_t)k]);
        total += sizes[(size_t)k];
    }
    if (total > out_cap) return BWTS_E_INTERNAL;
    pack_header_write_v(head, version, n, B, dir);
    HIPC(hipMemcpyAsync(d_out + PACK_HEADER_BYTES, dir, entry * nblk, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(d_out, head, PACK_HEADER_BYTES, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    *out_bytes = total;
    return BWTS_OK;
}

// is any block split at all?  (none in versions 1 and 2, whose list of widths is empty, nor where every member has width 1)
static bool widths_split(const std::vector<u32> &widths)
{
    for (u32 w : widths) if (w != 1u) return true;
    return false;
}

// is any block filtered?  (none outside a version-2 member frame, whose list alone is not empty)
static bool filters_named(const std::vector<u32> &filters)
{
    for (u32 f : filters) if (f != DELTA_FILTER_NONE) return true;
    return false;
}

// the delta filter (delta.hip) over blocks of `total` bytes in all: one block through the single-input stage, several in one launch
// per sweep at the widths and filters given
static int frame_delta(bwts_ctx *ctx, const u8 *from, u64 total, const std::vector<u32> &widths, const std::vector<u32> &filters, u8 *to, bool decode,
                       SegMode segs)
{
    if (!segs.table()) return delta_impl(ctx, from, total, widths[0], to, decode);
    return delta_f_impl(ctx, from, total, widths.data(), filters.data(), to, decode);
}

// A member frame: pack_device_impl's chain over members of any lengths, each filtered if asked (filters: null for none) and split at
// its own width (1: not at all), with the entries and the header of include/bwts_members.h.  One member goes through the single-input
// stages.  A pack in which no member names a filter writes the version-1 frame.
int pack_members_device_impl(bwts_ctx *ctx, const u8 *d_in, const u64 *lengths, const u32 *widths, const u32 *filters, u64 count, u64 n, u8 *d_out, u64 out_cap,
                             u64 *out_bytes)
{
    const u64 fixed = members_fixed_bytes(count);
    const bool seg = count > 1;
    if (out_cap < members_least_bytes(count)) return BWTS_E_SPACE;
    std::vector<u32> ws((size_t)count, 1u);
    if (widths) ws.assign(widths, widths + count);
    std::vector<u32> fs((size_t)count, DELTA_FILTER_NONE);
    if (filters) fs.assign(filters, filters + count);
    const bool delta = filters_named(fs);
    auto members_set = [&] { u64 total = 0; return seg ? seg_table_set(ctx, lengths, count, &total) : BWTS_OK; };
    BWTS_TRY(members_set());
    SegMode segs = seg ? seg_mode(ctx) : SEG_SINGLE;
    std::vector<u32> crcs((size_t)count);
    std::vector<u64> sizes((size_t)count), coded((size_t)count);
    BWTS_TRY(crc_impl(ctx, d_in, n, segs, crcs.data()));
    u8 *to = nullptr, *other = nullptr;
    BWTS_TRY(pack_stage(ctx, 0, n, &to));
    BWTS_TRY(pack_stage(ctx, 1, n, &other));
    const u8 *from = d_in;
    auto done = [&] { from = to; std::swap(to, other); return hipStreamSynchronize(ctx->stream); };
    if (delta) {
        // every filtered member on its own; the checksums above are the original bytes'
        BWTS_TRY(frame_delta(ctx, from, n, ws, fs, to, false, segs));
        HIPC(done());
    }
    if (widths_split(ws)) {
        bool alike = true;
        for (u32 w : ws) alike = alike && w == ws[0];
        BWTS_TRY(alike ? planes_impl(ctx, from, n, ws[0], to, false, segs) : planes_w_impl(ctx, from, n, ws.data(), to, false));
        HIPC(done());
    }
    BWTS_TRY(seg ? forward_segments_impl(ctx, from, n, to) : forward_device_impl(ctx, from, n, to));
    HIPC(done());
    BWTS_TRY(mtf_impl(ctx, from, n, to, false, segs));
    HIPC(done());
    BWTS_TRY(zrl_encode_impl(ctx, from, n, to, n, segs, coded.data()));
    HIPC(done());
    u64 m = 0;
    BWTS_TRY(pack_coded_set(ctx, coded, &m));
    if (seg) segs = seg_mode(ctx);
    BWTS_TRY(ec_encode_impl(ctx, from, m, d_out + fixed, out_cap - fixed, segs, sizes.data()));
    HIPC(hipStreamSynchronize(ctx->stream));
    u8 *head = (u8 *)(ctx->h_small + SM_PACK_HEAD), *dir = nullptr;
    std::vector<u8> own;
    BWTS_TRY(pack_dir_staging(ctx, PACK_VERSION_3, count, own, &dir));
    u64 total = fixed;
    for (u64 k = 0; k < count; k++) {
        members_entry_write(dir + (u64)MEMBERS_ENTRY_BYTES * k, sizes[(size_t)k], crcs[(size_t)k], delta_word(ws[(size_t)k], fs[(size_t)k]), coded[(size_t)k], lengths[k]);
        total += sizes[(size_t)k];
    }
    if (total > out_cap) return BWTS_E_INTERNAL;
    members_header_write_v(head, delta ? MEMBERS_VERSION_2 : MEMBERS_VERSION, n, count, dir);
    HIPC(hipMemcpyAsync(d_out + MEMBERS_HEADER_BYTES, dir, (u64)MEMBERS_ENTRY_BYTES * count, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(d_out, head, MEMBERS_HEADER_BYTES, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    *out_bytes = total;
    return BWTS_OK;
}

// The frame is not trusted: header, then directory, are brought to the host and judged by the predicates of pack_plan.h before
// anything is made of them; the coder and the zero-run decoder judge their inputs themselves.
// What both unpacks know of a frame before a stream is touched.  The segment table is the frame's blocks when this returns; dir is
// staging that the next stage writes over (seg_layout.h): what the directory says is copied out at once.
// A member frame ("BWTM", include/bwts_members.h) is carried as a version-3 frame whose blocks are the members: H.nblk members,
// H.B unused, every block with a length and a width of its own.
struct FrameHead {
    PackHeader H;
    std::vector<u8> own;
    u8 *dir;
    u64 fixed, entry;
    bool members = false;
    std::vector<u64> off;       // members: where every member begins in the concatenation (count + 1)
    u64 len_at(u64 k) const { return members ? off[(size_t)k + 1] - off[(size_t)k] : pack_block_at(H.n, H.B, k); }
    u32 width_at(u64 k) const { return members ? members_entry_width(dir, k) : H.width; }
    u32 filter_at(u64 k) const { return members ? members_entry_filter(dir, k) : DELTA_FILTER_NONE; }
};

// the blocks of a judged frame as the segment table of the stages
static int frame_blocks_set(bwts_ctx *ctx, const FrameHead &F)
{
    if (!F.members) return pack_blocks_set(ctx, F.H.n, F.H.B, F.H.nblk);
    if (F.H.nblk == 1) return BWTS_OK;
    std::vector<u64> lengths((size_t)F.H.nblk);
    for (u64 k = 0; k < F.H.nblk; k++) lengths[(size_t)k] = F.len_at(k);
    u64 total = 0;
    BWTS_TRY(seg_table_set(ctx, lengths.data(), F.H.nblk, &total));
    return total == F.H.n ? BWTS_OK : BWTS_E_INTERNAL;
}

// the join behind the inverse transform: blocks of `total` bytes in all at the widths given (one block, or all widths alike: the
// uniform kernels; else one launch at mixed widths)
static int frame_join(bwts_ctx *ctx, const u8 *from, u64 total, const std::vector<u32> &widths, u8 *to, SegMode segs)
{
    bool alike = true;
    for (u32 w : widths) alike = alike && w == widths[0];
    if (alike) return planes_impl(ctx, from, total, widths[0], to, true, segs);
    return planes_w_impl(ctx, from, total, widths.data(), to, true);
}

static int unpack_members_head(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, const u8 *head, FrameHead &F)
{
    MembersHeader M;
    BWTS_TRY(members_header_check(head, in_bytes, &M));
    F.members = true;
    F.H = PackHeader{M.n, 0, M.count, M.dir_crc, PACK_VERSION_3, 0u};      // (either version of the member frame)
    F.fixed = members_fixed_bytes(M.count);
    F.entry = MEMBERS_ENTRY_BYTES;
    BWTS_TRY(pack_dir_staging(ctx, PACK_VERSION_3, M.count, F.own, &F.dir));
    if (M.count > 1) {
        HIPC(hipMemcpyAsync(F.dir, d_in + MEMBERS_HEADER_BYTES, F.entry * M.count, hipMemcpyDeviceToHost, ctx->stream));
        HIPC(hipStreamSynchronize(ctx->stream));
    }
    u64 frame = 0;
    BWTS_TRY(members_directory_check(F.dir, M, in_bytes, true, &frame));
    F.off = members_offsets(F.dir, M.count);
    if (M.count == 1) {
        // (the small block is the stages' too: the one entry is kept here)
        F.own.assign(F.dir, F.dir + MEMBERS_ENTRY_BYTES);
        F.dir = F.own.data();
    }
    return frame_blocks_set(ctx, F);
}

static int unpack_frame_head(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, FrameHead &F)
{
    if (in_bytes < PACK_LEAST_FRAME || (in_bytes & 15u)) return BWTS_E_FORMAT;
    u8 *head = (u8 *)(ctx->h_small + SM_PACK_HEAD);
    const u64 first = in_bytes < PACK_HEADER_BYTES + PACK_ENTRY_BYTES_V2 ? in_bytes : PACK_HEADER_BYTES + PACK_ENTRY_BYTES_V2;
    HIPC(hipMemcpyAsync(head, d_in, first, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    if (members_magic(head)) return unpack_members_head(ctx, d_in, in_bytes, head, F);
    PackHeader &H = F.H;
    BWTS_TRY(pack_header_check(head, in_bytes, &H));
    F.fixed = pack_fixed_bytes_v(H.version, H.nblk);
    F.entry = pack_entry_bytes(H.version);
    BWTS_TRY(pack_blocks_set(ctx, H.n, H.B, H.nblk));
    BWTS_TRY(pack_dir_staging(ctx, H.version, H.nblk, F.own, &F.dir));
    if (H.nblk > 1) {
        HIPC(hipMemcpyAsync(F.dir, d_in + PACK_HEADER_BYTES, F.entry * H.nblk, hipMemcpyDeviceToHost, ctx->stream));
        HIPC(hipStreamSynchronize(ctx->stream));
    }
    u64 frame = 0;
    return pack_directory_check(F.dir, H, in_bytes, true, &frame);
}

int unpack_device_impl(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, u8 *d_out, u64 out_cap, u64 *n_out)
{
    FrameHead F;
    BWTS_TRY(unpack_frame_head(ctx, d_in, in_bytes, F));
    const PackHeader &H = F.H;
    const u8 *dir = F.dir;
    std::vector<u32> widths, filters;
    if (H.version == PACK_VERSION_3)
        for (u64 k = 0; k < H.nblk; k++) { widths.push_back(F.width_at(k)); filters.push_back(F.filter_at(k)); }
    const bool seg = H.nblk > 1, zrl = H.version != PACK_VERSION, planes = widths_split(widths), delta = filters_named(filters);
    const u64 fixed = F.fixed, entry = F.entry;
    const SegMode segs = seg ? seg_mode(ctx) : SEG_SINGLE;
    if (H.n > out_cap) return BWTS_E_SPACE;
    ctx->tm.n = H.n;
    // (the staging is the next stage's: what the directory says is kept here)
    std::vector<u64> sizes((size_t)H.nblk), coded((size_t)H.nblk);
    std::vector<u32> want((size_t)H.nblk), got((size_t)H.nblk);
    for (u64 k = 0; k < H.nblk; k++) {
        sizes[(size_t)k] = pack_le64(dir + entry * k);
        want[(size_t)k] = ec_le32(dir + entry * k + 8);
        coded[(size_t)k] = zrl ? pack_le64(dir + entry * k + 16) : F.len_at(k);
    }
    // The stages go to and fro between d_out and the stage block, and the last one lands in d_out.  Version 1, three stages: ranks
    // into d_out, bytes of the transform into the block, the input's bytes into d_out.  Version 2, four: the ranks' coded bytes into
    // the block first.  Version 3, five: the coded bytes into d_out first (they are no more than the H.n bytes it holds), the ranks
    // into the block, and at the end the join from the block into d_out.  A member frame with filters has the delta decode behind the
    // join (or in its place): one stage more, and the first one writes the other buffer.
    u8 *block = nullptr;
    BWTS_TRY(pack_stage(ctx, 0, H.n, &block));
    const bool odd = (3 + zrl + planes + delta) % 2 != 0;        // an odd number of stages: the first one writes d_out
    u8 *to = odd ? d_out : block, *other = odd ? block : d_out;
    const u8 *from = nullptr;
    auto done = [&] { from = to; std::swap(to, other); return hipStreamSynchronize(ctx->stream); };
    u64 m = H.n;
    SegMode csegs = segs;
    if (zrl) {
        BWTS_TRY(pack_coded_set(ctx, coded, &m));
        if (seg) csegs = seg_mode(ctx);
    }
    if (seg) {
        BWTS_TRY(ec_decode_impl(ctx, d_in + fixed, m, to, m, nullptr, csegs, sizes.data()));
    } else {
        u64 named = 0;
        const int rc = ec_decode_impl(ctx, d_in + fixed, sizes[0], to, m, &named, csegs, nullptr);
        // (room for the bytes the directory names is what the coder was given: a stream that names more, or less, is not this frame's)
        if (rc == BWTS_E_SPACE || (rc == BWTS_OK && named != m)) return BWTS_E_FORMAT;
        BWTS_TRY(rc);
    }
    from = to; std::swap(to, other);
    if (zrl) {
        HIPC(hipStreamSynchronize(ctx->stream));
        ctx->tm.n = H.n;        // (the coder has put its own n there: the coded bytes)
        BWTS_TRY(frame_blocks_set(ctx, F));
        BWTS_TRY(zrl_decode_impl(ctx, from, m, to, H.n, segs, coded.data()));
        HIPC(done());
    }
    BWTS_TRY(mtf_impl(ctx, from, H.n, to, true, segs));
    HIPC(done());
    BWTS_TRY(seg ? inverse_segments_impl(ctx, from, H.n, to) : inverse_device_impl(ctx, from, H.n, to));
    HIPC(done());
    if (planes) {
        BWTS_TRY(frame_join(ctx, from, H.n, widths, to, segs));
        HIPC(done());
    }
    if (delta) {
        BWTS_TRY(frame_delta(ctx, from, H.n, widths, filters, to, true, segs));
        HIPC(done());
    }
    if (from != d_out) return BWTS_E_INTERNAL;
    BWTS_TRY(crc_impl(ctx, d_out, H.n, segs, got.data()));
    if (memcmp(got.data(), want.data(), (size_t)H.nblk * sizeof(u32)) != 0) return BWTS_E_CHECKSUM;
    *n_out = H.n;
    return BWTS_OK;
}

// Ranges of a frame (include/bwts_pack.h, "Ranges"): the frame is judged as above, then the ranges; the plan of pack_plan.h names the
// covered blocks, and only their streams are decoded, through the same stages over a segment table of the covered blocks alone.  The
// bytes go to and fro between the two stage blocks (neither is d_out here); the covered blocks' checksums are held against the
// directory, and only then are the ranges cut out of the last stage's block into d_out.
enum { RG_GATHER = 1, RG_DECODE = 2, RG_ZRL = 4, RG_MTF = 8, RG_INVERSE = 16, RG_JOIN = 32, RG_CRC = 64, RG_CUT = 128, RG_DELTA = 256 };

int unpack_ranges_device_impl(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, bool packed, const PackRange *ranges, u64 count, u8 *d_out, u64 out_cap, u64 *out_bytes,
                              const u64 *indices)
{
    u64 *rep = ctx->ranges_report;
    memset(rep, 0, sizeof ctx->ranges_report);
    FrameHead F;
    BWTS_TRY(unpack_frame_head(ctx, d_in, in_bytes, F));
    const PackHeader &H = F.H;
    const bool zrl = H.version != PACK_VERSION;
    u64 sum = 0;
    // whole members as ranges (bwts_unpack_members_device): a member frame alone has them
    std::vector<PackRange> whole;
    if (indices) {
        if (!F.members) return BWTS_E_FORMAT;
        BWTS_TRY(members_index_ranges(F.off, indices, count, &whole));
        ranges = whole.data();
    }
    BWTS_TRY(pack_ranges_check(H, ranges, count, out_cap, &sum));
    PackRangesPlan P;
    if (F.members) members_ranges_plan(F.off, F.dir, ranges, count, &P);
    else pack_ranges_plan(H, F.dir, ranges, count, &P);
    const u64 C = P.covered_bytes, nb = P.blocks.size();
    const bool seg = nb > 1, gather = !packed && P.runs.size() > 1;
    // (the staging is the next stage's: what the directory says of the covered blocks is kept here)
    std::vector<u64> lengths((size_t)nb), sizes((size_t)nb), coded((size_t)nb);
    std::vector<u32> want((size_t)nb), got((size_t)nb), widths, filters;
    for (u64 k = 0; k < nb; k++) {
        const u8 *e = F.dir + F.entry * P.blocks[(size_t)k];
        lengths[(size_t)k] = F.len_at(P.blocks[(size_t)k]);
        if (H.version == PACK_VERSION_3) { widths.push_back(F.width_at(P.blocks[(size_t)k])); filters.push_back(F.filter_at(P.blocks[(size_t)k])); }
        sizes[(size_t)k] = pack_le64(e);
        want[(size_t)k] = ec_le32(e + 8);
        coded[(size_t)k] = zrl ? pack_le64(e + 16) : lengths[(size_t)k];
    }
    ctx->tm.n = C;
    rep[0] = nb; rep[1] = P.runs.size(); rep[2] = C; rep[3] = P.stream_bytes; rep[4] = gather; rep[5] = P.out.size(); rep[7] = !seg;
    // one covered block: no table, the single-input stages, as a frame of one block
    auto blocks_set = [&] { u64 total = 0; return seg ? seg_table_set(ctx, lengths.data(), nb, &total) : BWTS_OK; };
    BWTS_TRY(blocks_set());
    const SegMode segs = seg ? seg_mode(ctx) : SEG_SINGLE;
    // the stage blocks hold the covered bytes, and the gathered streams where there are any (a stream may be longer than its block)
    const u64 room = gather && P.stream_bytes > C ? P.stream_bytes : C;
    u8 *to = nullptr, *other = nullptr;
    BWTS_TRY(pack_stage(ctx, 0, room, &to));
    BWTS_TRY(pack_stage(ctx, 1, room, &other));
    // the covered streams, back to back: behind the directory (host form), gathered, or where the one run lies in the frame
    const u8 *from = packed ? d_in + F.fixed : d_in + P.streams[0].src;
    auto done = [&](u64 bit) { rep[6] |= bit; from = to; std::swap(to, other); return hipStreamSynchronize(ctx->stream); };
    if (gather) {
        BWTS_TRY(copy_pieces_impl(ctx, d_in, in_bytes, P.streams.data(), P.streams.size(), to));
        HIPC(done(RG_GATHER));
    }
    u64 m = C;
    SegMode csegs = segs;
    if (zrl) {
        BWTS_TRY(pack_coded_set(ctx, coded, &m));
        if (seg) csegs = seg_mode(ctx);
    }
    if (seg) {
        BWTS_TRY(ec_decode_impl(ctx, from, m, to, m, nullptr, csegs, sizes.data()));
    } else {
        u64 named = 0;
        const int rc = ec_decode_impl(ctx, from, sizes[0], to, m, &named, csegs, nullptr);
        if (rc == BWTS_E_SPACE || (rc == BWTS_OK && named != m)) return BWTS_E_FORMAT;
        BWTS_TRY(rc);
    }
    HIPC(done(RG_DECODE));
    ctx->tm.n = C;        // (the coder has put its own n there)
    if (zrl) {
        BWTS_TRY(blocks_set());
        BWTS_TRY(zrl_decode_impl(ctx, from, m, to, C, segs, coded.data()));
        HIPC(done(RG_ZRL));
    }
    BWTS_TRY(mtf_impl(ctx, from, C, to, true, segs));
    HIPC(done(RG_MTF));
    BWTS_TRY(seg ? inverse_segments_impl(ctx, from, C, to) : inverse_device_impl(ctx, from, C, to));
    HIPC(done(RG_INVERSE));
    if (widths_split(widths)) {
        BWTS_TRY(frame_join(ctx, from, C, widths, to, segs));
        HIPC(done(RG_JOIN));
    }
    if (filters_named(filters)) {
        // a touched member is decoded whole, filter included
        BWTS_TRY(frame_delta(ctx, from, C, widths, filters, to, true, segs));
        HIPC(done(RG_DELTA));
    }
    BWTS_TRY(crc_impl(ctx, from, C, segs, got.data()));
    rep[6] |= RG_CRC;
    if (memcmp(got.data(), want.data(), (size_t)nb * sizeof(u32)) != 0) return BWTS_E_CHECKSUM;
    BWTS_TRY(copy_pieces_impl(ctx, from, C, P.out.data(), P.out.size(), d_out));
    rep[6] |= RG_CUT;
    *out_bytes = sum;
    return BWTS_OK;
}
