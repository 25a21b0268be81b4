// pack.hip -- the packed frames as one call each way (include/bwts_pack.h, include/bwts_members.h).  No kernel of its own: the stages
// are the ones behind the single calls, run one after the other inside one call bracket; the frames' arithmetic, the checks of an
// untrusted frame and the plan of a range read are in pack_plan.h and members_plan.h.
//
// Two chains, each written once:
//   encode_chain: crc, (delta), (split), transform, move-to-front, (zero-run coding), coder.  pack_device_impl ("BWTZ", versions 1 to
//     3) and pack_members_device_impl ("BWTM") say in an EncodeSet what the blocks are and which stages apply to them, and write their
//     own directory entries and header around the streams.
//   decode_chain: coder, (zero-run decoding), inverse move-to-front, inverse transform, (join), (delta), crc compare.  The reader
//     judges the frame into a Frame (members_plan.h); unpack_device_impl runs the chain over all its blocks, unpack_ranges_device_impl
//     over the blocks its ranges touch, and cuts the ranges out with pieces.hip's copy kernel.
//
// One block goes through the single-input stages, several through the segment forms (the bytes are the same by the segment forms'
// contract).  The stages share the context's arena, and the segment forms the pinned staging of their tables: the stream is drained
// between two stages, so that no table copy of the stage before is still to come when the next stage writes its own (seg_layout.h:
// the regions, and who overlaps whom).  The context's table changes hands inside a chain: the coder's segments are the blocks'
// zero-run coded bytes where that stage runs, every other stage's the blocks themselves.
// bwts_pack_members_a* leave filters and methods to the pack: the estimator (estimate.hip) in front of the chain resolves the filters,
// and encode_candidates, a second arrangement of the same stages, encodes the members whose method is open both ways.
// A member of a version-3 member frame may skip the middle of either chain (its method, include/bwts_members.h): such direct members
// go from the split straight to the coder, every plane of a long one as a coder segment of its own (members_plan.h: the cut rule).
// The chain stages then run over the chain members alone, gathered to the front of a stage block with pieces.hip's copy kernel, and
// the coder runs once over all coder segments in member order; where either set is empty nothing is gathered and the calls are those
// of the other kind alone.
// Header and directory travel through pinned memory too: the small block, and for several blocks the directory region behind the
// segment table (16-byte entries, "BWTZ" version 1; the 32-byte entries do not fit that region and travel through a host block of the
// call's own).  Either is staging that the next stage writes over: a Frame holds everything the directory says.
// The bytes between two stages go to and fro between two blocks; in a whole unpack one of the two is d_out, and the first stage
// writes the one that makes the last stage land in d_out (decode_stages).
#include "internal.h"
#include "members_plan.h"
#include "estimate_plan.h"
#include "../../include/bwts_members.h"

#include <string.h>
#include <utility>

static_assert(MEMBERS_METHOD_CHAIN == BWTS_METHOD_CHAIN && MEMBERS_METHOD_ORDER0 == BWTS_METHOD_ORDER0, "members_plan.h names the header's methods");
static_assert(PACK_OK == BWTS_OK && PACK_RANGE == BWTS_E_RANGE && PACK_FORMAT == BWTS_E_FORMAT && PACK_ARG == BWTS_E_ARG && PACK_SPACE == BWTS_E_SPACE,
              "pack_plan.h answers in the library's codes");

// the n-byte block between two stages
static int pack_stage(bwts_ctx *ctx, int i, u64 n, u8 **p)
{
    BWTS_TRY(kept_grow(ctx, ctx->kept[KB_PACK + i], n, 1 << 16, -1));
    *p = (u8 *)ctx->kept[KB_PACK + i].p;
    return BWTS_OK;
}

// blocks of n bytes in all as the segment table of the stages; one block: no table, the single-input stages
static int blocks_set(bwts_ctx *ctx, const std::vector<u64> &lengths, u64 n)
{
    if (lengths.size() == 1) return BWTS_OK;
    u64 total = 0;
    BWTS_TRY(seg_table_set(ctx, lengths.data(), lengths.size(), &total));
    return total == n ? BWTS_OK : BWTS_E_INTERNAL;
}

// the coder's segments where the zero-run stage runs: the blocks' coded bytes
static int pack_coded_set(bwts_ctx *ctx, const std::vector<u64> &coded, u64 *total)
{
    if (coded.size() == 1) { *total = coded[0]; return BWTS_OK; }
    return seg_table_set(ctx, coded.data(), coded.size(), total);
}

// the blocks of a "BWTZ" frame: all B long but the last
static std::vector<u64> uniform_lengths(u64 n, u64 B)
{
    std::vector<u64> lengths((size_t)pack_blocks(n, B), B);
    lengths.back() = pack_block_at(n, B, lengths.size() - 1);
    return lengths;
}

// room on the host for a directory of nblk entries: the small block behind the header, or for several blocks the directory region
// behind the segment table (pinned; 16-byte entries, and the table is nblk segments when this is called) or `own` (32-byte entries,
// and behind them the ext words of a member frame's extension table, with which one block's directory goes there too)
static int pack_dir_staging(bwts_ctx *ctx, u64 entry, u64 nblk, u64 ext, std::vector<u8> &own, u8 **dir)
{
    if (nblk == 1 && ext == 0) { *dir = (u8 *)(ctx->h_small + SM_PACK_HEAD) + PACK_HEADER_BYTES; return BWTS_OK; }
    if (entry != PACK_ENTRY_BYTES) {
        own.resize((size_t)(entry * nblk + 8u * ext));
        *dir = own.data();
        return BWTS_OK;
    }
    return seg_pinned_region(ctx, seg_dir_at(nblk), seg_dir_words(nblk), (void **)dir);
}

// split or join (planes.hip) of blocks of `total` bytes in all at the widths given: one block, or all widths alike, through the
// uniform kernels; else one launch at mixed widths
static int frame_planes(bwts_ctx *ctx, const u8 *from, u64 total, const std::vector<u32> &widths, u8 *to, bool join, SegMode segs)
{
    bool alike = true;
    for (u32 w : widths) alike = alike && w == widths[0];
    if (alike) return planes_impl(ctx, from, total, widths[0], to, join, segs);
    return planes_w_impl(ctx, from, total, widths.data(), to, join);
}

// the delta filter (delta.hip) likewise: one block through the single-input stage, several in one launch per sweep
static int frame_delta(bwts_ctx *ctx, const u8 *from, u64 total, const std::vector<u32> &widths, const std::vector<u32> &filters, u8 *to, bool decode,
                       SegMode segs)
{
    if (!segs.table()) return delta_impl(ctx, from, total, widths[0], to, decode);
    return delta_f_impl(ctx, from, total, widths.data(), filters.data(), to, decode);
}

static bool any_split(const std::vector<u32> &widths)
{
    for (u32 w : widths) if (w != 1u) return true;
    return false;
}

static bool any_filter(const std::vector<u32> &filters)
{
    for (u32 f : filters) if (f != DELTA_FILTER_NONE) return true;
    return false;
}

// ---- the two sets of a call whose blocks name methods ----
// The chain set (method 0) and the direct set (method 1) of the blocks of a call, and the coder's segments over both, in block order:
// a chain block's one segment is its (zero-run) coded bytes, a direct block's segments are its split bytes by the cut rule.
struct MethodSets {
    size_t chain = 0, direct = 0;               // blocks of either set
    u64 chain_bytes = 0, direct_bytes = 0;      // their bytes
    std::vector<u64> chain_lengths;             // the chain set's segment table
    std::vector<u32> segs;                      // per block: its coder segments
    bool mixed() const { return chain && direct; }
};
static bool is_direct(const std::vector<u32> &methods, size_t k) { return !methods.empty() && methods[k] == MEMBERS_METHOD_ORDER0; }
static MethodSets method_sets(const std::vector<u64> &lengths, const std::vector<u32> &widths, const std::vector<u32> &methods)
{
    MethodSets M;
    M.segs.assign(lengths.size(), 1u);
    for (size_t k = 0; k < lengths.size(); k++) {
        if (is_direct(methods, k)) {
            M.direct++; M.direct_bytes += lengths[k];
            M.segs[k] = members_direct_segments(lengths[k], widths[k]);
        } else {
            M.chain++; M.chain_bytes += lengths[k];
            M.chain_lengths.push_back(lengths[k]);
        }
    }
    return M;
}
// The coder's segment lengths: `coded` per chain block, the cut rule's per direct block.
static std::vector<u64> coder_lengths(const MethodSets &M, const std::vector<u64> &lengths, const std::vector<u32> &widths, const std::vector<u32> &methods,
                                      const std::vector<u64> &coded)
{
    std::vector<u64> cl;
    for (size_t k = 0; k < lengths.size(); k++) {
        if (!is_direct(methods, k)) { cl.push_back(coded[k]); continue; }
        for (u32 i = 0; i < M.segs[k]; i++) cl.push_back(members_direct_segment_bytes(lengths[k], widths[k], i));
    }
    return cl;
}
// The pieces that regroup a buffer of blocks in order (sizes `in_order`: chain blocks at their coded or plain size, direct blocks at
// their length) into the chain blocks back to back from 0 and the direct blocks back to back from `direct_at`; neighbouring blocks of
// one set are one piece.  back: the other way round.  At most one piece per block: 2^20, what pieces.hip takes.
static std::vector<PackPiece> regroup_pieces(const std::vector<u32> &methods, const std::vector<u64> &in_order, u64 direct_at, bool back)
{
    std::vector<PackPiece> ps;
    u64 at = 0, chain_at = 0, dir_at = direct_at;
    for (size_t k = 0; k < in_order.size(); k++) {
        const bool d = is_direct(methods, k);
        u64 &set_at = d ? dir_at : chain_at;
        if (k > 0 && is_direct(methods, k - 1) == d) ps.back().bytes += in_order[k];
        else ps.push_back(back ? PackPiece{set_at, at, in_order[k]} : PackPiece{at, set_at, in_order[k]});
        at += in_order[k];
        set_at += in_order[k];
    }
    return ps;
}
// a table of these lengths for the stages that follow (one length: none, the single-input stages)
static int table_set(bwts_ctx *ctx, const std::vector<u64> &lengths, SegMode *segs)
{
    *segs = SEG_SINGLE;
    if (lengths.size() == 1) return BWTS_OK;
    u64 total = 0;
    BWTS_TRY(seg_table_set(ctx, lengths.data(), lengths.size(), &total));
    *segs = seg_mode(ctx);
    return BWTS_OK;
}

// ---- encoding ----
// What a pack is asked for: the blocks, each with its width (1: not split) and filter, whether the zero-run stage runs, and the room
// the frame needs at least (`fixed` of it header and directory).
struct EncodeSet {
    std::vector<u64> lengths;
    std::vector<u32> widths, filters;
    bool zrl;
    u64 n, fixed, least;
    std::vector<u32> methods;           // empty: every block through the whole chain
};
struct Encoded {
    std::vector<u64> sizes, coded;      // per block: stream bytes; zero-run coded bytes (where that stage ran; a direct block: its length)
    std::vector<u32> crcs;
    std::vector<u64> seg_sizes;         // per coder segment, where a block is direct: stream bytes
};

// The middle of the encode chain where blocks are direct: the chain set's split bytes through transform, move-to-front and zero-run
// coding, the direct set's kept, and the coder's input put together in block order.  On entry `from` holds all blocks' split bytes;
// when this returns it holds the coder's input, E.coded says how much of it every block has, and the context's table is the
// coder's segments (*segs).  The two stage blocks hold n bytes each, and `from` may be the call's input, which is only read.
//   all direct: nothing moves.
//   mixed: a gather puts the chain set at [0, chain bytes) and the direct set at [chain bytes, n) of `to`; the three stages go to and
//     fro in [0, chain bytes) of both blocks and leave the coded bytes in the block that does not hold the direct set, so a plain copy
//     takes them over (they are the small side) before the second gather writes that block in block order.
static int encode_middle(bwts_ctx *ctx, const EncodeSet &S, const MethodSets &M, const u8 *&from, u8 *&to, u8 *&other, Encoded &E, u64 *m, SegMode *segs)
{
    const size_t count = S.lengths.size();
    for (size_t k = 0; k < count; k++) E.coded[k] = S.lengths[k];
    if (M.mixed()) {
        const u64 nc = M.chain_bytes;
        auto done = [&] { from = to; std::swap(to, other); return hipStreamSynchronize(ctx->stream); };
        const std::vector<PackPiece> apart = regroup_pieces(S.methods, S.lengths, nc, false);
        BWTS_TRY(copy_pieces_impl(ctx, from, S.n, apart.data(), apart.size(), to));
        HIPC(done());
        u8 *const sets = (u8 *)from;        // (a stage block: chain set, then direct set)
        SegMode cs;
        BWTS_TRY(table_set(ctx, M.chain_lengths, &cs));
        BWTS_TRY(cs.table() ? forward_segments_impl(ctx, from, nc, to) : forward_device_impl(ctx, from, nc, to));
        HIPC(done());
        BWTS_TRY(mtf_impl(ctx, from, nc, to, false, cs));
        HIPC(done());
        std::vector<u64> chain_coded(M.chain);
        BWTS_TRY(zrl_encode_impl(ctx, from, nc, to, nc, cs, chain_coded.data()));
        HIPC(done());
        u64 mc = 0;
        for (size_t k = 0, c = 0; k < count; k++)
            if (!is_direct(S.methods, k)) { E.coded[k] = chain_coded[c++]; mc += E.coded[k]; }
        HIPC(hipMemcpyAsync(sets, from, mc, hipMemcpyDeviceToDevice, ctx->stream));
        HIPC(hipStreamSynchronize(ctx->stream));
        u8 *const order = (u8 *)from;       // (the other stage block: its coded bytes are taken over)
        const std::vector<PackPiece> back = regroup_pieces(S.methods, E.coded, nc, true);
        BWTS_TRY(copy_pieces_impl(ctx, sets, S.n, back.data(), back.size(), order));
        HIPC(hipStreamSynchronize(ctx->stream));
        from = order;
    }
    const std::vector<u64> cl = coder_lengths(M, S.lengths, S.widths, S.methods, E.coded);
    *m = 0;
    for (u64 l : cl) *m += l;
    return table_set(ctx, cl, segs);
}

// From d_in to the streams behind d_out + S.fixed.  A stage reads `from` and writes `to`; the two stage blocks swap behind it.
static int encode_chain(bwts_ctx *ctx, const EncodeSet &S, const u8 *d_in, u8 *d_out, u64 out_cap, Encoded &E)
{
    const size_t count = S.lengths.size();
    const u64 n = S.n;
    const bool seg = count > 1;
    if (out_cap < S.least) return BWTS_E_SPACE;
    BWTS_TRY(blocks_set(ctx, S.lengths, n));
    const SegMode segs = seg ? seg_mode(ctx) : SEG_SINGLE;       // (of the blocks, and of their coded bytes: as many segments)
    E.crcs.resize(count); E.sizes.resize(count); E.coded.resize(count);
    BWTS_TRY(crc_impl(ctx, d_in, n, segs, E.crcs.data()));
    u8 *to = nullptr, *other = nullptr;
    BWTS_TRY(pack_stage(ctx, 0, n, &to));
    BWTS_TRY(pack_stage(ctx, 1, n, &other));
    const u8 *from = d_in;
    auto done = [&] { from = to; std::swap(to, other); return hipStreamSynchronize(ctx->stream); };
    if (any_filter(S.filters)) {
        // every filtered block on its own; the checksums above are the original bytes'
        BWTS_TRY(frame_delta(ctx, from, n, S.widths, S.filters, to, false, segs));
        HIPC(done());
    }
    if (any_split(S.widths)) {
        BWTS_TRY(frame_planes(ctx, from, n, S.widths, to, false, segs));
        HIPC(done());
    }
    const MethodSets M = method_sets(S.lengths, S.widths, S.methods);
    if (M.direct) {
        // the coder's segments are no longer the blocks: one table entry per plane of a long direct block
        u64 m = 0;
        SegMode cs;
        BWTS_TRY(encode_middle(ctx, S, M, from, to, other, E, &m, &cs));
        E.seg_sizes.resize(cs.table() ? (size_t)cs.count : 1);
        BWTS_TRY(ec_encode_impl(ctx, from, m, d_out + S.fixed, out_cap - S.fixed, cs, E.seg_sizes.data()));
        HIPC(hipStreamSynchronize(ctx->stream));
        for (size_t k = 0, at = 0; k < count; at += M.segs[k], k++) {
            E.sizes[k] = 0;
            for (u32 i = 0; i < M.segs[k]; i++) E.sizes[k] += E.seg_sizes[at + i];
        }
        ctx->tm.n = n;
        return BWTS_OK;
    }
    BWTS_TRY(seg ? forward_segments_impl(ctx, from, n, to) : forward_device_impl(ctx, from, n, to));
    HIPC(done());
    BWTS_TRY(mtf_impl(ctx, from, n, to, false, segs));
    HIPC(done());
    u64 m = n;
    if (S.zrl) {
        // the ranks' coded bytes, one block's behind the other's: the coder's segments
        BWTS_TRY(zrl_encode_impl(ctx, from, n, to, n, segs, E.coded.data()));
        HIPC(done());
        BWTS_TRY(pack_coded_set(ctx, E.coded, &m));
    }
    // the streams go straight to their place; a frame that does not fit is refused by the coder before it writes anything
    BWTS_TRY(ec_encode_impl(ctx, from, m, d_out + S.fixed, out_cap - S.fixed, segs, E.sizes.data()));
    HIPC(hipStreamSynchronize(ctx->stream));
    return BWTS_OK;
}

// where a pack writes header and directory before they go to the front of the frame
struct FrameStaging { u8 *head, *dir; std::vector<u8> own; };
static int encode_staging(bwts_ctx *ctx, u64 entry, u64 count, u64 ext, FrameStaging &T)
{
    T.head = (u8 *)(ctx->h_small + SM_PACK_HEAD);
    return pack_dir_staging(ctx, entry, count, ext, T.own, &T.dir);
}
static int encode_finish(bwts_ctx *ctx, const EncodeSet &S, const Encoded &E, const FrameStaging &T, u8 *d_out, u64 out_cap, u64 *out_bytes)
{
    u64 total = S.fixed;
    for (u64 sb : E.sizes) total += sb;
    if (total > out_cap) return BWTS_E_INTERNAL;
    HIPC(hipMemcpyAsync(d_out + PACK_HEADER_BYTES, T.dir, S.fixed - PACK_HEADER_BYTES, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(d_out, T.head, PACK_HEADER_BYTES, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    *out_bytes = total;
    return BWTS_OK;
}

// "BWTZ": blocks of B bytes; version 2 adds the zero-run stage, version 3 the split at one width from {2, 4, 8} (so it always runs)
int pack_device_impl(bwts_ctx *ctx, u32 version, u32 width, const u8 *d_in, u64 n, u64 B, u8 *d_out, u64 out_cap, u64 *out_bytes)
{
    const u64 nblk = pack_blocks(n, B), entry = pack_entry_bytes(version);
    EncodeSet S{uniform_lengths(n, B), {}, {}, version != PACK_VERSION, n, pack_fixed_bytes_v(version, nblk), pack_least_bytes_of(version, n, B), {}};
    S.widths.assign((size_t)nblk, version == PACK_VERSION_3 ? width : 1u);
    S.filters.assign((size_t)nblk, DELTA_FILTER_NONE);
    Encoded E;
    BWTS_TRY(encode_chain(ctx, S, d_in, d_out, out_cap, E));
    FrameStaging T;
    BWTS_TRY(encode_staging(ctx, entry, nblk, 0, T));
    for (size_t k = 0; k < (size_t)nblk; k++) {
        if (version == PACK_VERSION_3) pack_entry_write_v3(T.dir + entry * k, E.sizes[k], E.crcs[k], E.coded[k], width);
        else if (S.zrl) pack_entry_write_v2(T.dir + entry * k, E.sizes[k], E.crcs[k], E.coded[k]);
        else pack_entry_write(T.dir + entry * k, E.sizes[k], E.crcs[k]);
    }
    pack_header_write_v(T.head, version, n, B, T.dir);
    return encode_finish(ctx, S, E, T, d_out, out_cap, out_bytes);
}

// Entries, extension table and header of a member frame whose streams lie behind d_out + S.fixed; S.methods is empty where no member
// names a method.  E.seg_sizes: one word per member, and per stream of a member that has several.
static int members_finish(bwts_ctx *ctx, const EncodeSet &S, const Encoded &E, u64 ext, u8 *d_out, u64 out_cap, u64 *out_bytes)
{
    const u64 count = S.lengths.size();
    const bool v3 = !S.methods.empty();
    FrameStaging T;
    BWTS_TRY(encode_staging(ctx, MEMBERS_ENTRY_BYTES, count, ext, T));
    u8 *table = T.dir + (u64)MEMBERS_ENTRY_BYTES * count;
    if (ext) memset(table, 0, (size_t)(8u * ext));
    for (size_t k = 0, seg = 0; k < (size_t)count; k++) {
        const u32 method = v3 ? S.methods[k] : MEMBERS_METHOD_CHAIN, words = members_table_words(S.lengths[k], S.widths[k], method);
        members_entry_write(T.dir + (u64)MEMBERS_ENTRY_BYTES * k, E.sizes[k], E.crcs[k], members_word(S.widths[k], S.filters[k], method), E.coded[k], S.lengths[k]);
        for (u32 i = 0; i < words; i++, table += 8) pack_put64(table, E.seg_sizes[seg + i]);
        seg += words ? words : 1u;
    }
    members_header_write_x(T.head, v3 ? MEMBERS_VERSION_3 : any_filter(S.filters) ? MEMBERS_VERSION_2 : MEMBERS_VERSION, S.n, count, ext, T.dir);
    return encode_finish(ctx, S, E, T, d_out, out_cap, out_bytes);
}

// "BWTM": members of any lengths, each filtered if asked (filters: null for none) and split at its own width (widths: null for 1, not
// at all), with the entries and the header of include/bwts_members.h.  methods: null for the whole chain everywhere; a member of
// method 1 is coded directly.  A pack in which no member names a method writes version 2 where one names a filter, else version 1;
// one that does writes version 3, with the stream sizes of every member that has several in the table behind the entries.
int pack_members_device_impl(bwts_ctx *ctx, const u8 *d_in, const u64 *lengths, const u32 *widths, const u32 *filters, const u32 *methods, u64 count, u64 n,
                             u8 *d_out, u64 out_cap, u64 *out_bytes)
{
    const bool v3 = members_any_method(methods, count);
    const u64 ext = v3 ? members_ext_words(lengths, widths, methods, count) : 0;
    EncodeSet S{std::vector<u64>(lengths, lengths + count), {}, {}, true, n, members_fixed_bytes_x(count, ext),
                v3 ? members_least_bytes_m(lengths, widths, methods, count) : members_least_bytes(count), {}};
    S.widths.assign((size_t)count, 1u);
    if (widths) S.widths.assign(widths, widths + count);
    S.filters.assign((size_t)count, DELTA_FILTER_NONE);
    if (filters) S.filters.assign(filters, filters + count);
    if (v3) S.methods.assign(methods, methods + count);
    Encoded E;
    BWTS_TRY(encode_chain(ctx, S, d_in, d_out, out_cap, E));
    return members_finish(ctx, S, E, ext, d_out, out_cap, out_bytes);
}

// ---- a pack that chooses filters and methods (include/bwts_members.h, "AUTO") ----
// the pieces that gather the blocks a set names (a byte per block) from a buffer of all blocks in order to the front of another;
// neighbouring blocks are one piece
static std::vector<PackPiece> set_pieces(const std::vector<u64> &lengths, const std::vector<u8> &in_set)
{
    std::vector<PackPiece> ps;
    u64 at = 0, to = 0;
    for (size_t k = 0; k < lengths.size(); at += lengths[k], k++) {
        if (!in_set[k]) continue;
        if (!ps.empty() && ps.back().src + ps.back().bytes == at) ps.back().bytes += lengths[k];
        else ps.push_back(PackPiece{at, to, lengths[k]});
        to += lengths[k];
    }
    return ps;
}

// Both encodings of the members whose method is open, and the winners' streams to their places.  S holds the resolved filters and, in
// S.methods, what was asked (MEMBERS_AUTO among it); the direct candidates are the members that name method 1 or AUTO, the chain
// candidates those that name method 0 or AUTO, and there is one of either.  Checksum, filter and split run once over all members;
// the coder runs over the direct candidates' split bytes, then the chain stages and the coder over the chain candidates' -- both into
// the context's candidates block, which the bounds size, so that nothing is written to d_out before the frame is known to fit.  On
// return S.methods are the resolved ones (empty where none is direct), E says what members_finish needs, and *ext the table's words.
static int encode_candidates(bwts_ctx *ctx, EncodeSet &S, const u8 *d_in, u8 *d_out, u64 out_cap, Encoded &E, u64 *ext)
{
    const size_t count = S.lengths.size();
    const u64 n = S.n;
    std::vector<u8> chain(count), direct(count);
    std::vector<u64> chain_lengths, direct_lengths;         // the chain candidates; the direct candidates' coder segments
    std::vector<u32> dsegs(count, 0u);
    u64 nc = 0, nd = 0, bound_c = 0, bound_d = 0;
    size_t chains = 0, directs = 0;
    for (size_t k = 0; k < count; k++) {
        chain[k] = S.methods[k] != MEMBERS_METHOD_ORDER0;
        direct[k] = S.methods[k] != MEMBERS_METHOD_CHAIN;
        if (chain[k]) { chains++; nc += S.lengths[k]; chain_lengths.push_back(S.lengths[k]); bound_c += ec_bound_bytes(S.lengths[k]); }
        if (direct[k]) {
            directs++; nd += S.lengths[k]; bound_d += members_streams_bound(S.lengths[k], S.widths[k], MEMBERS_METHOD_ORDER0);
            dsegs[k] = members_direct_segments(S.lengths[k], S.widths[k]);
            for (u32 i = 0; i < dsegs[k]; i++) direct_lengths.push_back(members_direct_segment_bytes(S.lengths[k], S.widths[k], i));
        }
    }
    BWTS_TRY(blocks_set(ctx, S.lengths, n));
    const SegMode segs = count > 1 ? seg_mode(ctx) : SEG_SINGLE;
    E.crcs.resize(count); E.sizes.resize(count); E.coded.resize(count);
    BWTS_TRY(crc_impl(ctx, d_in, n, segs, E.crcs.data()));
    u8 *to = nullptr, *other = nullptr;
    BWTS_TRY(pack_stage(ctx, 0, n, &to));
    BWTS_TRY(pack_stage(ctx, 1, n, &other));
    const u64 direct_at = 0, chain_at = align_up(bound_d, 256), cand_bytes = chain_at + bound_c;
    BWTS_TRY(kept_grow(ctx, ctx->kept[KB_PACK + 2], cand_bytes, 1 << 16, -1));
    u8 *const cand = (u8 *)ctx->kept[KB_PACK + 2].p;
    const u8 *from = d_in;
    auto done = [&] { from = to; std::swap(to, other); return hipStreamSynchronize(ctx->stream); };
    if (any_filter(S.filters)) {
        BWTS_TRY(frame_delta(ctx, from, n, S.widths, S.filters, to, false, segs));
        HIPC(done());
    }
    if (any_split(S.widths)) {
        BWTS_TRY(frame_planes(ctx, from, n, S.widths, to, false, segs));
        HIPC(done());
    }
    // `from` holds every member's split bytes, and `to` is free.  The direct candidates: gathered there unless they are all members
    std::vector<u64> dsizes(direct_lengths.size()), csizes(chains), ccoded(chains);
    {
        const u8 *dfrom = from;
        if (directs != count) {
            const std::vector<PackPiece> ps = set_pieces(S.lengths, direct);
            BWTS_TRY(copy_pieces_impl(ctx, from, n, ps.data(), ps.size(), to));
            dfrom = to;
        }
        SegMode ds;
        BWTS_TRY(table_set(ctx, direct_lengths, &ds));
        BWTS_TRY(ec_encode_impl(ctx, dfrom, nd, cand + direct_at, bound_d, ds, dsizes.data()));
        HIPC(hipStreamSynchronize(ctx->stream));
    }
    // The chain candidates: gathered likewise, after which the split bytes are no longer needed and their block (where it is a stage
    // block: `other`) is the second one of the to and fro
    if (chains != count) {
        const std::vector<PackPiece> ps = set_pieces(S.lengths, chain);
        BWTS_TRY(copy_pieces_impl(ctx, from, n, ps.data(), ps.size(), to));
        HIPC(done());
    }
    SegMode cs;
    BWTS_TRY(table_set(ctx, chain_lengths, &cs));
    BWTS_TRY(cs.table() ? forward_segments_impl(ctx, from, nc, to) : forward_device_impl(ctx, from, nc, to));
    HIPC(done());
    BWTS_TRY(mtf_impl(ctx, from, nc, to, false, cs));
    HIPC(done());
    BWTS_TRY(zrl_encode_impl(ctx, from, nc, to, nc, cs, ccoded.data()));
    HIPC(done());
    u64 mc = 0;
    BWTS_TRY(pack_coded_set(ctx, ccoded, &mc));
    BWTS_TRY(ec_encode_impl(ctx, from, mc, cand + chain_at, bound_c, cs, csizes.data()));
    HIPC(hipStreamSynchronize(ctx->stream));
    // the choice, and where every winner's streams lie in the candidates block
    std::vector<PackPiece> win;
    std::vector<u32> resolved(count);
    bool v3 = false;
    u64 d_at = direct_at, c_at = chain_at, total = 0;
    for (size_t k = 0, di = 0, ci = 0; k < count; k++) {
        u64 dsb = 0, csb = chain[k] ? csizes[ci] : 0;
        for (u32 i = 0; i < dsegs[k]; i++) dsb += dsizes[di + i];
        u32 m = S.methods[k];
        if (m == MEMBERS_AUTO)
            m = members_method_choice(members_method_cost(csb, S.lengths[k], S.widths[k], MEMBERS_METHOD_CHAIN),
                                      members_method_cost(dsb, S.lengths[k], S.widths[k], MEMBERS_METHOD_ORDER0));
        resolved[k] = m;
        const bool d = m == MEMBERS_METHOD_ORDER0;
        v3 = v3 || d;
        E.sizes[k] = d ? dsb : csb;
        E.coded[k] = d ? S.lengths[k] : ccoded[ci];
        if (d) E.seg_sizes.insert(E.seg_sizes.end(), dsizes.begin() + (long)di, dsizes.begin() + (long)(di + dsegs[k]));
        else E.seg_sizes.push_back(csb);
        const u64 src = d ? d_at : c_at;
        if (!win.empty() && win.back().src + win.back().bytes == src) win.back().bytes += E.sizes[k];
        else win.push_back(PackPiece{src, total, E.sizes[k]});
        total += E.sizes[k];
        if (direct[k]) { d_at += dsb; di += dsegs[k]; }
        if (chain[k]) { c_at += csb; ci++; }
    }
    S.methods = resolved;
    *ext = v3 ? members_ext_words(S.lengths.data(), S.widths.data(), S.methods.data(), count) : 0;
    S.fixed = members_fixed_bytes_x(count, *ext);
    if (S.fixed + total > out_cap) return BWTS_E_SPACE;
    BWTS_TRY(copy_pieces_impl(ctx, cand, cand_bytes, win.data(), win.size(), d_out + S.fixed));
    if (!v3) S.methods.clear();
    ctx->tm.n = n;
    return BWTS_OK;
}

// lengths, widths (null: 1), filters (null: none) and methods (null: the chain), MEMBERS_AUTO among the last two, have passed
// members_args_check_a; n is the lengths' sum.  filters_out, methods_out: null, or room for the resolved values.
int pack_members_auto_device_impl(bwts_ctx *ctx, const u8 *d_in, const u64 *lengths, const u32 *widths, const u32 *filters, const u32 *methods, u64 count, u64 n,
                                  u8 *d_out, u64 out_cap, u64 *out_bytes, u32 *filters_out, u32 *methods_out)
{
    EncodeSet S{std::vector<u64>(lengths, lengths + count), {}, {}, true, n, 0, 0, {}};
    S.widths.assign((size_t)count, 1u);
    if (widths) S.widths.assign(widths, widths + count);
    S.filters.assign((size_t)count, DELTA_FILTER_NONE);
    if (filters) S.filters.assign(filters, filters + count);
    S.methods.assign((size_t)count, MEMBERS_METHOD_CHAIN);
    if (methods) S.methods.assign(methods, methods + count);
    if (members_any_auto(S.filters.data(), count)) {
        // the estimate of the members whose filter is open, and the rule of estimate_plan.h
        std::vector<u8> take((size_t)count);
        std::vector<u64> none((size_t)count), delta((size_t)count);
        for (size_t k = 0; k < (size_t)count; k++) take[k] = S.filters[k] == MEMBERS_AUTO;
        u64 total = 0;
        BWTS_TRY(seg_table_set(ctx, lengths, count, &total));
        BWTS_TRY(estimate_impl(ctx, d_in, n, S.widths.data(), take.data(), none.data(), delta.data()));
        for (size_t k = 0; k < (size_t)count; k++)
            if (take[k]) S.filters[k] = estimate_filter(none[k], delta[k]);
    }
    if (!members_any_auto(S.methods.data(), count)) {
        BWTS_TRY(pack_members_device_impl(ctx, d_in, lengths, S.widths.data(), S.filters.data(), S.methods.data(), count, n, d_out, out_cap, out_bytes));
    } else {
        Encoded E;
        u64 ext = 0;
        BWTS_TRY(encode_candidates(ctx, S, d_in, d_out, out_cap, E, &ext));
        BWTS_TRY(members_finish(ctx, S, E, ext, d_out, out_cap, out_bytes));
        if (S.methods.empty()) S.methods.assign((size_t)count, MEMBERS_METHOD_CHAIN);
    }
    for (size_t k = 0; k < (size_t)count; k++) {
        if (filters_out) filters_out[k] = S.filters[k];
        if (methods_out) methods_out[k] = S.methods[k];
    }
    return BWTS_OK;
}

// ---- decoding ----
// The frame is not trusted: header, then directory, are brought to the host and judged (frame_head_check, frame_dir_check) before
// anything is made of them; the coder and the zero-run decoder judge their inputs themselves.  The segment table is the frame's
// blocks when this returns.
static int unpack_frame_head(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, Frame &F)
{
    if (in_bytes < PACK_LEAST_FRAME || (in_bytes & 15u)) return BWTS_E_FORMAT;
    u8 *head = (u8 *)(ctx->h_small + SM_PACK_HEAD), *dir = nullptr;
    const u64 first = in_bytes < PACK_HEADER_BYTES + PACK_ENTRY_BYTES_V2 ? in_bytes : PACK_HEADER_BYTES + PACK_ENTRY_BYTES_V2;
    HIPC(hipMemcpyAsync(head, d_in, first, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    BWTS_TRY(frame_head_check(head, in_bytes, &F));
    // a "BWTZ" frame's blocks are known from the header, and the directory region lies behind their table; a member frame's blocks
    // come with the directory
    if (!F.members) BWTS_TRY(blocks_set(ctx, uniform_lengths(F.n, F.B), F.n));
    std::vector<u8> own;
    BWTS_TRY(pack_dir_staging(ctx, F.entry, F.count, F.ext, own, &dir));
    if (F.count > 1 || F.ext) {
        // (the extension table of a version-3 member frame comes with the entries: the header check has held both against in_bytes)
        HIPC(hipMemcpyAsync(dir, d_in + PACK_HEADER_BYTES, F.fixed - PACK_HEADER_BYTES, hipMemcpyDeviceToHost, ctx->stream));
        HIPC(hipStreamSynchronize(ctx->stream));
    }
    u64 frame = 0;
    BWTS_TRY(frame_dir_check(dir, F, in_bytes, true, &frame));
    if (!F.members) return BWTS_OK;
    std::vector<u64> lengths((size_t)F.count);
    for (size_t k = 0; k < lengths.size(); k++) lengths[k] = F.len(k);
    return blocks_set(ctx, lengths, F.n);
}

// The blocks of a judged frame that a call decodes: all of them, or the covered blocks of a plan.
struct DecodeSet {
    u64 total = 0;                              // the blocks' bytes
    std::vector<u64> lengths, sizes, coded;     // per block: bytes, stream bytes, coded bytes
    std::vector<u32> want, widths, filters;     // ... checksum, width, filter
    std::vector<u32> methods;                   // ... method; empty where no block is direct
    std::vector<u64> seg_sizes;                 // per coder segment, where a block is direct: stream bytes
    MethodSets M;
    bool zrl = false, split = false, delta = false;
};
static DecodeSet decode_set(const Frame &F, const std::vector<u64> *blocks)
{
    DecodeSet S;
    const size_t nb = blocks ? blocks->size() : (size_t)F.count;
    S.lengths.resize(nb); S.sizes.resize(nb); S.coded.resize(nb); S.want.resize(nb); S.widths.resize(nb); S.filters.resize(nb);
    for (size_t i = 0; i < nb; i++) {
        const size_t k = blocks ? (size_t)(*blocks)[i] : i;
        S.lengths[i] = F.len(k); S.sizes[i] = F.stream[k]; S.coded[i] = F.coded[k];
        S.want[i] = F.crc[k]; S.widths[i] = F.width[k]; S.filters[i] = F.filter[k];
        S.total += F.len(k);
    }
    S.zrl = F.zrl; S.split = any_split(S.widths); S.delta = any_filter(S.filters);
    bool direct = false;
    for (size_t i = 0; i < nb; i++) direct = direct || F.direct(blocks ? (*blocks)[i] : i);
    if (direct) {
        S.methods.resize(nb);
        for (size_t i = 0; i < nb; i++) {
            const size_t k = blocks ? (size_t)(*blocks)[i] : i;
            S.methods[i] = F.method[k];
            if (F.table_at[k + 1] == F.table_at[k]) S.seg_sizes.push_back(F.stream[k]);
            else S.seg_sizes.insert(S.seg_sizes.end(), F.table.begin() + (ptrdiff_t)F.table_at[k], F.table.begin() + (ptrdiff_t)F.table_at[k + 1]);
        }
    }
    S.M = method_sets(S.lengths, S.widths, S.methods);
    return S;
}
// how many stages write a buffer: coder, inverse move-to-front and inverse transform always; where every block is direct the coder
// alone, and in a mixed set the two gathers and the copy between them besides (decode_middle)
static int decode_stages(const DecodeSet &S)
{
    if (S.M.direct) return (S.M.chain ? 7 : 1) + S.split + S.delta;
    return 3 + S.zrl + S.split + S.delta;
}

// the stages of a range read, as the bits of its report (include/bwts_test.h)
enum { RG_GATHER = 1, RG_DECODE = 2, RG_ZRL = 4, RG_MTF = 8, RG_INVERSE = 16, RG_JOIN = 32, RG_CRC = 64, RG_CUT = 128, RG_DELTA = 256, RG_REGROUP = 512 };

static int decode_tail(bwts_ctx *ctx, const DecodeSet &S, const u8 *&from, u8 *to, u8 *other, u64 *stages);

// The front of the decode chain where blocks are direct: one coder decode over all coder segments, the cut rule's for a direct block;
// then, where chain blocks are among them, their coded bytes through zero-run decoding, inverse move-to-front and the inverse
// transform under a table of the chain set alone.  When this returns, `from` holds every block's split bytes in block order, and
// to / other are the buffers the next two stages write.  Both buffers hold S.total bytes.
//   all direct: the coder's output is that already.
//   mixed: a gather puts the chain set's coded bytes at the front and the direct set at [chain bytes, total) of the second buffer; a
//     plain copy takes the coded bytes (the small side) back to the first, so that the three stages, which go to and fro in [0, chain
//     bytes) of both, end in the buffer that holds the direct set; a second gather restores block order.  Seven writes of a buffer.
static int decode_middle(bwts_ctx *ctx, const DecodeSet &S, const u8 *&from, u8 *&to, u8 *&other, u64 *stages)
{
    const MethodSets &M = S.M;
    auto next = [&](u64 bit) { if (stages) *stages |= bit; from = to; std::swap(to, other); };
    auto done = [&](u64 bit) { next(bit); return hipStreamSynchronize(ctx->stream); };
    const std::vector<u64> cl = coder_lengths(M, S.lengths, S.widths, S.methods, S.coded);
    u64 m = 0;
    for (u64 l : cl) m += l;
    SegMode cs;
    BWTS_TRY(table_set(ctx, cl, &cs));
    if (cs.table()) {
        BWTS_TRY(ec_decode_impl(ctx, from, m, to, m, nullptr, cs, S.seg_sizes.data()));
    } else {
        u64 named = 0;
        const int rc = ec_decode_impl(ctx, from, S.seg_sizes[0], to, m, &named, cs, nullptr);
        if (rc == BWTS_E_SPACE || (rc == BWTS_OK && named != m)) return BWTS_E_FORMAT;
        BWTS_TRY(rc);
    }
    next(RG_DECODE);
    if (!M.chain) return BWTS_OK;
    const u64 nc = M.chain_bytes;
    std::vector<u64> in_order(S.lengths), chain_coded;
    u64 mc = 0;
    for (size_t k = 0; k < in_order.size(); k++)
        if (!is_direct(S.methods, k)) { in_order[k] = S.coded[k]; chain_coded.push_back(S.coded[k]); mc += S.coded[k]; }
    const std::vector<PackPiece> apart = regroup_pieces(S.methods, in_order, nc, false);
    BWTS_TRY(copy_pieces_impl(ctx, from, m, apart.data(), apart.size(), to));
    HIPC(done(RG_REGROUP));
    HIPC(hipMemcpyAsync(to, from, mc, hipMemcpyDeviceToDevice, ctx->stream));
    HIPC(done(0));
    SegMode chain;
    BWTS_TRY(table_set(ctx, M.chain_lengths, &chain));
    BWTS_TRY(zrl_decode_impl(ctx, from, mc, to, nc, chain, chain_coded.data()));
    HIPC(done(RG_ZRL));
    BWTS_TRY(mtf_impl(ctx, from, nc, to, true, chain));
    HIPC(done(RG_MTF));
    BWTS_TRY(chain.table() ? inverse_segments_impl(ctx, from, nc, to) : inverse_device_impl(ctx, from, nc, to));
    HIPC(done(RG_INVERSE));
    const std::vector<PackPiece> back = regroup_pieces(S.methods, S.lengths, nc, true);
    BWTS_TRY(copy_pieces_impl(ctx, from, S.total, back.data(), back.size(), to));
    HIPC(done(0));
    return BWTS_OK;
}

// From the streams at `from`, back to back, to the blocks' bytes with their checksums held against the directory: `from` is where
// they are when this returns.  The context's table is S's blocks on entry; the first stage writes `to`, the next one `other`, and so
// on.  stages: not null to have the bit of every stage that ran ORed in.
static int decode_chain(bwts_ctx *ctx, const DecodeSet &S, const u8 *&from, u8 *to, u8 *other, u64 *stages)
{
    const bool seg = S.lengths.size() > 1;
    const SegMode segs = seg ? seg_mode(ctx) : SEG_SINGLE;       // (of the blocks, and of their coded bytes: as many segments)
    const u64 n = S.total;
    auto next = [&](u64 bit) { if (stages) *stages |= bit; from = to; std::swap(to, other); };
    auto done = [&](u64 bit) { next(bit); return hipStreamSynchronize(ctx->stream); };
    u64 m = n;
    if (S.M.direct) {
        BWTS_TRY(decode_middle(ctx, S, from, to, other, stages));
        ctx->tm.n = n;
        BWTS_TRY(blocks_set(ctx, S.lengths, n));
        return decode_tail(ctx, S, from, to, other, stages);
    }
    if (S.zrl) BWTS_TRY(pack_coded_set(ctx, S.coded, &m));
    if (seg) {
        BWTS_TRY(ec_decode_impl(ctx, from, m, to, m, nullptr, segs, S.sizes.data()));
    } else {
        u64 named = 0;
        const int rc = ec_decode_impl(ctx, from, S.sizes[0], to, m, &named, segs, nullptr);
        // (room for the bytes the directory names is what the coder was given: a stream that names more, or less, is not this frame's)
        if (rc == BWTS_E_SPACE || (rc == BWTS_OK && named != m)) return BWTS_E_FORMAT;
        BWTS_TRY(rc);
    }
    next(RG_DECODE);        // (the coder has drained the stream itself: it reads its verdict back)
    ctx->tm.n = n;          // (... and has put its own n there: the coded bytes)
    if (S.zrl) {
        BWTS_TRY(blocks_set(ctx, S.lengths, n));
        BWTS_TRY(zrl_decode_impl(ctx, from, m, to, n, segs, S.coded.data()));
        HIPC(done(RG_ZRL));
    }
    BWTS_TRY(mtf_impl(ctx, from, n, to, true, segs));
    HIPC(done(RG_MTF));
    BWTS_TRY(seg ? inverse_segments_impl(ctx, from, n, to) : inverse_device_impl(ctx, from, n, to));
    HIPC(done(RG_INVERSE));
    return decode_tail(ctx, S, from, to, other, stages);
}

// The end of the decode chain, over all blocks of S (the context's table): join, delta decode, and the checksums against the directory.
static int decode_tail(bwts_ctx *ctx, const DecodeSet &S, const u8 *&from, u8 *to, u8 *other, u64 *stages)
{
    const SegMode segs = S.lengths.size() > 1 ? seg_mode(ctx) : SEG_SINGLE;
    const u64 n = S.total;
    auto done = [&](u64 bit) { if (stages) *stages |= bit; from = to; std::swap(to, other); return hipStreamSynchronize(ctx->stream); };
    if (S.split) {
        BWTS_TRY(frame_planes(ctx, from, n, S.widths, to, true, segs));
        HIPC(done(RG_JOIN));
    }
    if (S.delta) {
        // a touched member is decoded whole, filter included
        BWTS_TRY(frame_delta(ctx, from, n, S.widths, S.filters, to, true, segs));
        HIPC(done(RG_DELTA));
    }
    std::vector<u32> got(S.want.size());
    BWTS_TRY(crc_impl(ctx, from, n, segs, got.data()));
    if (stages) *stages |= RG_CRC;
    return got == S.want ? BWTS_OK : BWTS_E_CHECKSUM;
}

// The stages go to and fro between d_out and the stage block (d_out holds n bytes, and no stage's output is more), and the first one
// writes the buffer that makes the last one land in d_out.
int unpack_device_impl(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, u8 *d_out, u64 out_cap, u64 *n_out)
{
    Frame F;
    BWTS_TRY(unpack_frame_head(ctx, d_in, in_bytes, F));
    if (F.n > out_cap) return BWTS_E_SPACE;
    ctx->tm.n = F.n;
    const DecodeSet S = decode_set(F, nullptr);
    u8 *block = nullptr;
    BWTS_TRY(pack_stage(ctx, 0, F.n, &block));
    const bool odd = decode_stages(S) % 2 != 0;
    const u8 *from = d_in + F.fixed;
    BWTS_TRY(decode_chain(ctx, S, from, odd ? d_out : block, odd ? block : d_out, nullptr));
    if (from != d_out) return BWTS_E_INTERNAL;
    *n_out = F.n;
    return BWTS_OK;
}

// The destinations of bwts_unpack_members_p_device against the members asked for (r: one per destination): a NULL table or entry,
// then room, then two destinations that share a byte or one that overlaps the frame -- only the member's bytes of a destination count.
static int member_dsts_check(const MemberDsts &D, const PackRange *r, u64 count, const u8 *d_in, u64 in_bytes)
{
    if (!D.dsts || !D.dst_bytes) return BWTS_E_ARG;
    for (u64 j = 0; j < count; j++)
        if (!D.dsts[j]) return BWTS_E_ARG;
    for (u64 j = 0; j < count; j++)
        if (D.dst_bytes[j] < r[j].bytes) return BWTS_E_SPACE;
    std::vector<std::pair<u64, u64>> spans((size_t)count);
    for (u64 j = 0; j < count; j++) {
        if (ranges_overlap(d_in, in_bytes, D.dsts[j], r[j].bytes)) return BWTS_E_ARG;
        spans[(size_t)j] = {(u64)(uintptr_t)D.dsts[j], r[j].bytes};
    }
    return spans_disjoint(spans) ? BWTS_OK : BWTS_E_ARG;
}

// Ranges of a frame (include/bwts_pack.h, "Ranges"): the frame is judged as above, then the ranges; the plan names the covered blocks,
// and only their streams are decoded, over a segment table of the covered blocks alone.  The bytes go to and fro between the two
// stage blocks (neither is d_out here); only when the covered blocks' checksums agree are the ranges cut out of the last stage's
// block into d_out.
// With ptrs (bwts_unpack_members_p_device: whole members, each into a buffer of its own) the cut is pieces.hip's copy between scattered
// buffers, d_out is not read, and the destinations are judged behind the frame and the indices (include/bwts_members.h, "Pointers").
int unpack_ranges_device_impl(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, bool packed, const PackRange *ranges, u64 count, u8 *d_out, u64 out_cap, u64 *out_bytes,
                              const u64 *indices, const MemberDsts *ptrs)
{
    u64 *rep = ctx->ranges_report;
    memset(rep, 0, sizeof ctx->ranges_report);
    Frame F;
    BWTS_TRY(unpack_frame_head(ctx, d_in, in_bytes, F));
    u64 sum = 0;
    // whole members as ranges (bwts_unpack_members_device): a member frame alone has them
    std::vector<PackRange> whole;
    std::vector<u64> all;
    if (ptrs && !indices) {
        // every member in order: the count must be the frame's
        if (!F.members) return BWTS_E_FORMAT;
        if (count != F.count) return BWTS_E_ARG;
        all.resize((size_t)count);
        for (u64 k = 0; k < count; k++) all[(size_t)k] = k;
        indices = all.data();
    }
    if (indices) {
        if (!F.members) return BWTS_E_FORMAT;
        BWTS_TRY(members_index_ranges(F, indices, count, &whole));
        ranges = whole.data();
    }
    BWTS_TRY(pack_ranges_check(F.n, ranges, count, out_cap, &sum));
    if (ptrs) BWTS_TRY(member_dsts_check(*ptrs, ranges, count, d_in, in_bytes));
    PackRangesPlan P;
    ranges_plan(F, ranges, count, &P);
    const DecodeSet S = decode_set(F, &P.blocks);
    const u64 C = P.covered_bytes, nb = P.blocks.size();
    const bool gather = !packed && P.runs.size() > 1;
    ctx->tm.n = C;
    rep[0] = nb; rep[1] = P.runs.size(); rep[2] = C; rep[3] = P.stream_bytes; rep[4] = gather; rep[5] = P.out.size(); rep[7] = nb == 1;
    // one covered block: no table, the single-input stages, as a frame of one block
    BWTS_TRY(blocks_set(ctx, S.lengths, C));
    // the stage blocks hold the covered bytes, and the gathered streams where there are any (a stream may be longer than its block)
    const u64 room = gather && P.stream_bytes > C ? P.stream_bytes : C;
    u8 *to = nullptr, *other = nullptr;
    BWTS_TRY(pack_stage(ctx, 0, room, &to));
    BWTS_TRY(pack_stage(ctx, 1, room, &other));
    // the covered streams, back to back: behind the directory (host form), gathered, or where the one run lies in the frame
    const u8 *from = packed ? d_in + F.fixed : d_in + P.streams[0].src;
    if (gather) {
        BWTS_TRY(copy_pieces_impl(ctx, d_in, in_bytes, P.streams.data(), P.streams.size(), to));
        HIPC(hipStreamSynchronize(ctx->stream));
        rep[6] |= RG_GATHER;
        from = to;
        std::swap(to, other);
    }
    BWTS_TRY(decode_chain(ctx, S, from, to, other, &rep[6]));
    if (ptrs) {
        // (one piece per range, in the ranges' order: its place in the covered bytes to the destination that asked for it)
        std::vector<PackPiece> apart(P.out);
        for (size_t j = 0; j < apart.size(); j++) apart[j] = PackPiece{(u64)(uintptr_t)from + P.out[j].src, (u64)(uintptr_t)ptrs->dsts[j], P.out[j].bytes};
        BWTS_TRY(scatter_pieces_impl(ctx, apart.data(), apart.size()));
    } else {
        BWTS_TRY(copy_pieces_impl(ctx, from, C, P.out.data(), P.out.size(), d_out));
    }
    rep[6] |= RG_CUT;
    *out_bytes = sum;
    return BWTS_OK;
}
