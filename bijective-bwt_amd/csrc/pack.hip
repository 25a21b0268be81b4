// pack.hip -- the chain as one call (include/bwts_pack.h): checksums, transform, move-to-front and entropy coder over the blocks of
// a frame, and the way back.  No kernel of its own: the stages are the ones behind the single calls, run one after the other inside
// one call bracket; the frame's arithmetic and the checks of an untrusted frame are in pack_plan.h.
//
// A frame of one block goes through the single-input stages, one of several blocks through the segment forms (the bytes are the
// same by the segment forms' contract).  The stages share the context's arena, and the segment forms the pinned staging of their
// tables: the stream is drained between two stages, so that no table copy of the stage before is still to come when the next stage
// writes its own (seg_layout.h: the regions, and who overlaps whom).  Header and directory travel through pinned memory too: the
// small block, and for several blocks the directory region behind the segment table.
#include "internal.h"
#include "pack_plan.h"
#include "../../include/bwts_pack.h"

#include <string.h>

static_assert(PACK_OK == BWTS_OK && PACK_RANGE == BWTS_E_RANGE && PACK_FORMAT == BWTS_E_FORMAT, "pack_plan.h answers in the library's codes");

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

// pinned room for a directory of nblk entries: the small block behind the header, or the directory region behind the segment table
static int pack_dir_staging(bwts_ctx *ctx, u64 nblk, u8 **dir)
{
    if (nblk == 1) { *dir = (u8 *)(ctx->h_small + SM_PACK_HEAD) + PACK_HEADER_BYTES; return BWTS_OK; }
    return seg_pinned_region(ctx, seg_dir_at(nblk), seg_dir_words(nblk), (void **)dir);
}

int pack_device_impl(bwts_ctx *ctx, const u8 *d_in, u64 n, u64 B, u8 *d_out, u64 out_cap, u64 *out_bytes)
{
    const u64 nblk = pack_blocks(n, B), fixed = pack_fixed_bytes(nblk);
    const bool seg = nblk > 1;
    if (out_cap < pack_least_bytes(n, B)) return BWTS_E_SPACE;
    BWTS_TRY(pack_blocks_set(ctx, n, B, nblk));
    const SegMode segs = seg ? seg_mode(ctx) : SEG_SINGLE;
    std::vector<u32> crcs((size_t)nblk);
    std::vector<u64> sizes((size_t)nblk);
    BWTS_TRY(crc_impl(ctx, d_in, n, segs, crcs.data()));
    u8 *a = nullptr, *b = nullptr;
    BWTS_TRY(pack_stage(ctx, 0, n, &a));
    BWTS_TRY(pack_stage(ctx, 1, n, &b));
    BWTS_TRY(seg ? forward_segments_impl(ctx, d_in, n, a) : forward_device_impl(ctx, d_in, n, a));
    HIPC(hipStreamSynchronize(ctx->stream));
    BWTS_TRY(mtf_impl(ctx, a, n, b, false, segs));
    HIPC(hipStreamSynchronize(ctx->stream));
    // the streams go straight to their place; a frame that does not fit is refused by the coder before it writes anything
    BWTS_TRY(ec_encode_impl(ctx, b, n, d_out + fixed, out_cap - fixed, segs, sizes.data()));
    HIPC(hipStreamSynchronize(ctx->stream));
    u8 *head = (u8 *)(ctx->h_small + SM_PACK_HEAD), *dir = nullptr;
    BWTS_TRY(pack_dir_staging(ctx, nblk, &dir));
    u64 total = fixed;
    for (u64 k = 0; k < nblk; k++) {
        pack_entry_write(dir + PACK_ENTRY_BYTES * k, sizes[(size_t)k], crcs[(size_t)k]);
        total += sizes[(size_t)k];
    }
    if (total > out_cap) return BWTS_E_INTERNAL;
    pack_header_write(head, n, B, dir);
    HIPC(hipMemcpyAsync(d_out + PACK_HEADER_BYTES, dir, PACK_ENTRY_BYTES * nblk, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(d_out, head, PACK_HEADER_BYTES, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    *out_bytes = total;
    return BWTS_OK;
}

// The frame is not trusted: header, then directory, are brought to the host and judged by the predicates of pack_plan.h before
// anything is made of them; the coder judges its streams itself.
int unpack_device_impl(bwts_ctx *ctx, const u8 *d_in, u64 in_bytes, u8 *d_out, u64 out_cap, u64 *n_out)
{
    if (in_bytes < PACK_LEAST_FRAME || (in_bytes & 15u)) return BWTS_E_FORMAT;
    u8 *head = (u8 *)(ctx->h_small + SM_PACK_HEAD), *dir = nullptr;
    HIPC(hipMemcpyAsync(head, d_in, PACK_LEAST_FRAME, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    PackHeader H;
    BWTS_TRY(pack_header_check(head, in_bytes, &H));
    const bool seg = H.nblk > 1;
    const u64 fixed = pack_fixed_bytes(H.nblk);
    BWTS_TRY(pack_blocks_set(ctx, H.n, H.B, H.nblk));
    const SegMode segs = seg ? seg_mode(ctx) : SEG_SINGLE;
    BWTS_TRY(pack_dir_staging(ctx, H.nblk, &dir));
    if (seg) {
        HIPC(hipMemcpyAsync(dir, d_in + PACK_HEADER_BYTES, PACK_ENTRY_BYTES * H.nblk, hipMemcpyDeviceToHost, ctx->stream));
        HIPC(hipStreamSynchronize(ctx->stream));
    }
    u64 frame = 0;
    BWTS_TRY(pack_directory_check(dir, H, in_bytes, true, &frame));
    if (H.n > out_cap) return BWTS_E_SPACE;
    ctx->tm.n = H.n;
    // (the staging is the next stage's: what the directory says is kept here)
    std::vector<u64> sizes((size_t)H.nblk);
    std::vector<u32> want((size_t)H.nblk), got((size_t)H.nblk);
    for (u64 k = 0; k < H.nblk; k++) {
        sizes[(size_t)k] = pack_le64(dir + PACK_ENTRY_BYTES * k);
        want[(size_t)k] = ec_le32(dir + PACK_ENTRY_BYTES * k + 8);
    }
    // ranks into d_out, bytes of the transform into the stage block, the input's bytes into d_out
    if (seg) {
        BWTS_TRY(ec_decode_impl(ctx, d_in + fixed, H.n, d_out, H.n, nullptr, segs, sizes.data()));
    } else {
        u64 m = 0;
        const int rc = ec_decode_impl(ctx, d_in + fixed, sizes[0], d_out, H.n, &m, segs, nullptr);
        // (room for the frame's n is what the coder was given: a stream that names more, or less, is not this frame's)
        if (rc == BWTS_E_SPACE || (rc == BWTS_OK && m != H.n)) return BWTS_E_FORMAT;
        BWTS_TRY(rc);
    }
    u8 *a = nullptr;
    BWTS_TRY(pack_stage(ctx, 0, H.n, &a));
    BWTS_TRY(mtf_impl(ctx, d_out, H.n, a, true, segs));
    HIPC(hipStreamSynchronize(ctx->stream));
    BWTS_TRY(seg ? inverse_segments_impl(ctx, a, H.n, d_out) : inverse_device_impl(ctx, a, H.n, d_out));
    HIPC(hipStreamSynchronize(ctx->stream));
    BWTS_TRY(crc_impl(ctx, d_out, H.n, segs, got.data()));
    if (memcmp(got.data(), want.data(), (size_t)H.nblk * sizeof(u32)) != 0) return BWTS_E_CHECKSUM;
    *n_out = H.n;
    return BWTS_OK;
}
