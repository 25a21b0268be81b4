// members_plan.h -- the arithmetic of the member frame (include/bwts_members.h): members of any lengths and widths in one frame, its
// bound, what makes its header and directory valid; and, for a frame of either magic, the judged Frame that every reader fills and
// the plan of a range read: which blocks a list of byte ranges touches.  In the style of pack_plan.h,
// whose codes, CRC-32 and range types it uses: pack.hip, the host side of the calls and a stand-alone host program
// (tests/members_plan_check.cc, built with the sanitizers) all compile this file.
// Version 2 of the frame names a filter (delta_plan.h) beside a member's width; tests/delta_plan_check.cc holds its predicates.
// Version 3 names a method too: a member of method 1 is coded directly, its split bytes cut into coder segments by the rule below, and
// the sizes of a member's several streams lie in a table behind the entries; tests/members_v3_plan_check.cc holds those predicates.
#pragma once
#include "pack_plan.h"
#include "delta_plan.h"

#define MEMBERS_MAGIC 0x4D545742u        // "BWTM"
#define MEMBERS_VERSION 1u
#define MEMBERS_VERSION_2 2u             // entries may name a filter (delta_plan.h) beside the width; written only where one does
#define MEMBERS_VERSION_3 3u             // entries may name a method too, and a table of stream sizes follows them; written only where one does
#define MEMBERS_METHOD_CHAIN 0u          // (delta), split, transform, move-to-front, zero-run coding, coder
#define MEMBERS_METHOD_ORDER0 1u         // (delta), split, coder: every byte plane of a long member a stream of its own
#define MEMBERS_PLANE_MIN 8192u          // elements from which a member's planes are coded apart (the derivation: DESIGN section 20)
#define MEMBERS_HEADER_BYTES 32u
#define MEMBERS_ENTRY_BYTES 32u
#define MEMBERS_MAX_COUNT (1ull << 20)   // the largest directory a "BWTZ" frame can have: 2^32 / 4096
#define MEMBERS_LEAST_FRAME 64u          // header and one directory entry

EC_HD bool members_magic(const uint8_t *h) { return ec_le32(h) == MEMBERS_MAGIC; }
EC_HD uint64_t members_fixed_bytes(uint64_t count) { return MEMBERS_HEADER_BYTES + (uint64_t)MEMBERS_ENTRY_BYTES * count; }

// The word at offset 12 of an entry: the width in bits 0-7, in a version-2 frame the filter in bits 8-15, nothing above.  In a
// version-1 frame the whole word is the width, as it always was.
// In a version-3 frame the method follows in bits 16-23, and bits 24-31 are zero.
EC_HD bool members_method_ok(uint64_t m) { return m <= MEMBERS_METHOD_ORDER0; }
EC_HD uint32_t members_word(uint32_t w, uint32_t f, uint32_t m) { return w | f << 8 | m << 16; }
EC_HD bool members_word_ok(uint32_t word, uint32_t version)
{
    if (version == MEMBERS_VERSION_3)
        return planes_width_w_ok(word & 0xffu) && delta_filter_ok((word >> 8) & 0xffu) && members_method_ok((word >> 16) & 0xffu) && (word >> 24) == 0;
    if (version != MEMBERS_VERSION_2) return planes_width_w_ok(word);
    return planes_width_w_ok(word & 0xffu) && delta_filter_ok((word >> 8) & 0xffu) && (word >> 16) == 0;
}

// The cut of a method-1 member of len bytes and width w into coder segments, the one rule of pack, unpack, the bound and the model:
// with q = len / w elements, w > 1 and q >= MEMBERS_PLANE_MIN make w segments, planes 0 .. w-2 of q bytes each and plane w-1 with the
// tail behind it (q + len - q w bytes: the split's own layout, planes_plan.h); everything else, w = 1 and len < w among it, is one
// segment of len bytes.
EC_HD uint32_t members_direct_segments(uint64_t len, uint32_t w) { return w > 1u && len / w >= MEMBERS_PLANE_MIN ? w : 1u; }
EC_HD uint64_t members_direct_segment_bytes(uint64_t len, uint32_t w, uint32_t i)
{
    if (members_direct_segments(len, w) == 1u) return len;
    const uint64_t q = len / w;
    return i + 1u < w ? q : q + (len - q * w);
}
// the words a member has in the extension table: one per stream where it has several, none where the entry's stream_bytes says it all
EC_HD uint32_t members_table_words(uint64_t len, uint32_t w, uint32_t method)
{
    const uint32_t segs = method == MEMBERS_METHOD_ORDER0 ? members_direct_segments(len, w) : 1u;
    return segs > 1u ? segs : 0u;
}
// does any member name a method?  (methods == NULL: none does.)  Such a pack writes a version-3 frame.
static inline bool members_any_method(const uint32_t *methods, uint64_t count)
{
    for (uint64_t k = 0; methods && k < count; k++)
        if (methods[k] != MEMBERS_METHOD_CHAIN) return true;
    return false;
}
// The 8-byte words of the extension table, the pad word that makes them even among them (widths == NULL: all 1; methods == NULL: all
// 0).  At most 8 count <= 2^23: nothing wraps.
static inline uint64_t members_ext_words(const uint64_t *lengths, const uint32_t *widths, const uint32_t *methods, uint64_t count)
{
    uint64_t words = 0;
    for (uint64_t k = 0; methods && k < count; k++) words += members_table_words(lengths[k], widths ? widths[k] : 1u, methods[k]);
    return words + (words & 1u);
}
EC_HD uint64_t members_fixed_bytes_x(uint64_t count, uint64_t ext) { return members_fixed_bytes(count) + 8u * ext; }
// does any member name a filter?  (filters == NULL: none does.)  Such a pack writes a version-2 frame, every other one version 1.
static inline bool members_any_filter(const uint32_t *filters, uint64_t count)
{
    for (uint64_t k = 0; filters && k < count; k++)
        if (filters[k] != DELTA_FILTER_NONE) return true;
    return false;
}

// What a pack is asked for: PACK_ARG for no members, a zero length, a bad width (widths == NULL: all 1) or a bad filter (filters ==
// NULL: none), PACK_RANGE for more than 2^20 members or more than 2^32 bytes, else PACK_OK and *n.  The sum cannot wrap: it is held
// against 2^32 after every member.
// methods == NULL: all 0; a method other than 0 or 1 is PACK_ARG with the bad widths and filters.
static inline int members_args_check_m(const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters, const uint32_t *methods, uint64_t count,
                                       uint64_t *n)
{
    if (!lengths || count == 0) return PACK_ARG;
    if (count > MEMBERS_MAX_COUNT) return PACK_RANGE;
    for (uint64_t k = 0; k < count; k++)
        if (lengths[k] == 0 || (widths && !planes_width_w_ok(widths[k])) || (filters && !delta_filter_ok(filters[k])) ||
            (methods && !members_method_ok(methods[k])))
            return PACK_ARG;
    uint64_t sum = 0;
    for (uint64_t k = 0; k < count; k++) {
        if (lengths[k] > PACK_MAX_N - sum) return PACK_RANGE;
        sum += lengths[k];
    }
    *n = sum;
    return PACK_OK;
}
static inline int members_args_check_f(const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters, uint64_t count, uint64_t *n)
{
    return members_args_check_m(lengths, widths, filters, nullptr, count, n);
}
static inline int members_args_check(const uint64_t *lengths, const uint32_t *widths, uint64_t count, uint64_t *n)
{
    return members_args_check_f(lengths, widths, nullptr, count, n);
}

// 32 + 32 count + the coder's bound of every member (the split never changes a length, the zero-run stage never expands); 0 on
// arguments that members_args_check refuses
static inline uint64_t members_bound_bytes(const uint64_t *lengths, uint64_t count)
{
    uint64_t n = 0;
    if (members_args_check(lengths, nullptr, count, &n) != PACK_OK) return 0;
    uint64_t total = members_fixed_bytes(count);
    for (uint64_t k = 0; k < count; k++) total += ec_bound_bytes(lengths[k]);
    return total;
}
// every member at least one coded byte
EC_HD uint64_t members_least_bytes(uint64_t count) { return members_fixed_bytes(count) + count * ec_least_bytes(1u); }
// With methods: 32 + 32 count + 8 ext + the coder's bound of every coder segment, a chain member's one of len bytes and a direct
// member's by the cut rule; 0 on arguments that members_args_check_m refuses.  Without a method it is members_bound_bytes.
static inline uint64_t members_bound_bytes_m(const uint64_t *lengths, const uint32_t *widths, const uint32_t *methods, uint64_t count)
{
    uint64_t n = 0;
    if (members_args_check_m(lengths, widths, nullptr, methods, count, &n) != PACK_OK) return 0;
    uint64_t total = members_fixed_bytes_x(count, members_ext_words(lengths, widths, methods, count));
    for (uint64_t k = 0; k < count; k++) {
        const uint32_t w = widths ? widths[k] : 1u;
        const uint32_t segs = methods && methods[k] == MEMBERS_METHOD_ORDER0 ? members_direct_segments(lengths[k], w) : 1u;
        for (uint32_t i = 0; i < segs; i++) total += ec_bound_bytes(segs > 1u ? members_direct_segment_bytes(lengths[k], w, i) : lengths[k]);
    }
    return total;
}
// the least room a pack needs: a chain member's stream codes one byte at least, a direct member's segments are known
static inline uint64_t members_least_bytes_m(const uint64_t *lengths, const uint32_t *widths, const uint32_t *methods, uint64_t count)
{
    uint64_t total = members_fixed_bytes_x(count, members_ext_words(lengths, widths, methods, count));
    for (uint64_t k = 0; k < count; k++) {
        const uint32_t w = widths ? widths[k] : 1u;
        if (!methods || methods[k] != MEMBERS_METHOD_ORDER0) { total += ec_least_bytes(1u); continue; }
        const uint32_t segs = members_direct_segments(lengths[k], w);
        for (uint32_t i = 0; i < segs; i++) total += ec_least_bytes(members_direct_segment_bytes(lengths[k], w, i));
    }
    return total;
}

// ---- a filter or a method left to the pack (bwts_pack_members_a*; the rules: include/bwts_members.h, "AUTO") ----
#define MEMBERS_AUTO 255u                // BWTS_FILTER_AUTO, BWTS_METHOD_AUTO
// members_args_check_m with MEMBERS_AUTO among the filters and the methods
static inline int members_args_check_a(const uint64_t *lengths, const uint32_t *widths, const uint32_t *filters, const uint32_t *methods, uint64_t count,
                                       uint64_t *n)
{
    const int rc = members_args_check_m(lengths, widths, nullptr, nullptr, count, n);
    if (rc != PACK_OK) return rc;
    for (uint64_t k = 0; k < count; k++)
        if ((filters && filters[k] != MEMBERS_AUTO && !delta_filter_ok(filters[k])) || (methods && methods[k] != MEMBERS_AUTO && !members_method_ok(methods[k])))
            return PACK_ARG;
    return PACK_OK;
}
static inline bool members_any_auto(const uint32_t *values, uint64_t count)
{
    for (uint64_t k = 0; values && k < count; k++)
        if (values[k] == MEMBERS_AUTO) return true;
    return false;
}
// the coder's bound of a member's streams under a method that is 0 or 1
static inline uint64_t members_streams_bound(uint64_t len, uint32_t w, uint32_t method)
{
    const uint32_t segs = method == MEMBERS_METHOD_ORDER0 ? members_direct_segments(len, w) : 1u;
    uint64_t total = 0;
    for (uint32_t i = 0; i < segs; i++) total += ec_bound_bytes(segs > 1u ? members_direct_segment_bytes(len, w, i) : len);
    return total;
}
// What a method's encoding of a member costs the frame: its streams and its words of the extension table.  The smaller cost wins an
// AUTO, and a tie goes to the chain.
EC_HD uint64_t members_method_cost(uint64_t stream_bytes, uint64_t len, uint32_t w, uint32_t method)
{
    return stream_bytes + 8u * members_table_words(len, w, method);
}
EC_HD uint32_t members_method_choice(uint64_t chain_cost, uint64_t direct_cost) { return direct_cost < chain_cost ? MEMBERS_METHOD_ORDER0 : MEMBERS_METHOD_CHAIN; }
// The bound with AUTO among the methods: the extension table with every AUTO member's words, and an AUTO member's streams at the
// larger of its two bounds; without AUTO it is members_bound_bytes_m.  0 on arguments that members_args_check_a refuses.
static inline uint64_t members_bound_bytes_a(const uint64_t *lengths, const uint32_t *widths, const uint32_t *methods, uint64_t count)
{
    uint64_t n = 0, words = 0;
    if (members_args_check_a(lengths, widths, nullptr, methods, count, &n) != PACK_OK) return 0;
    uint64_t total = 0;
    for (uint64_t k = 0; k < count; k++) {
        const uint32_t w = widths ? widths[k] : 1u, m = methods ? methods[k] : MEMBERS_METHOD_CHAIN;
        const uint64_t chain = members_streams_bound(lengths[k], w, MEMBERS_METHOD_CHAIN), direct = members_streams_bound(lengths[k], w, MEMBERS_METHOD_ORDER0);
        if (m != MEMBERS_METHOD_CHAIN) words += members_table_words(lengths[k], w, MEMBERS_METHOD_ORDER0);
        total += m == MEMBERS_METHOD_CHAIN ? chain : (m == MEMBERS_METHOD_ORDER0 ? direct : (chain > direct ? chain : direct));
    }
    return total + members_fixed_bytes_x(count, words + (words & 1u));
}

EC_HD void members_entry_write(uint8_t e[32], uint64_t stream_bytes, uint32_t crc, uint32_t width, uint64_t coded_bytes, uint64_t len)
{
    pack_put64(e, stream_bytes); ec_put32(e + 8, crc); ec_put32(e + 12, width); pack_put64(e + 16, coded_bytes); pack_put64(e + 24, len);
}
// the header of a frame whose directory (count entries, and behind them ext words of the extension table: version 3 alone has any) is
// complete; the word at offset 16 is the count, and in a version-3 header its upper half is ext
EC_HD void members_header_write_x(uint8_t h[32], uint32_t version, uint64_t n, uint64_t count, uint64_t ext, const uint8_t *dir)
{
    ec_put32(h, MEMBERS_MAGIC); ec_put32(h + 4, version); pack_put64(h + 8, n); pack_put64(h + 16, count | ext << 32);
    ec_put32(h + 24, crc32_bytes(dir, (uint64_t)MEMBERS_ENTRY_BYTES * count + 8u * ext));
    ec_put32(h + 28, crc32_bytes(h, 28));
}
EC_HD void members_header_write_v(uint8_t h[32], uint32_t version, uint64_t n, uint64_t count, const uint8_t *dir)
{
    members_header_write_x(h, version, n, count, 0, dir);
}
EC_HD void members_header_write(uint8_t h[32], uint64_t n, uint64_t count, const uint8_t *dir)
{
    members_header_write_v(h, MEMBERS_VERSION, n, count, dir);
}

struct MembersHeader { uint64_t n, count; uint32_t dir_crc, version; uint64_t ext = 0; };

// The header of a frame of which in_bytes bytes are at hand (h: the first 32 of them, read only when in_bytes allows a frame at all).
// PACK_OK and *H, PACK_FORMAT, or PACK_RANGE for a sound header that names more than 2^32 bytes or more than 2^20 members.
EC_HD int members_header_check(const uint8_t *h, uint64_t in_bytes, MembersHeader *H)
{
    if (in_bytes < MEMBERS_LEAST_FRAME || (in_bytes & 15u)) return PACK_FORMAT;
    if (ec_le32(h) != MEMBERS_MAGIC || (ec_le32(h + 4) != MEMBERS_VERSION && ec_le32(h + 4) != MEMBERS_VERSION_2)) return PACK_FORMAT;
    if (ec_le32(h + 28) != crc32_bytes(h, 28)) return PACK_FORMAT;
    const uint64_t n = pack_le64(h + 8), count = pack_le64(h + 16);
    if (n == 0) return PACK_FORMAT;
    if (n > PACK_MAX_N) return PACK_RANGE;
    if (count == 0 || count > n) return PACK_FORMAT;
    if (count > MEMBERS_MAX_COUNT) return PACK_RANGE;
    H->n = n; H->count = count; H->dir_crc = ec_le32(h + 24); H->version = ec_le32(h + 4);
    if (members_fixed_bytes(count) > in_bytes) return PACK_FORMAT;
    return PACK_OK;
}

// A version-3 header: the same checks in the same order, with the word at offset 16 read as u32 count and u32 ext.  Versions 1 and 2
// stay with members_header_check, which knows no other; members_head_check sends a header to the one its version word names.
// Nothing wraps: count <= 2^20 when the fixed bytes are formed, and ext < 2^32, so 32 + 32 count + 8 ext < 2^36.
EC_HD int members_header_check_v3(const uint8_t *h, uint64_t in_bytes, MembersHeader *H)
{
    if (in_bytes < MEMBERS_LEAST_FRAME || (in_bytes & 15u)) return PACK_FORMAT;
    if (ec_le32(h) != MEMBERS_MAGIC || ec_le32(h + 4) != MEMBERS_VERSION_3) return PACK_FORMAT;
    if (ec_le32(h + 28) != crc32_bytes(h, 28)) return PACK_FORMAT;
    const uint64_t n = pack_le64(h + 8), count = ec_le32(h + 16), ext = ec_le32(h + 20);
    if (n == 0) return PACK_FORMAT;
    if (n > PACK_MAX_N) return PACK_RANGE;
    if (count == 0 || count > n) return PACK_FORMAT;
    if (count > MEMBERS_MAX_COUNT) return PACK_RANGE;
    H->n = n; H->count = count; H->dir_crc = ec_le32(h + 24); H->version = MEMBERS_VERSION_3; H->ext = ext;
    if (members_fixed_bytes_x(count, ext) > in_bytes) return PACK_FORMAT;
    return PACK_OK;
}
EC_HD int members_head_check(const uint8_t *h, uint64_t in_bytes, MembersHeader *H)
{
    if (in_bytes >= MEMBERS_LEAST_FRAME && ec_le32(h + 4) == MEMBERS_VERSION_3) return members_header_check_v3(h, in_bytes, H);
    return members_header_check(h, in_bytes, H);
}

// The directory behind a header that passed (dir: H.count entries and H.ext table words, which in_bytes holds).  exact: the frame must
// be all of in_bytes (an unpack), else it may end earlier (stepping through concatenated frames).  PACK_OK and *frame_bytes, or
// PACK_FORMAT.
EC_HD int members_directory_check(const uint8_t *dir, const MembersHeader &H, uint64_t in_bytes, bool exact, uint64_t *frame_bytes)
{
    const bool v3 = H.version == MEMBERS_VERSION_3;
    const uint8_t *table = dir + (uint64_t)MEMBERS_ENTRY_BYTES * H.count;
    if (crc32_bytes(dir, (uint64_t)MEMBERS_ENTRY_BYTES * H.count + 8u * H.ext) != H.dir_crc) return PACK_FORMAT;
    uint64_t total = members_fixed_bytes_x(H.count, H.ext), sum = 0, words = 0;
    bool filtered = false, direct = false;
    for (uint64_t k = 0; k < H.count; k++) {
        const uint8_t *e = dir + (uint64_t)MEMBERS_ENTRY_BYTES * k;
        const uint64_t sb = pack_le64(e), coded = pack_le64(e + 16), len = pack_le64(e + 24);
        const uint32_t word = ec_le32(e + 12);
        if (!members_word_ok(word, H.version)) return PACK_FORMAT;
        filtered = filtered || (word >> 8) != 0;
        if (len == 0 || len > H.n - sum) return PACK_FORMAT;       // (by subtraction: the running sum stays within n <= 2^32)
        sum += len;
        if (coded == 0 || coded > len) return PACK_FORMAT;
        const uint32_t method = v3 ? (word >> 16) & 0xffu : MEMBERS_METHOD_CHAIN, segs = members_table_words(len, word & 0xffu, method);
        if (method == MEMBERS_METHOD_ORDER0) {
            direct = true;
            if (coded != len) return PACK_FORMAT;
        }
        if (segs == 0) {
            if ((sb & 15u) || sb < ec_least_bytes(coded) || sb > ec_bound_bytes(coded)) return PACK_FORMAT;      // (so the sum cannot overflow)
        } else {
            // the member's table words: inside the table (words <= ext < 2^32 here, segs <= 8), and each inside what the coder can make
            // of its segment, at most ec_bound_bytes(2^32) < 2^34, so that eight of them cannot wrap; total grows by what the frame's
            // length bounds at the end, as it always did
            if (segs > H.ext - words) return PACK_FORMAT;
            uint64_t member = 0;
            for (uint32_t i = 0; i < segs; i++) {
                const uint64_t ssb = pack_le64(table + 8u * (words + i)), slen = members_direct_segment_bytes(len, word & 0xffu, i);
                if ((ssb & 15u) || ssb < ec_least_bytes(slen) || ssb > ec_bound_bytes(slen)) return PACK_FORMAT;
                member += ssb;
            }
            if (member != sb) return PACK_FORMAT;
            words += segs;
        }
        total += sb;
    }
    // the frame is canonical: version 2 is written only where an entry names a filter, version 3 only where one names a method; the
    // table is exactly what the entries demand, and its pad word is zero
    if (v3 && !direct) return PACK_FORMAT;
    if (words + (words & 1u) != H.ext) return PACK_FORMAT;
    if ((words & 1u) && pack_le64(table + 8u * words) != 0) return PACK_FORMAT;
    if (H.version == MEMBERS_VERSION_2 && !filtered) return PACK_FORMAT;
    if (sum != H.n) return PACK_FORMAT;
    if (exact ? total != in_bytes : total > in_bytes) return PACK_FORMAT;
    *frame_bytes = total;
    return PACK_OK;
}

// width and filter of an entry of a directory that passed its check
EC_HD uint32_t members_entry_width(const uint8_t *dir, uint64_t k) { return ec_le32(dir + (uint64_t)MEMBERS_ENTRY_BYTES * k + 12) & 0xffu; }
EC_HD uint32_t members_entry_filter(const uint8_t *dir, uint64_t k) { return (ec_le32(dir + (uint64_t)MEMBERS_ENTRY_BYTES * k + 12) >> 8) & 0xffu; }
EC_HD uint32_t members_entry_method(const uint8_t *dir, uint64_t k) { return (ec_le32(dir + (uint64_t)MEMBERS_ENTRY_BYTES * k + 12) >> 16) & 0xffu; }      // (version 3)

// ---- a judged frame of either magic ----
// What every user of a frame needs of its header and directory, so that nobody reads either again: the device forms' directory lies
// in staging that the first stage writes over.  A reader fills it in two steps, frame_head_check and frame_dir_check, because the
// device form reads the header before it can fetch the directory.  "BWTZ": the blocks are min(k B, n), the width is the directory's
// one (version 3; else 1, no split) and no block is filtered.  "BWTM": every member is a block, and its entry says all of it.
struct Frame {
    bool members = false;                       // "BWTM"
    PackHeader z;                               // the judged header: "BWTZ" ...
    MembersHeader m;                            // ... or "BWTM"
    uint64_t n = 0, count = 0;                  // bytes and blocks
    uint64_t B = 0;                             // the uniform block length ("BWTZ"); 0: the block of a byte is found by bisecting off
    uint64_t entry = 0, fixed = 0;              // bytes of a directory entry, and of header and directory
    bool zrl = false;                           // the streams are the coder's over zero-run coded bytes
    std::vector<uint64_t> off, stream, coded;   // per block: where it begins (count + 1), stream bytes, coded bytes (not zrl: its length)
    std::vector<uint32_t> crc, width, filter;
    // "BWTM" version 3: every block's method, and the extension table (ext words, behind the entries and inside `fixed`): the stream
    // sizes of block k's segments are table[table_at[k]] .. table[table_at[k + 1]), none where it has one stream.  Empty elsewhere.
    uint64_t ext = 0;
    std::vector<uint32_t> method;
    std::vector<uint64_t> table_at, table;
    bool direct(uint64_t k) const { return !method.empty() && method[(size_t)k] == MEMBERS_METHOD_ORDER0; }
    uint64_t len(uint64_t k) const { return off[(size_t)k + 1] - off[(size_t)k]; }
};

static_assert(MEMBERS_HEADER_BYTES == PACK_HEADER_BYTES, "the directory of either frame begins behind 32 bytes");

// The header of a frame of which in_bytes bytes are at hand (h: the first 32 of them, read only when in_bytes allows them): the magic
// chooses the predicate, whose code this returns.  PACK_OK: everything of *F that needs no directory.
static inline int frame_head_check(const uint8_t *h, uint64_t in_bytes, Frame *F)
{
    int rc;
    F->members = in_bytes >= MEMBERS_HEADER_BYTES && members_magic(h);
    if (F->members) {
        if ((rc = members_head_check(h, in_bytes, &F->m)) != PACK_OK) return rc;
        F->n = F->m.n; F->count = F->m.count; F->B = 0; F->entry = MEMBERS_ENTRY_BYTES; F->zrl = true; F->ext = F->m.ext;
    } else {
        if ((rc = pack_header_check(h, in_bytes, &F->z)) != PACK_OK) return rc;
        F->n = F->z.n; F->count = F->z.nblk; F->B = F->z.B; F->entry = pack_entry_bytes(F->z.version); F->zrl = F->z.version != PACK_VERSION;
    }
    F->fixed = PACK_HEADER_BYTES + F->entry * F->count + 8u * F->ext;
    return PACK_OK;
}

// The directory behind a header that passed (dir: F.count entries and F.ext table words, which in_bytes holds; exact: as the predicates take it).  PACK_OK,
// *frame_bytes and the rest of F, or the predicate's code.
static inline int frame_dir_check(const uint8_t *dir, Frame &F, uint64_t in_bytes, bool exact, uint64_t *frame_bytes)
{
    const int rc = F.members ? members_directory_check(dir, F.m, in_bytes, exact, frame_bytes) : pack_directory_check(dir, F.z, in_bytes, exact, frame_bytes);
    if (rc != PACK_OK) return rc;
    const size_t c = (size_t)F.count;
    F.off.assign(c + 1, 0); F.stream.resize(c); F.coded.resize(c); F.crc.resize(c); F.width.resize(c); F.filter.resize(c);
    for (size_t k = 0; k < c; k++) {
        const uint8_t *e = dir + F.entry * k;
        const uint64_t len = F.members ? pack_le64(e + 24) : pack_block_at(F.n, F.B, k);
        F.off[k + 1] = F.off[k] + len;
        F.stream[k] = pack_le64(e);
        F.crc[k] = ec_le32(e + 8);
        F.coded[k] = F.zrl ? pack_le64(e + 16) : len;
        F.width[k] = F.members ? members_entry_width(dir, k) : F.z.version == PACK_VERSION_3 ? F.z.width : 1u;
        F.filter[k] = F.members ? members_entry_filter(dir, k) : DELTA_FILTER_NONE;
    }
    if (!F.members || F.m.version != MEMBERS_VERSION_3) return PACK_OK;
    F.method.resize(c); F.table_at.assign(c + 1, 0); F.table.clear();
    const uint8_t *table = dir + F.entry * c;
    for (size_t k = 0; k < c; k++) {
        F.method[k] = members_entry_method(dir, k);
        const uint32_t words = members_table_words(F.len(k), F.width[k], F.method[k]);
        for (uint32_t i = 0; i < words; i++) F.table.push_back(pack_le64(table + 8u * (F.table_at[k] + i)));
        F.table_at[k + 1] = F.table_at[k] + words;
    }
    return PACK_OK;
}

// the block that holds byte `at` (at < n): a division where the blocks are uniform, else the last one that does not begin behind it
static inline uint64_t frame_block_of(const Frame &F, uint64_t at)
{
    if (F.B) return at / F.B;
    uint64_t lo = 0, hi = F.count;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (F.off[(size_t)mid] <= at) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The indices of a bwts_unpack_members call against a judged member frame, as the ranges they stand for: PACK_ARG, then PACK_RANGE for
// more than 2^20 indices or one that names no member; else PACK_OK and one range per index, in the order asked.
static inline int members_index_ranges(const Frame &F, const uint64_t *indices, uint64_t icount, std::vector<PackRange> *r)
{
    if (!indices || icount == 0) return PACK_ARG;
    if (icount > PACK_MAX_RANGES) return PACK_RANGE;
    r->clear();
    for (uint64_t i = 0; i < icount; i++) {
        if (indices[i] >= F.count) return PACK_RANGE;
        r->push_back(PackRange{F.off[(size_t)indices[i]], F.len(indices[i])});
    }
    return PACK_OK;
}

// The plan of a range read (pack_plan.h: PackRangesPlan).  F has passed both checks, the ranges pack_ranges_check against F.n.  Nothing
// here can overflow: the directory check has held the sum of all stream bytes against the frame's length, the coded bytes against the
// blocks' lengths, and the blocks' lengths add up to n <= 2^32; the ranges' sum is bounded by their check.
static inline void ranges_plan(const Frame &F, const PackRange *r, uint64_t count, PackRangesPlan *P)
{
    // how many ranges begin in a block minus how many end in the one before: a running sum above zero marks a covered block
    std::vector<int32_t> step((size_t)F.count + 1, 0);
    for (uint64_t i = 0; i < count; i++) {
        step[(size_t)frame_block_of(F, r[i].offset)]++;
        step[(size_t)frame_block_of(F, r[i].offset + r[i].bytes - 1u) + 1]--;
    }
    std::vector<uint64_t> at((size_t)F.count, 0);        // where a covered block begins in the covered-block buffer
    P->runs.clear(); P->streams.clear(); P->out.clear(); P->blocks.clear();
    P->covered_bytes = P->stream_bytes = P->coded_bytes = P->out_bytes = 0;
    uint64_t frame_at = F.fixed;
    int64_t open = 0;
    bool in_run = false;
    for (uint64_t b = 0; b < F.count; b++) {
        const uint64_t sb = F.stream[(size_t)b];
        open += step[(size_t)b];
        if (open > 0) {
            if (!in_run) {
                P->runs.push_back(PackRun{b, 0});
                P->streams.push_back(PackPiece{frame_at, P->stream_bytes, 0});
            }
            P->runs.back().blocks++;
            P->streams.back().bytes += sb;
            P->blocks.push_back(b);
            at[(size_t)b] = P->covered_bytes;
            P->covered_bytes += F.len(b);
            P->stream_bytes += sb;
            P->coded_bytes += F.coded[(size_t)b];
        }
        in_run = open > 0;
        frame_at += sb;
    }
    for (uint64_t i = 0; i < count; i++) {
        const uint64_t b = frame_block_of(F, r[i].offset);
        P->out.push_back(PackPiece{at[(size_t)b] + (r[i].offset - F.off[(size_t)b]), P->out_bytes, r[i].bytes});
        P->out_bytes += r[i].bytes;
    }
}

// A frame that the host holds whole, and the ranges asked of it: header, directory and ranges judged in unpack's order with unpack's
// codes, then the plan.  indices: not null for whole members as the ranges (`ranges` is then not read, a "BWTZ" frame is PACK_FORMAT,
// and *ranges_out points into *whole).
static inline int frame_ranges_plan(const uint8_t *frame, uint64_t in_bytes, const PackRange *ranges, const uint64_t *indices, uint64_t count,
                                    uint64_t out_cap, Frame *F, uint64_t *sum, std::vector<PackRange> *whole, const PackRange **ranges_out,
                                    PackRangesPlan *P)
{
    uint64_t frame_bytes = 0;
    int rc;
    if ((rc = frame_head_check(frame, in_bytes, F)) != PACK_OK) return rc;
    if ((rc = frame_dir_check(frame + PACK_HEADER_BYTES, *F, in_bytes, true, &frame_bytes)) != PACK_OK) return rc;
    if (indices) {
        if (!F->members) return PACK_FORMAT;
        if ((rc = members_index_ranges(*F, indices, count, whole)) != PACK_OK) return rc;
        ranges = whole->data();
    }
    if ((rc = pack_ranges_check(F->n, ranges, count, out_cap, sum)) != PACK_OK) return rc;
    ranges_plan(*F, ranges, count, P);
    *ranges_out = ranges;
    return PACK_OK;
}
