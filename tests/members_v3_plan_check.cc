// members_v3_plan_check.cc -- stand-alone host program over the version-3 arithmetic of bijective-bwt_amd/csrc/members_plan.h: the cut
// rule of a direct member, the extension table's words, the predicates, the bound, and frames with hostile words.
// tests/test_pack_members_v3_model.py builds it with -fsanitize=address,undefined and runs it: every buffer below is a heap block of
// exactly the size the checked function may touch.  Prints the number of checks and "ok"; exits 1 with the failing line otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "members_plan.h"

static long checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        checks++;                                                                \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

// a heap block of exactly n bytes
struct Exact {
    uint8_t *p;
    explicit Exact(uint64_t n) : p((uint8_t *)malloc(n ? n : 1)) {}
    ~Exact() { free(p); }
};

static const uint32_t WIDTHS[4] = {1, 2, 4, 8};

static void cut_checks()
{
    for (uint32_t w : WIDTHS) {
        const uint64_t at = (uint64_t)w * MEMBERS_PLANE_MIN;
        const uint64_t lens[] = {1, w - 1u ? w - 1u : 1u, w, at - 1, at, at + 1, at + w - 1, at + w, 3 * at + 5, 1ull << 32};
        for (uint64_t len : lens) {
            const uint32_t segs = members_direct_segments(len, w);
            CHECK(segs == (w > 1 && len / w >= 8192 ? w : 1u));
            uint64_t sum = 0;
            for (uint32_t i = 0; i < segs; i++) {
                const uint64_t s = members_direct_segment_bytes(len, w, i);
                CHECK(s >= 1 && (segs == 1 || s >= MEMBERS_PLANE_MIN) && (segs == 1 || i + 1 == segs || s == len / w));
                sum += s;
            }
            CHECK(sum == len);
            CHECK(members_table_words(len, w, MEMBERS_METHOD_ORDER0) == (segs > 1 ? segs : 0u) && members_table_words(len, w, MEMBERS_METHOD_CHAIN) == 0);
        }
    }
    // q = 8191 and q = 8192 at width 2, and the tail behind the last plane
    CHECK(members_direct_segments(2 * 8191 + 1, 2) == 1 && members_direct_segments(2 * 8192, 2) == 2);
    CHECK(members_direct_segment_bytes(2 * 8192 + 1, 2, 0) == 8192 && members_direct_segment_bytes(2 * 8192 + 1, 2, 1) == 8193);
    CHECK(members_direct_segment_bytes(8 * 8192 + 7, 8, 6) == 8192 && members_direct_segment_bytes(8 * 8192 + 7, 8, 7) == 8199);
    CHECK(members_direct_segment_bytes(100, 4, 0) == 100);
}

static void word_and_args_checks()
{
    CHECK(members_word(4, 1, 1) == 0x10104 && members_word(2, 0, 0) == 2);
    CHECK(members_word_ok(0x10104, MEMBERS_VERSION_3) && members_word_ok(4, MEMBERS_VERSION_3) && members_word_ok(0x104, MEMBERS_VERSION_3));
    CHECK(!members_word_ok(0x20104, MEMBERS_VERSION_3) && !members_word_ok(0xff0004, MEMBERS_VERSION_3) && !members_word_ok(0x1010104, MEMBERS_VERSION_3));
    CHECK(!members_word_ok(0x80010104u, MEMBERS_VERSION_3) && !members_word_ok(0x10103, MEMBERS_VERSION_3) && !members_word_ok(0x10204, MEMBERS_VERSION_3));
    // versions 1 and 2 know no method
    CHECK(!members_word_ok(0x10104, MEMBERS_VERSION_2) && !members_word_ok(0x10004, MEMBERS_VERSION));
    for (uint64_t m = 0; m < 40; m++) CHECK(members_method_ok(m) == (m <= 1));
    CHECK(!members_method_ok(1ull << 32) && !members_method_ok(~0ull));
    const uint64_t ls[4] = {16385, 100, 32768, 9};
    const uint32_t ws[4] = {2, 4, 4, 8}, ms[4] = {1, 1, 1, 0}, none[4] = {0, 0, 0, 0}, bad[4] = {0, 2, 0, 0}, two[4] = {1, 1, 0, 0};
    uint64_t n = 0;
    CHECK(members_args_check_m(ls, ws, nullptr, ms, 4, &n) == PACK_OK && n == 49262 && members_args_check_m(ls, ws, nullptr, nullptr, 4, &n) == PACK_OK);
    CHECK(members_args_check_m(ls, ws, nullptr, bad, 4, &n) == PACK_ARG && members_args_check_m(ls, nullptr, nullptr, ms, 4, &n) == PACK_OK);
    CHECK(members_any_method(ms, 4) && !members_any_method(none, 4) && !members_any_method(nullptr, 4));
    // the table: w words per member with planes, an even number in all
    CHECK(members_ext_words(ls, ws, ms, 4) == 6 && members_ext_words(ls, ws, two, 4) == 2 && members_ext_words(ls, ws, none, 4) == 0);
    CHECK(members_ext_words(ls, ws, nullptr, 4) == 0 && members_ext_words(ls, nullptr, ms, 4) == 0);
    // the bound: every coder segment's own, and without a method the bound that always was
    uint64_t want = 32 + 32 * 4 + 48;
    const uint64_t segs[8] = {8192, 8193, 100, 8192, 8192, 8192, 8192, 9};
    for (uint64_t s : segs) want += ec_bound_bytes(s);
    CHECK(members_bound_bytes_m(ls, ws, ms, 4) == want && members_bound_bytes_m(ls, ws, none, 4) == members_bound_bytes(ls, 4));
    CHECK(members_bound_bytes_m(ls, ws, nullptr, 4) == members_bound_bytes(ls, 4) && members_bound_bytes_m(ls, ws, bad, 4) == 0);
    CHECK(members_bound_bytes_m(ls, ws, ms, 0) == 0 && members_bound_bytes_m(nullptr, ws, ms, 4) == 0);
    uint64_t least = 32 + 32 * 4 + 48 + ec_least_bytes(1);
    for (int i = 0; i < 7; i++) least += ec_least_bytes(segs[i]);
    CHECK(members_least_bytes_m(ls, ws, ms, 4) == least && members_least_bytes_m(ls, ws, nullptr, 4) == members_least_bytes(4));
    CHECK(members_least_bytes_m(ls, ws, ms, 4) <= members_bound_bytes_m(ls, ws, ms, 4));
}

// A frame of three members -- chain, direct with two planes, direct in one segment -- with the least streams the coder can make: head,
// dir (entries and table) are heap blocks of exactly their size.  edit: what is wrong with it.
enum Edit { SOUND, NO_METHOD, METHOD_2, BIT_24, CODED_SHORT, WORD_ODD, WORD_LOW, WORD_HIGH, WORD_WRAP, SUM_OFF, SINGLE_LOW, EXT_MORE, EXT_NONE, EXT_MAX,
            EXT_LONG, EDITS };
static int judge(Edit edit, uint64_t *frame_out)
{
    const uint64_t ls[3] = {5, 2 * 8192 + 1, 4003};
    const uint32_t ws[3] = {1, 2, 4};
    uint32_t ms[3] = {0, 1, 1};
    if (edit == NO_METHOD) ms[1] = ms[2] = 0;
    uint64_t ext = edit == NO_METHOD ? 0 : 2;
    if (edit == EXT_MORE) ext = 4;
    if (edit == EXT_NONE) ext = 0;
    Exact head(MEMBERS_HEADER_BYTES), dir(3 * MEMBERS_ENTRY_BYTES + 8 * ext);
    uint64_t t[2] = {ec_least_bytes(8192), ec_least_bytes(8193)};
    if (edit == WORD_ODD) { t[0] += 8; t[1] -= 8; }
    if (edit == WORD_LOW) { t[0] -= 16; t[1] += 16; }
    if (edit == WORD_HIGH) { t[0] = ec_bound_bytes(8192) + 16; }
    if (edit == WORD_WRAP) { t[0] = ~0ull - 15; t[1] = 32 + ec_least_bytes(8192) + ec_least_bytes(8193); }     // (their sum wraps to a stream size)
    uint64_t sb[3] = {ec_least_bytes(5), ec_least_bytes(8192) + ec_least_bytes(8193), ec_least_bytes(4003)};
    if (edit == NO_METHOD) sb[1] = ec_least_bytes(ls[1]);
    if (edit == WORD_HIGH) sb[1] = t[0] + t[1];
    if (edit == SUM_OFF) sb[1] += 16;
    if (edit == SINGLE_LOW) sb[2] -= 16;
    uint64_t total = members_fixed_bytes_x(3, ext);
    for (int k = 0; k < 3; k++) {
        uint32_t word = members_word(ws[k], 0, ms[k]);
        if (edit == METHOD_2 && k == 1) word = members_word(2, 0, 2);
        if (edit == BIT_24 && k == 2) word |= 1u << 24;
        const uint64_t coded = edit == CODED_SHORT && k == 2 ? ls[k] - 1 : ls[k];
        members_entry_write(dir.p + MEMBERS_ENTRY_BYTES * k, sb[k], 0x12345678u, word, coded, ls[k]);
        total += sb[k];
    }
    uint8_t *table = dir.p + 3 * MEMBERS_ENTRY_BYTES;
    for (uint64_t i = 0; i < ext; i++) pack_put64(table + 8 * i, i < 2 ? t[i] : 0);
    uint64_t named = ext;
    if (edit == EXT_MAX) named = 0xffffffffull;
    if (edit == EXT_LONG) named = total / 8;
    members_header_write_x(head.p, MEMBERS_VERSION_3, 16385 + 4003 + 5, 3, ext, dir.p);
    if (named != ext) {
        // the header names a table that is not there: its own CRC made right again, so that the size check is what refuses
        pack_put64(head.p + 16, 3 | named << 32);
        ec_put32(head.p + 28, crc32_bytes(head.p, 28));
    }
    MembersHeader M;
    int rc = members_head_check(head.p, total, &M);
    if (rc != PACK_OK) return rc;
    CHECK(M.version == MEMBERS_VERSION_3 && M.count == 3 && M.ext == ext);
    rc = members_directory_check(dir.p, M, total, true, frame_out);
    if (rc == PACK_OK) CHECK(*frame_out == total);
    return rc;
}

static void frame_checks()
{
    for (int e = 0; e < EDITS; e++) {
        uint64_t frame = 0;
        const int rc = judge((Edit)e, &frame);
        if (rc != (e == SOUND ? PACK_OK : PACK_FORMAT)) fprintf(stderr, "edit %d: %d\n", e, rc);
        CHECK(rc == (e == SOUND ? PACK_OK : PACK_FORMAT));
    }
    // the judged frame: methods, and the table words where a member has them
    const uint64_t ls[3] = {5, 2 * 8192 + 1, 4003};
    const uint64_t t[2] = {ec_least_bytes(8192), ec_least_bytes(8193)};
    Exact frame(members_fixed_bytes_x(3, 2));
    const uint32_t ws[3] = {1, 2, 4}, ms[3] = {0, 1, 1};
    uint64_t total = members_fixed_bytes_x(3, 2);
    for (int k = 0; k < 3; k++) {
        const uint64_t sb = k == 1 ? t[0] + t[1] : ec_least_bytes(ls[k]);
        members_entry_write(frame.p + 32 + 32 * k, sb, 7, members_word(ws[k], 0, ms[k]), ls[k], ls[k]);
        total += sb;
    }
    pack_put64(frame.p + 32 + 96, t[0]); pack_put64(frame.p + 32 + 104, t[1]);
    members_header_write_x(frame.p, MEMBERS_VERSION_3, 16385 + 4003 + 5, 3, 2, frame.p + 32);
    Frame F;
    uint64_t bytes = 0;
    CHECK(frame_head_check(frame.p, total, &F) == PACK_OK && F.members && F.count == 3 && F.ext == 2 && F.fixed == 32 + 96 + 16);
    CHECK(frame_dir_check(frame.p + 32, F, total, true, &bytes) == PACK_OK && bytes == total);
    CHECK(!F.direct(0) && F.direct(1) && F.direct(2) && F.table.size() == 2 && F.table[0] == t[0] && F.table[1] == t[1]);
    CHECK(F.table_at[0] == 0 && F.table_at[1] == 0 && F.table_at[2] == 2 && F.table_at[3] == 2 && F.stream[1] == t[0] + t[1] && F.coded[2] == 4003);
    // a version-3 header is not one of the earlier versions, and the other way round
    MembersHeader M;
    CHECK(members_header_check(frame.p, total, &M) == PACK_FORMAT && members_header_check_v3(frame.p, total, &M) == PACK_OK);
    CHECK(members_header_check_v3(frame.p, members_fixed_bytes_x(3, 2) - 16, &M) == PACK_FORMAT);
}

int main()
{
    cut_checks();
    word_and_args_checks();
    frame_checks();
    printf("%ld checks ok\n", checks);
    return 0;
}
