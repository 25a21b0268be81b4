// delta_plan_check.cc -- stand-alone host program over bijective-bwt_amd/csrc/delta_plan.h, the arithmetic that the delta filter's
// kernels share with the host, and over the version-2 predicates of members_plan.h.  tests/test_delta_model.py builds it with
// -fsanitize=address,undefined and runs it: every buffer below is a heap block of exactly the size the checked function may touch.
// Prints the number of checks and "ok"; exits 1 with the failing line otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "delta_plan.h"
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

static void predicate_checks()
{
    for (uint64_t w = 0; w < 40; w++) CHECK(delta_width_ok(w) == (w == 1 || w == 2 || w == 4 || w == 8));
    for (uint64_t f = 0; f < 40; f++) CHECK(delta_filter_ok(f) == (f <= 1));
    CHECK(!delta_width_ok(1ull << 32 | 4) && !delta_filter_ok(1ull << 32) && !delta_filter_ok(~0ull));
    CHECK(delta_log_w(1) == 0 && delta_log_w(2) == 1 && delta_log_w(4) == 2 && delta_log_w(8) == 3);
    CHECK(delta_mask(1) == 0xFF && delta_mask(2) == 0xFFFF && delta_mask(4) == 0xFFFFFFFFull && delta_mask(8) == ~0ull);
    CHECK(delta_tile_bytes(1) == 4096 && delta_tile_bytes(8) == 32768 && delta_word(4, 1) == 0x104 && delta_word(8, 0) == 8);
}

// the zigzag by the header's words: 0, -1, 1, -2, ... become 0, 1, 2, 3, ...; the most negative difference is the largest code
static void zigzag_checks()
{
    for (uint32_t w : WIDTHS) {
        const uint64_t m = delta_mask(w), top = 1ull << (8 * w - 1);
        CHECK(delta_zigzag(0, w) == 0 && delta_zigzag(m, w) == 1 && delta_zigzag(1, w) == 2 && delta_zigzag(m - 1, w) == 3);
        CHECK(delta_zigzag(top, w) == m && delta_zigzag(top - 1, w) == m - 1);
        for (uint64_t k = 0; k < 70000; k++) {
            const uint64_t d = (k * 0x9E3779B97F4A7C15ull + (k << 7)) & m;
            CHECK(delta_unzigzag(delta_zigzag(d, w), w) == d && delta_zigzag(delta_unzigzag(d, w), w) == d);
        }
    }
}

// the serial statements over L bytes against the definition spelled out with 128-bit-free plain loops, both ways, and the tiles
static void string_checks(uint64_t L, uint32_t w, int kind)
{
    Exact in(L), out(L), back(L), want(L);
    for (uint64_t i = 0; i < L; i++) {
        in.p[i] = kind == 0 ? (uint8_t)(i * 131 + (i >> 8) * 7 + w) : (kind == 1 ? 0xFF : (uint8_t)((i % w) == w - 1 ? 0x80 : 0));
        out.p[i] = 0xEE; want.p[i] = 0xDD;
    }
    const uint64_t q = L / w, m = delta_mask(w);
    uint64_t prev = 0;
    for (uint64_t i = 0; i < q; i++) {
        uint64_t a = 0;
        for (uint32_t k = 0; k < w; k++) a |= (uint64_t)in.p[i * w + k] << (8 * k);
        const uint64_t d = (a - prev) & m;
        const uint64_t z = (d >> (8 * w - 1)) ? ((~d << 1) | 1) & m : (d << 1) & m;        // negative: 2 (-d) - 1 = ((not d) << 1) + 1
        for (uint32_t k = 0; k < w; k++) want.p[i * w + k] = (uint8_t)(z >> (8 * k));
        prev = a;
    }
    for (uint64_t j = q * w; j < L; j++) want.p[j] = in.p[j];
    delta_encode_serial(in.p, L, w, out.p);
    CHECK(memcmp(out.p, want.p, L) == 0);
    delta_decode_serial(out.p, L, w, back.p);
    CHECK(memcmp(back.p, in.p, L) == 0);
    // every byte string is a valid input of the decoder too
    delta_decode_serial(in.p, L, w, out.p);
    delta_encode_serial(out.p, L, w, back.p);
    CHECK(memcmp(back.p, in.p, L) == 0);
    if (L < w) CHECK(memcmp(out.p, in.p, L) == 0);
    CHECK(delta_q(L, w) == q && delta_tail_at(L, w) == q * w && L - delta_tail_at(L, w) < w);
    // the tiles: ceil(L / T) of them; their elements follow each other, add up to q, and only the last may be short of E
    const uint64_t T = delta_tile_bytes(w), tiles = delta_tiles(L, w);
    CHECK(tiles == (L + T - 1) / T && (L == 0 || tiles >= 1));
    uint64_t sum = 0;
    for (uint64_t j = 0; j < tiles; j++) {
        const uint32_t e = delta_tile_elems(L, w, j);
        CHECK(e <= PLANES_E && (e == PLANES_E || sum + e == q));
        CHECK((j * PLANES_E + e) * w <= delta_tail_at(L, w));
        sum += e;
    }
    CHECK(sum == q && delta_tile_elems(L, w, tiles) == 0);
    CHECK(delta_tiles_f(L, w, DELTA_FILTER_DELTA) == tiles && delta_tiles_f(L, w, DELTA_FILTER_NONE) == (L + PLANES_COPY_T - 1) / PLANES_COPY_T);
}

// the cut of a mixed call: every segment's tiles one after the other
static void cut_checks()
{
    const uint64_t lengths[6] = {1, 4097, 70001, 32768, 32769, 9};
    const uint32_t widths[6] = {8, 1, 4, 2, 8, 4}, filters[6] = {1, 1, 0, 0, 1, 0};
    uint64_t off[7] = {0}, first[7];
    for (int s = 0; s < 6; s++) off[s + 1] = off[s] + lengths[s];
    const uint64_t tiles = delta_cut_f(off, widths, filters, 6, first);
    const uint64_t want[7] = {0, 1, 3, 6, 7, 9, 10};
    CHECK(tiles == 10 && memcmp(first, want, sizeof want) == 0);
}

// version 2 of the member frame: the word, the argument check, and a directory judged under both versions
static void members_checks()
{
    CHECK(members_word_ok(4, MEMBERS_VERSION) && !members_word_ok(0x104, MEMBERS_VERSION) && members_word_ok(0x104, MEMBERS_VERSION_2));
    CHECK(members_word_ok(1, MEMBERS_VERSION_2) && !members_word_ok(0x204, MEMBERS_VERSION_2) && !members_word_ok(0x10104, MEMBERS_VERSION_2));
    CHECK(!members_word_ok(0x103, MEMBERS_VERSION_2) && !members_word_ok(0x80000104u, MEMBERS_VERSION_2) && !members_word_ok(0x100, MEMBERS_VERSION_2));
    const uint64_t ls[3] = {5, 4096, 9};
    const uint32_t ws[3] = {1, 4, 8}, fs[3] = {0, 1, 0}, none[3] = {0, 0, 0}, bad[3] = {0, 2, 0};
    uint64_t n = 0;
    CHECK(members_args_check_f(ls, ws, fs, 3, &n) == PACK_OK && n == 4110 && members_args_check_f(ls, ws, nullptr, 3, &n) == PACK_OK);
    CHECK(members_args_check_f(ls, ws, bad, 3, &n) == PACK_ARG && members_args_check_f(ls, nullptr, fs, 3, &n) == PACK_OK);
    CHECK(members_any_filter(fs, 3) && !members_any_filter(none, 3) && !members_any_filter(nullptr, 3));
    // a frame of three members, the streams' sizes the least the coder can make; dir and head are heap blocks of exactly their size
    for (int variant = 0; variant < 6; variant++) {
        Exact head(MEMBERS_HEADER_BYTES), dir(3 * MEMBERS_ENTRY_BYTES);
        uint64_t total = members_fixed_bytes(3);
        for (int k = 0; k < 3; k++) {
            uint32_t word = delta_word(ws[k], fs[k]);
            if (variant == 1) word = ws[k];                         // no filter anywhere
            if (variant == 3 && k == 1) word = delta_word(4, 2);    // a filter there is none of
            if (variant == 4 && k == 2) word |= 1u << 16;           // a bit above the filter
            const uint64_t sb = ec_least_bytes(ls[k]);
            members_entry_write(dir.p + MEMBERS_ENTRY_BYTES * k, sb, 0x12345678u, word, ls[k], ls[k]);
            total += sb;
        }
        const uint32_t version = variant == 2 || variant == 5 ? MEMBERS_VERSION : MEMBERS_VERSION_2;
        if (variant == 5)                                            // version 1 and plain widths: as it always was
            for (int k = 0; k < 3; k++) members_entry_write(dir.p + MEMBERS_ENTRY_BYTES * k, ec_least_bytes(ls[k]), 0x12345678u, ws[k], ls[k], ls[k]);
        members_header_write_v(head.p, version, 4110, 3, dir.p);
        MembersHeader M;
        uint64_t frame = 0;
        CHECK(members_header_check(head.p, total, &M) == PACK_OK && M.version == version && M.count == 3);
        const int rc = members_directory_check(dir.p, M, total, true, &frame);
        // 0: sound; 1: version 2 without a filter; 2: a filter under version 1; 3, 4: a bad word; 5: sound version 1
        CHECK(rc == (variant == 0 || variant == 5 ? PACK_OK : PACK_FORMAT));
        if (rc == PACK_OK) {
            CHECK(frame == total && members_entry_width(dir.p, 1) == 4 && members_entry_filter(dir.p, 1) == (variant == 0 ? 1u : 0u));
            CHECK(members_entry_filter(dir.p, 0) == 0 && members_entry_width(dir.p, 2) == 8);
        }
    }
    Exact head(MEMBERS_HEADER_BYTES), dir(MEMBERS_ENTRY_BYTES);
    members_entry_write(dir.p, ec_least_bytes(7), 1, 1, 7, 7);
    members_header_write_v(head.p, 3, 7, 1, dir.p);
    MembersHeader M;
    CHECK(members_header_check(head.p, 64 + ec_least_bytes(7) - 32, &M) == PACK_FORMAT);
}

int main()
{
    predicate_checks();
    zigzag_checks();
    const uint64_t extra[] = {0, 1, 4095, 4096, 4097, 70001};
    for (uint32_t w : WIDTHS)
        for (int kind = 0; kind < 3; kind++) {
            for (uint64_t L = 0; L <= 40; L++) string_checks(L, w, kind);
            for (uint64_t L : extra) { string_checks(L * w + w - 1, w, kind); string_checks(L * w, w, kind); }
        }
    cut_checks();
    members_checks();
    printf("%ld checks ok\n", checks);
    return 0;
}
