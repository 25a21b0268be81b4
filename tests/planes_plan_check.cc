// planes_plan_check.cc -- stand-alone host program over bijective-bwt_amd/csrc/planes_plan.h, the tile and tail arithmetic that the
// byte-plane split's kernels share with the host, and over the version-3 frame predicates of pack_plan.h.  tests/test_planes_model.py
// builds it with -fsanitize=address,undefined and runs it: every buffer below is a heap block of exactly the size the checked function
// may touch.  Prints the number of checks and "ok"; exits 1 with the failing line otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "planes_plan.h"
#include "pack_plan.h"

static long checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        checks++;                                                                \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

typedef std::vector<uint8_t> Bytes;

// a heap block of exactly n bytes
struct Exact {
    uint8_t *p;
    explicit Exact(uint64_t n) : p((uint8_t *)malloc(n ? n : 1)) {}
    ~Exact() { free(p); }
};

static void width_checks()
{
    for (uint64_t w = 0; w < 40; w++) CHECK(planes_width_ok(w) == (w == 2 || w == 4 || w == 8));
    CHECK(!planes_width_ok(1ull << 32 | 4) && !planes_width_ok(~0ull));
    CHECK(planes_log_w(2) == 1 && planes_log_w(4) == 2 && planes_log_w(8) == 3);
    CHECK(planes_tile_bytes(2) == 8192 && planes_tile_bytes(4) == 16384 && planes_tile_bytes(8) == 32768);
}

// the serial split of L bytes against the literal double loop of the header, the join against the input, and the tiles against both
static void string_checks(uint64_t L, uint32_t w)
{
    Exact in(L), out(L), back(L), want(L);
    for (uint64_t i = 0; i < L; i++) { in.p[i] = (uint8_t)(i * 131 + (i >> 8) * 7 + w); out.p[i] = 0xEE; want.p[i] = 0xDD; }
    const uint64_t q = L / w;
    for (uint64_t k = 0; k < w; k++)
        for (uint64_t i = 0; i < q; i++) want.p[k * q + i] = in.p[i * w + k];
    for (uint64_t j = q * w; j < L; j++) want.p[j] = in.p[j];
    planes_split_serial(in.p, L, w, out.p);
    CHECK(memcmp(out.p, want.p, L) == 0);
    planes_join_serial(out.p, L, w, back.p);
    CHECK(memcmp(back.p, in.p, L) == 0);
    if (L < w) CHECK(memcmp(out.p, in.p, L) == 0);
    CHECK(planes_q(L, w) == q && planes_tail_at(L, w) == q * w && L - planes_tail_at(L, w) < w);
    // the tiles: ceil(L / T) of them, at least one; their elements follow each other, add up to q, and only the last may be short of E
    const uint64_t T = planes_tile_bytes(w), tiles = planes_tiles(L, w);
    CHECK(tiles == (L + T - 1) / T && tiles >= 1);
    uint64_t sum = 0;
    for (uint64_t j = 0; j < tiles; j++) {
        const uint32_t e = planes_tile_elems(L, w, j);
        CHECK(e <= PLANES_E && (e == PLANES_E || sum + e == q));
        // what the tile's workgroup touches lies inside the string: its interleaved bytes, and its piece of every plane
        CHECK((j * PLANES_E + e) * w <= planes_tail_at(L, w));
        for (uint64_t k = 0; k < w && e; k++) CHECK(k * q + j * PLANES_E + e <= (k + 1) * q);
        sum += e;
    }
    CHECK(sum == q);
    CHECK(planes_tile_elems(L, w, tiles) == 0);
}

static void boundary_checks()
{
    for (uint32_t w : {2u, 4u, 8u}) {
        const uint64_t T = planes_tile_bytes(w);
        for (uint64_t L = 1; L <= 40; L++) string_checks(L, w);
        const uint64_t lengths[] = {16ull * w - 1, 16ull * w, 16ull * w + 1, 4095, 4096, 4097, T - w, T - 1, T, T + 1, T + w - 1, T + w, 2 * T - 1, 2 * T, 2 * T + w + 1, 70001,
                                    3 * T + w - 1};
        for (uint64_t L : lengths)
            string_checks(L, w);
        // where a tile is there for the tail alone
        CHECK(planes_tiles(T + 1, w) == 2 && planes_tile_elems(T + 1, w, 1) == 0 && planes_tile_elems(T + 1, w, 0) == PLANES_E);
        CHECK(planes_tiles(T + w, w) == 2 && planes_tile_elems(T + w, w, 1) == 1);
        CHECK(planes_tiles(1, w) == 1 && planes_tile_elems(1, w, 0) == 0 && planes_tiles(w - 1, w) == 1);
        // beyond 2^32: nothing wraps
        const uint64_t big = (1ull << 32) + (1ull << 20) + 3;
        CHECK(planes_q(big, w) == big / w && planes_tiles(big, w) == (big + T - 1) / T);
        CHECK(planes_split_index(big, w, big - 1) == (big % w ? big - 1 : (w - 1) * (big / w) + big / w - 1));
        CHECK(planes_split_index(big, w, w + 1) == big / w + 1);
        CHECK(planes_tiles(PLANES_MAX_N, w) == PLANES_MAX_N / T && planes_tile_elems(PLANES_MAX_N, w, PLANES_MAX_N / T - 1) == PLANES_E);
    }
}

// ---- the version-3 frame predicates of pack_plan.h ----
static int judge(const Bytes &frame, bool exact, uint64_t *n, uint64_t *frame_bytes, uint32_t *width)
{
    Exact e(frame.size());
    memcpy(e.p, frame.data(), frame.size());
    PackHeader H;
    int rc = pack_header_check(e.p, frame.size(), &H);
    if (rc != PACK_OK) return rc;
    rc = pack_directory_check(e.p + PACK_HEADER_BYTES, H, frame.size(), exact, frame_bytes);
    if (rc == PACK_OK) { *n = H.n; *width = H.width; }
    return rc;
}

struct EntryV3 { uint64_t sb; uint32_t crc, width; uint64_t coded, rsv2; };

static Bytes make_frame(uint32_t version, uint64_t n, uint64_t B, const std::vector<EntryV3> &entries)
{
    uint64_t total = PACK_HEADER_BYTES + 32 * entries.size();
    for (const EntryV3 &e : entries) total += e.sb < (1ull << 20) ? e.sb : 0;
    Bytes f(total, 0);
    for (size_t k = 0; k < entries.size(); k++) {
        uint8_t *e = &f[PACK_HEADER_BYTES + 32 * k];
        pack_entry_write_v3(e, entries[k].sb, entries[k].crc, entries[k].coded, entries[k].width);
        pack_put64(e + 24, entries[k].rsv2);
    }
    pack_header_write_v(f.data(), version, n, B, &f[PACK_HEADER_BYTES]);
    return f;
}

static void frame_v3_checks()
{
    const uint64_t n = 2 * 4096 + 100, B = 4096;
    uint64_t got_n = 0, fb = 0;
    uint32_t width = 99;
    CHECK(pack_version_ok(1) && pack_version_ok(2) && pack_version_ok(3) && !pack_version_ok(0) && !pack_version_ok(4));
    CHECK(pack_version_asked_ok(1) && pack_version_asked_ok(2) && !pack_version_asked_ok(3));
    CHECK(pack_entry_bytes(3) == 32 && pack_fixed_bytes_v(3, 3) == 128);
    auto entries = [&](uint32_t w0, uint32_t w1, uint32_t w2) {
        return std::vector<EntryV3>{{ec_least_bytes(700) + 32, 11, w0, 700, 0}, {ec_bound_bytes(4096), 12, w1, 4096, 0}, {ec_least_bytes(1), 13, w2, 1, 0}};
    };
    for (uint32_t w : {2u, 4u, 8u}) {
        const Bytes f = make_frame(3, n, B, entries(w, w, w));
        CHECK(judge(f, true, &got_n, &fb, &width) == PACK_OK && got_n == n && fb == f.size() && width == w);
        // the same words under versions 1 (16-byte entries) and 2 (the word must be zero)
        CHECK(judge(make_frame(2, n, B, entries(w, w, w)), true, &got_n, &fb, &width) == PACK_FORMAT);
        CHECK(judge(make_frame(1, n, B, entries(w, w, w)), true, &got_n, &fb, &width) == PACK_FORMAT);
    }
    for (uint32_t w : {0u, 1u, 3u, 5u, 6u, 7u, 9u, 16u, 0x10004u, 0xFFFFFFFFu})
        CHECK(judge(make_frame(3, n, B, entries(w, w, w)), true, &got_n, &fb, &width) == PACK_FORMAT);
    CHECK(judge(make_frame(3, n, B, entries(4, 2, 4)), true, &got_n, &fb, &width) == PACK_FORMAT);          // two entries differ
    CHECK(judge(make_frame(3, n, B, entries(4, 4, 8)), true, &got_n, &fb, &width) == PACK_FORMAT);
    CHECK(judge(make_frame(3, n, B, entries(0, 4, 4)), true, &got_n, &fb, &width) == PACK_FORMAT);
    // version 2's rules hold on a version-3 frame
    auto with = [&](size_t k, EntryV3 e) { std::vector<EntryV3> v = entries(4, 4, 4); v[k] = e; return make_frame(3, n, B, v); };
    auto bad = [&](const Bytes &g) { return judge(g, false, &got_n, &fb, &width) == PACK_FORMAT; };
    CHECK(bad(with(1, {ec_bound_bytes(4096), 12, 4, 4096, 1})));             // the trailing word
    CHECK(bad(with(0, {ec_least_bytes(1), 11, 4, 0, 0})));                   // coded_bytes = 0
    CHECK(bad(with(0, {ec_least_bytes(4097), 11, 4, 4097, 0})));             // coded_bytes = block length + 1
    CHECK(bad(with(0, {ec_least_bytes(700) - 16, 11, 4, 700, 0})));
    CHECK(bad(with(0, {ec_least_bytes(700) + 8, 11, 4, 700, 0})));
    CHECK(bad(with(2, {1ull << 63, 13, 4, 1, 0})));
    CHECK(!bad(with(2, {ec_least_bytes(100), 13, 4, 100, 0})));
    // a width of versions 1 and 2 is reported as 0
    Bytes v2 = make_frame(2, n, B, entries(0, 0, 0));
    CHECK(judge(v2, true, &got_n, &fb, &width) == PACK_OK && width == 0);
    // ... and a version-2 body under a version word of 3, resealed, is no frame
    ec_put32(&v2[4], 3);
    ec_put32(&v2[28], crc32_bytes(v2.data(), 28));
    CHECK(judge(v2, true, &got_n, &fb, &width) == PACK_FORMAT);
}

int main()
{
    width_checks();
    boundary_checks();
    frame_v3_checks();
    printf("%ld checks ok\n", checks);
    return 0;
}
