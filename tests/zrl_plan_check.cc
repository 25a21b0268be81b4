// zrl_plan_check.cc -- stand-alone host program over bijective-bwt_amd/csrc/zrl_plan.h, the arithmetic and validation that the zero-run
// stage's kernels share with the host, and over the version-2 frame predicates of pack_plan.h.  tests/test_zrl_model.py builds it with
// -fsanitize=address,undefined and runs it: every buffer below is a heap block of exactly the size the checked function may touch, so
// a read past a cut input aborts the program.  Prints the number of checks and "ok"; exits 1 with the failing line otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "zrl_plan.h"
#include "pack_plan.h"

static long checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        checks++;                                                                \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

typedef std::vector<uint8_t> Bytes;

// a heap copy of exactly `bytes` bytes of v: the sanitizer sees the input's true end
struct Exact {
    uint8_t *p;
    uint64_t bytes;
    Exact(const Bytes &v, uint64_t n) : p((uint8_t *)malloc(n ? n : 1)), bytes(n) { if (n) memcpy(p, v.data(), n); }
    ~Exact() { free(p); }
};

static uint32_t check_coded(const Bytes &z, uint64_t n)
{
    Exact e(z, z.size());
    return zrl_check(e.p, e.bytes, n);
}

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static void digit_checks()
{
    CHECK(zrl_digits(1) == 1 && zrl_digits(2) == 1 && zrl_digits(3) == 2 && zrl_digits(6) == 2 && zrl_digits(7) == 3);
    CHECK(zrl_digits((1ull << 36) - 2) == 35 && zrl_digits((1ull << 36) - 1) == 36 && zrl_digits(1ull << 36) == 36);
    for (uint64_t L = 1; L < 5000; L++) {
        uint64_t sum = 0;
        const uint32_t k = zrl_digits(L);
        for (uint32_t i = 0; i < k; i++) sum += (uint64_t)(zrl_digit(L, i) + 1) << i;
        CHECK(sum == L);
        // the header's rule: d = (L - 1) & 1, L = (L - 1 - d) >> 1
        uint64_t l = L;
        for (uint32_t i = 0; i < k; i++) {
            const uint32_t d = (uint32_t)((l - 1) & 1);
            CHECK(d == zrl_digit(L, i));
            l = (l - 1 - d) >> 1;
        }
        CHECK(l == 0);
    }
    CHECK(zrl_tiles(1) == 1 && zrl_tiles(ZRL_T) == 1 && zrl_tiles(ZRL_T + 1) == 2 && zrl_tiles(ZRL_MAX_N) == ZRL_MAX_N / ZRL_T);
}

static void malformed_checks()
{
    const Bytes good = {5, 0, 1, 3, 255, 1, 0, 0};       // 4, five zeros, 2, 255, three zeros: 11 ranks
    CHECK(check_coded(good, 11) == 0);
    CHECK(check_coded(good, 12) == ZRL_BAD_SUM);                     // a sum of n - 1
    CHECK(check_coded(good, 10) == ZRL_BAD_SUM);                     // a sum of n + 1
    CHECK(check_coded({5, 0, 255}, 40) & ZRL_BAD_END);               // a 255 at the end
    CHECK(check_coded({5, 255, 2, 0, 0}, 40) & ZRL_BAD_PAYLOAD);     // a 255 followed by 2
    Bytes many(42, 0);
    many[0] = 7; many[41] = 9;
    CHECK(check_coded(many, 4096) != 0);                             // 40 digits in a row
    CHECK(check_coded(many, 1ull << 36) & ZRL_BAD_DIGIT);
    CHECK(check_coded(Bytes(36, 0), 100) == ZRL_BAD_SUM);            // a digit of index 35, n = 100
    CHECK(check_coded(Bytes(36, 0), (1ull << 36) - 1) == 0);         // ... which is what the 36 digits stand for
    CHECK(check_coded(Bytes(36, 1), (1ull << 37) - 2) == 0);
    CHECK(check_coded(Bytes(37, 0), (1ull << 37) - 1) & ZRL_BAD_DIGIT);
    CHECK(check_coded({255, 255, 0}, 2) & ZRL_BAD_PAYLOAD);          // the second 255 is a payload
    CHECK(check_coded({255, 1, 255, 0, 0}, 3) == 0);                 // 255, 254, one zero: the digit behind a payload has index 0
    // every prefix of a good input, from a block of exactly its length
    for (uint64_t cut = 1; cut < good.size(); cut++) {
        Exact e(good, cut);
        CHECK(zrl_check(e.p, cut, 11) != 0);
    }
}

// the serial encoder and decoder against each other, and a decoder that starts anew at every multiple of `chunk` from zrl_state_at
// against the serial one: what the kernels' threads do
static void round_trip(const Bytes &r, uint64_t chunk)
{
    const uint64_t n = r.size();
    Exact in(r, n);
    const uint64_t m = zrl_encode_serial(in.p, n, nullptr);
    Exact z(Bytes(m, 0xEE), m);
    CHECK(zrl_encode_serial(in.p, n, z.p) == m);
    if (m >= n) return;
    CHECK(zrl_check(z.p, m, n) == 0);
    Exact out(Bytes(n, 0xEE), n);
    zrl_decode_serial(z.p, m, out.p, n);
    CHECK(memcmp(out.p, in.p, n) == 0);
    Exact out2(Bytes(n, 0), n);
    uint64_t at = 0;
    for (uint64_t p0 = 0; p0 < m; p0 += chunk) {
        zrl_state s = zrl_state_at(z.p, p0);
        s.pos = at;
        for (uint64_t p = p0; p < m && p < p0 + chunk; p++) {
            const uint64_t here = s.pos;
            const uint32_t v = zrl_step(s, z.p[p]);
            if (v) { CHECK(here < n); out2.p[here] = (uint8_t)v; }
        }
        CHECK(s.err == 0);
        at = s.pos;
    }
    CHECK(at == n && memcmp(out2.p, in.p, n) == 0);
}

static void round_trip_checks()
{
    for (int kind = 0; kind < 6; kind++) {
        for (uint64_t n : {1ull, 2ull, 3ull, 63ull, 64ull, 65ull, 1000ull, 70001ull}) {
            Bytes r(n);
            for (uint64_t i = 0; i < n; i++) {
                const uint32_t x = rnd();
                switch (kind) {
                case 0: r[i] = 0; break;
                case 1: r[i] = (x & 255) < 250 ? 0 : (uint8_t)(x >> 8); break;
                case 2: r[i] = (x & 3) ? 0 : (uint8_t)(253 + (x >> 8) % 3); break;
                case 3: r[i] = (uint8_t)(x >> 8); break;
                case 4: r[i] = (x & 1) ? 0 : 1; break;
                default: r[i] = i == 0 ? 113 : 0; break;
                }
            }
            for (uint64_t chunk : {1ull, 7ull, 64ull}) round_trip(r, chunk);
        }
    }
    // runs of 2^k - 2, 2^k - 1 and 2^k zeros, single ranks between them
    Bytes r;
    for (int k = 1; k <= 16; k++)
        for (uint64_t L : {(1ull << k) - 2, (1ull << k) - 1, 1ull << k}) {
            r.insert(r.end(), L, 0);
            r.push_back((uint8_t)(1 + k));
        }
    round_trip(r, 64);
    round_trip(r, 5);
}

// ---- the version-2 frame predicates of pack_plan.h ----
// what an unpack (exact) or a step through concatenated frames makes of header and directory, from a heap block of exactly `bytes`
static int judge(const Bytes &frame, uint64_t bytes, bool exact, uint64_t *n, uint64_t *frame_bytes)
{
    Exact e(frame, bytes);
    PackHeader H;
    int rc = pack_header_check(e.p, bytes, &H);
    if (rc != PACK_OK) return rc;
    rc = pack_directory_check(e.p + PACK_HEADER_BYTES, H, bytes, exact, frame_bytes);
    if (rc == PACK_OK) *n = H.n;
    return rc;
}

struct EntryV2 { uint64_t sb; uint32_t crc, rsv; uint64_t coded, rsv2; };

// header and directory of a frame of the given version over entries of 32 bytes, both CRCs right, the streams as zeros behind them
static Bytes make_frame(uint32_t version, uint64_t n, uint64_t B, const std::vector<EntryV2> &entries)
{
    uint64_t total = PACK_HEADER_BYTES + 32 * entries.size();
    for (const EntryV2 &e : entries) total += e.sb < (1ull << 20) ? e.sb : 0;
    Bytes f(total, 0);
    for (size_t k = 0; k < entries.size(); k++) {
        uint8_t *e = &f[PACK_HEADER_BYTES + 32 * k];
        pack_entry_write_v2(e, entries[k].sb, entries[k].crc, entries[k].coded);
        ec_put32(e + 12, entries[k].rsv); pack_put64(e + 24, entries[k].rsv2);
    }
    uint8_t *h = f.data();
    ec_put32(h, PACK_MAGIC); ec_put32(h + 4, version); pack_put64(h + 8, n); pack_put64(h + 16, B);
    ec_put32(h + 24, crc32_bytes(h + PACK_HEADER_BYTES, 32 * entries.size()));
    ec_put32(h + 28, crc32_bytes(h, 28));
    return f;
}

static void frame_v2_checks()
{
    const uint64_t n = 2 * 4096 + 100, B = 4096;
    const std::vector<EntryV2> good = {{ec_least_bytes(700) + 32, 11, 0, 700, 0}, {ec_bound_bytes(4096), 12, 0, 4096, 0}, {ec_least_bytes(1), 13, 0, 1, 0}};
    const Bytes f = make_frame(2, n, B, good);
    uint64_t got_n = 0, fb = 0;
    CHECK(pack_fixed_bytes_v(2, 3) == 128 && pack_fixed_bytes_v(1, 3) == pack_fixed_bytes(3) && pack_entry_bytes(2) == 32 && pack_entry_bytes(1) == 16);
    CHECK(pack_bound_bytes_v2(n, B) == 32 + 32 * 3 + 2 * ec_bound_bytes(4096) + ec_bound_bytes(100) && pack_bound_bytes_v2(n, B) == pack_bound_bytes(n, B) + 48);
    CHECK(pack_least_bytes_v2(n, B) == 128 + 3 * ec_least_bytes(1));
    CHECK(judge(f, f.size(), true, &got_n, &fb) == PACK_OK && got_n == n && fb == f.size());
    Bytes longer = f;
    longer.insert(longer.end(), 64, 0);
    CHECK(judge(longer, longer.size(), false, &got_n, &fb) == PACK_OK && fb == f.size());
    CHECK(judge(longer, longer.size(), true, &got_n, &fb) == PACK_FORMAT);
    // the valid frame cut at every length below 128, each from a heap block of exactly its length: the directory is not read
    for (uint64_t cut = 0; cut < 128; cut++) CHECK(judge(f, cut, false, &got_n, &fb) == PACK_FORMAT);
    for (uint64_t cut = 128; cut < f.size(); cut += 16) CHECK(judge(f, cut, false, &got_n, &fb) == PACK_FORMAT);
    // the malformed list
    auto with = [&](size_t k, EntryV2 e) { std::vector<EntryV2> v = good; v[k] = e; return make_frame(2, n, B, v); };
    auto bad = [&](const Bytes &g) { return judge(g, g.size(), false, &got_n, &fb) == PACK_FORMAT; };
    CHECK(bad(with(1, {ec_bound_bytes(4096), 12, 1, 4096, 0})));             // the first reserved word
    CHECK(bad(with(1, {ec_bound_bytes(4096), 12, 0, 4096, 1})));             // the second reserved word
    CHECK(bad(with(1, {ec_bound_bytes(4096), 12, 0, 4096, 1ull << 63})));
    CHECK(bad(with(0, {ec_least_bytes(1), 11, 0, 0, 0})));                   // coded_bytes = 0
    CHECK(bad(with(0, {ec_least_bytes(4097), 11, 0, 4097, 0})));             // coded_bytes = block length + 1
    CHECK(bad(with(2, {ec_least_bytes(101), 13, 0, 101, 0})));               // ... of the short last block
    CHECK(!bad(with(2, {ec_least_bytes(100), 13, 0, 100, 0})));
    CHECK(bad(with(0, {ec_least_bytes(700) - 16, 11, 0, 700, 0})));          // stream_bytes below the coder's least for coded_bytes
    CHECK(bad(with(0, {(ec_bound_bytes(700) & ~15ull) + 16, 11, 0, 700, 0})));          // ... above its bound, though within the block's
    CHECK(!bad(with(0, {ec_bound_bytes(700) & ~15ull, 11, 0, 700, 0})));
    CHECK(bad(with(0, {ec_least_bytes(700) + 8, 11, 0, 700, 0})));           // not a multiple of 16
    CHECK(bad(with(2, {1ull << 63, 13, 0, 1, 0})));
    CHECK(bad(make_frame(3, n, B, good)) && bad(make_frame(0, n, B, good)));  // any other version
    CHECK(bad(make_frame(1, n, B, good)));                                    // version 1 over 32-byte entries
    Bytes g = f;
    g[PACK_HEADER_BYTES + 32 + 16] ^= 1;                                      // a directory byte changed, the CRC left
    CHECK(bad(g));
    g = f;
    g[9] ^= 1;                                                                // a header byte changed
    CHECK(bad(g));
    // a version-1 body whose version word says 2, resealed: its directory CRC covers 16-byte entries
    Bytes v1(PACK_HEADER_BYTES + 48 + 3 * ec_least_bytes(100), 0);
    for (int k = 0; k < 3; k++) pack_entry_write(&v1[PACK_HEADER_BYTES + 16 * k], ec_least_bytes(100), 7);
    pack_header_write(v1.data(), 300, 100, &v1[PACK_HEADER_BYTES]);
    CHECK(judge(v1, v1.size(), true, &got_n, &fb) == PACK_FORMAT);            // (B = 100 < 4096 with B != n)
    v1.assign(PACK_HEADER_BYTES + 48 + 2 * ec_least_bytes(4096) + ec_least_bytes(100), 0);
    pack_entry_write(&v1[PACK_HEADER_BYTES], ec_least_bytes(4096), 7);
    pack_entry_write(&v1[PACK_HEADER_BYTES + 16], ec_least_bytes(4096), 8);
    pack_entry_write(&v1[PACK_HEADER_BYTES + 32], ec_least_bytes(100), 9);
    pack_header_write(v1.data(), n, B, &v1[PACK_HEADER_BYTES]);
    CHECK(judge(v1, v1.size(), true, &got_n, &fb) == PACK_OK && got_n == n);
    ec_put32(&v1[4], 2);
    ec_put32(&v1[28], crc32_bytes(v1.data(), 28));
    CHECK(judge(v1, v1.size(), true, &got_n, &fb) == PACK_FORMAT);
}

int main()
{
    digit_checks();
    malformed_checks();
    round_trip_checks();
    frame_v2_checks();
    printf("%ld checks ok\n", checks);
    return 0;
}
