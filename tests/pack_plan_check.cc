// pack_plan_check.cc -- the frame predicates and the CRC arithmetic of pack_plan.h as a host program of its own, for the sanitizers
// (tests/test_pack_model.py builds it with -fsanitize=address,undefined and runs it as a child process).
//
// argv[1]: a file of cases, each { i32 the answer the predicates must give (0, -5 or -8), u32 length, the frame's bytes }; the first
// case is a valid frame.  Every frame is judged from a heap block of exactly its length, so a predicate that reads past what
// in_bytes allows is caught; the valid frame is also cut at every length below 96, which must be refused without a read past the cut.
#include "pack_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// what an unpack (exact) or a step through concatenated frames (not exact) makes of header and directory
static int judge(const uint8_t *frame, uint64_t in_bytes, bool exact, uint64_t *n, uint64_t *frame_bytes)
{
    PackHeader H;
    int rc = pack_header_check(frame, in_bytes, &H);
    if (rc != PACK_OK) return rc;
    rc = pack_directory_check(frame + PACK_HEADER_BYTES, H, in_bytes, exact, frame_bytes);
    if (rc == PACK_OK) *n = H.n;
    return rc;
}

static int judge_copy(const uint8_t *bytes, uint64_t len, bool exact, uint64_t *n, uint64_t *frame_bytes)
{
    uint8_t *heap = (uint8_t *)malloc(len ? len : 1);
    memcpy(heap, bytes, len);
    const int rc = judge(heap, len, exact, n, frame_bytes);
    free(heap);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: pack_plan_check <cases>\n"); return 2; }
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fp)) > 0) file.insert(file.end(), buf, buf + got);
    fclose(fp);

    // CRC arithmetic
    CHECK(crc32_bytes((const uint8_t *)"123456789", 9) == 0xCBF43926u, "the check value of CRC-32");
    CHECK(crc32_bytes((const uint8_t *)"", 0) == 0u, "the empty string");
    CHECK(crc_mul(CRC_ONE, 0x12345678u) == 0x12345678u && crc_xpow8(0) == CRC_ONE, "one");
    for (uint32_t a = 1; a; a <<= 3) CHECK(crc_over_x(crc_times_x(a)) == a && crc_times_x(crc_over_x(a)) == a, "x and 1/x");
    for (uint64_t la : {0ull, 1ull, 5ull, 1000ull})
        for (uint64_t lb : {0ull, 1ull, 17ull, 4096ull}) {
            if (la + lb > file.size()) continue;
            CHECK(crc_combine(crc32_bytes(file.data(), la), crc32_bytes(file.data() + la, lb), lb) == crc32_bytes(file.data(), la + lb), "combine %llu %llu",
                  (unsigned long long)la, (unsigned long long)lb);
        }
    CHECK(crc_tiles(1) == 1 && crc_tiles(CRC_T) == 1 && crc_tiles(CRC_T + 1) == 2 && crc_groups(CRC_G) == 1 && crc_groups(CRC_G + 1) == 2, "tiles and groups");

    // blocks and bounds
    CHECK(pack_block_len(0, 0) == 0 && pack_block_len(PACK_MAX_N + 1, 0) == 0 && pack_block_len(5000, 4095) == 0, "bad arguments");
    CHECK(pack_block_len(10, 0) == 10 && pack_block_len(10, 3) == 0 && pack_block_len(3, 10) == 3 && pack_block_len(5000, 4096) == 4096 && pack_block_len(5000, 5000) == 5000, "block length");
    CHECK(pack_blocks(3 * 4096 + 1, 4096) == 4 && pack_block_at(3 * 4096 + 1, 4096, 3) == 1 && pack_block_at(3 * 4096 + 1, 4096, 2) == 4096, "blocks");
    CHECK(pack_bound_bytes(1, 1) == 48 + ec_bound_bytes(1), "bound of one byte");
    CHECK(pack_bound_bytes(3 * 4096 + 1, 4096) == 32 + 64 + 3 * ec_bound_bytes(4096) + ec_bound_bytes(1), "bound of four blocks");
    CHECK(pack_least_bytes(PACK_MAX_N, 4096) > pack_fixed_bytes(1u << 20) && pack_bound_bytes(PACK_MAX_N, 4096) > pack_least_bytes(PACK_MAX_N, 4096), "the largest frame");

    // the cases
    size_t at = 0, cases = 0;
    const uint8_t *valid = nullptr;
    uint64_t valid_len = 0;
    while (at + 8 <= file.size()) {
        int32_t want;
        uint32_t len;
        memcpy(&want, file.data() + at, 4);
        memcpy(&len, file.data() + at + 4, 4);
        at += 8;
        if (at + len > file.size()) { printf("cases file cut short\n"); return 2; }
        uint64_t n = 0, fb = 0;
        const int rc = judge_copy(file.data() + at, len, true, &n, &fb);
        CHECK(rc == want, "case %zu: %d, the model says %d", cases, rc, (int)want);
        if (rc == PACK_OK) CHECK(fb == len && n >= 1 && n <= PACK_MAX_N, "case %zu: frame_bytes %llu of %u", cases, (unsigned long long)fb, len);
        // with more bytes at hand than the frame has, the step finds the frame's own end
        if (want == PACK_OK) {
            std::vector<uint8_t> more(file.data() + at, file.data() + at + len);
            more.resize(len + 48, 0xEE);
            uint64_t n2 = 0, fb2 = 0;
            CHECK(judge_copy(more.data(), more.size(), false, &n2, &fb2) == PACK_OK && fb2 == len && n2 == n, "case %zu: stepping", cases);
            CHECK(judge_copy(more.data(), more.size(), true, &n2, &fb2) == PACK_FORMAT, "case %zu: exact with bytes behind", cases);
        }
        if (cases == 0) { valid = file.data() + at; valid_len = len; }
        at += len;
        cases++;
    }
    CHECK(cases >= 20 && valid && valid_len > 96, "%zu cases", cases);

    // a valid frame cut at every length below 96
    if (valid)
        for (uint64_t cut = 0; cut < 96 && cut < valid_len; cut++)
            for (int exact = 0; exact < 2; exact++) {
                uint64_t n = 0, fb = 0;
                CHECK(judge_copy(valid, cut, exact != 0, &n, &fb) == PACK_FORMAT, "cut at %llu", (unsigned long long)cut);
            }

    if (failures) { printf("%d checks FAILED\n", failures); return 1; }
    printf("%zu cases, checks ok\n", cases);
    return 0;
}
