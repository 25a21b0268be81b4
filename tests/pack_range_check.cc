// pack_range_check.cc -- the range plan of a "BWTZ" frame (pack_ranges_check, and ranges_plan over a judged Frame: members_plan.h) as
// a host program of its own, for the sanitizers (tests/test_pack_range_model.py builds it with -fsanitize=address,undefined and runs it as a child process).
//
// argv[1]: a file of cases, each { i32 the code the checks must give, u32 head_bytes, u64 in_bytes, u64 out_cap, u32 count, u32 words,
// head_bytes bytes: the frame's header and directory (all of the frame where those are refused), count (offset, bytes) pairs of u64,
// `words` u64 the model's plan: covered blocks, runs, covered bytes, stream bytes, coded bytes, output bytes, then the runs, the
// stream pieces and the output pieces }.  Frame head and ranges are judged from heap blocks of exactly their length, so a read past
// either is caught.  The first case is a valid frame of several blocks; it is paired here with ranges no model run could afford.
#include "members_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the library's order: header, directory, ranges, plan; the plan as the words of the cases file
static int judge(const uint8_t *head, uint64_t in_bytes, const PackRange *r, uint64_t count, uint64_t out_cap, std::vector<uint64_t> *words)
{
    Frame F;
    uint64_t frame = 0, sum = 0;
    int rc = frame_head_check(head, in_bytes, &F);
    if (rc != PACK_OK) return rc;
    rc = frame_dir_check(head + PACK_HEADER_BYTES, F, in_bytes, true, &frame);
    if (rc != PACK_OK) return rc;
    CHECK(!F.members && F.B == F.z.B && F.count == F.z.nblk, "a \"BWTZ\" frame, planned by dividing by B");
    rc = pack_ranges_check(F.n, r, count, out_cap, &sum);
    if (rc != PACK_OK) return rc;
    PackRangesPlan P;
    ranges_plan(F, r, count, &P);
    CHECK(P.out_bytes == sum && P.out.size() == count && P.runs.size() == P.streams.size(), "the plan's own sums");
    uint64_t blocks = 0, gathered = 0;
    for (size_t i = 0; i < P.runs.size(); i++) {
        CHECK(P.runs[i].blocks >= 1 && P.runs[i].first + P.runs[i].blocks <= F.count, "run %zu inside the frame", i);
        if (i) CHECK(P.runs[i - 1].first + P.runs[i - 1].blocks < P.runs[i].first, "runs %zu and %zu sorted and maximal", i - 1, i);
        CHECK(P.streams[i].dst == gathered && P.streams[i].src + P.streams[i].bytes <= in_bytes, "stream piece %zu", i);
        blocks += P.runs[i].blocks;
        gathered += P.streams[i].bytes;
    }
    CHECK(blocks == P.blocks.size() && gathered == P.stream_bytes && P.covered_bytes <= F.n && P.coded_bytes <= P.covered_bytes, "covered sums");
    for (size_t i = 0; i < P.out.size(); i++)
        CHECK(P.out[i].bytes == r[i].bytes && P.out[i].src + P.out[i].bytes <= P.covered_bytes && P.out[i].dst + P.out[i].bytes <= sum, "output piece %zu", i);
    if (words) {
        *words = {(uint64_t)P.blocks.size(), (uint64_t)P.runs.size(), P.covered_bytes, P.stream_bytes, P.coded_bytes, P.out_bytes};
        for (const PackRun &x : P.runs) { words->push_back(x.first); words->push_back(x.blocks); }
        for (const PackPiece &x : P.streams) { words->push_back(x.src); words->push_back(x.dst); words->push_back(x.bytes); }
        for (const PackPiece &x : P.out) { words->push_back(x.src); words->push_back(x.dst); words->push_back(x.bytes); }
    }
    return PACK_OK;
}

static int judge_copy(const uint8_t *head, uint64_t head_bytes, uint64_t in_bytes, const uint64_t *pairs, uint64_t count, uint64_t out_cap,
                      std::vector<uint64_t> *words)
{
    uint8_t *h = (uint8_t *)malloc(head_bytes ? head_bytes : 1);
    PackRange *r = (PackRange *)malloc(count ? count * sizeof(PackRange) : 1);
    memcpy(h, head, head_bytes);
    if (count) memcpy(r, pairs, count * sizeof(PackRange));
    const int rc = judge(h, in_bytes, count ? r : nullptr, count, out_cap, words);
    free(r);
    free(h);
    return rc;
}

int main(int argc, char **argv)
{
    static_assert(sizeof(PackRange) == 16, "two words");
    if (argc != 2) { printf("usage: pack_range_check <cases>\n"); return 2; }
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fp)) > 0) file.insert(file.end(), buf, buf + got);
    fclose(fp);

    CHECK(pieces_tiles(1, 0) == 1 && pieces_tiles(PIECES_T, 0) == 1 && pieces_tiles(PIECES_T + 1, 0) == 2 && PIECES_T % PIECES_LINE == 0, "tiles of a piece");
    CHECK(pieces_tiles(PIECES_T - 255, 255) == 1 && pieces_tiles(PIECES_T - 254, 255) == 2 && pieces_tiles(2 * PIECES_T - 255, 255) == 2 && pieces_tiles(2 * PIECES_T, 255) == 3, "a first tile that ends at a line");

    size_t at = 0, cases = 0, planned = 0;
    std::vector<uint8_t> valid;
    uint64_t valid_in_bytes = 0;
    while (at + 32 <= file.size()) {
        int32_t want;
        uint32_t head_bytes, count, nwords;
        uint64_t in_bytes, out_cap;
        memcpy(&want, file.data() + at, 4); memcpy(&head_bytes, file.data() + at + 4, 4);
        memcpy(&in_bytes, file.data() + at + 8, 8); memcpy(&out_cap, file.data() + at + 16, 8);
        memcpy(&count, file.data() + at + 24, 4); memcpy(&nwords, file.data() + at + 28, 4);
        at += 32;
        if (at + head_bytes + 16ull * count + 8ull * nwords > file.size()) { printf("cases file cut short\n"); return 2; }
        const uint8_t *head = file.data() + at;
        std::vector<uint64_t> pairs(2 * (size_t)count + 1), model((size_t)nwords), words;
        if (count) memcpy(pairs.data(), head + head_bytes, 16 * (size_t)count);
        if (nwords) memcpy(model.data(), head + head_bytes + 16 * (size_t)count, 8 * (size_t)nwords);
        const int rc = judge_copy(head, head_bytes, in_bytes, pairs.data(), count, out_cap, &words);
        CHECK(rc == want, "case %zu: %d, the model says %d", cases, rc, (int)want);
        if (rc == PACK_OK && want == PACK_OK) {
            CHECK(words == model, "case %zu: the plan is not the model's", cases);
            planned++;
            if (valid.empty()) { valid.assign(head, head + head_bytes); valid_in_bytes = in_bytes; }
        }
        at += head_bytes + 16 * (size_t)count + 8 * (size_t)nwords;
        cases++;
    }
    CHECK(cases >= 50 && planned >= 30 && !valid.empty(), "%zu cases, %zu planned", cases, planned);

    // a valid directory with hostile ranges
    if (!valid.empty()) {
        PackHeader H;
        CHECK(pack_header_check(valid.data(), valid_in_bytes, &H) == PACK_OK && H.nblk >= 2, "the first case is a frame of several blocks");
        const uint64_t big = ~0ull, n = H.n;
        const uint64_t overflow[][2] = {{big, 1}, {big, 2}, {1, big}, {big, big}, {big - 1, 2}, {n, 1}, {0, n + 1}, {n - 1, 2}, {1ull << 63, 1ull << 63}, {0, big}};
        for (const auto &o : overflow) CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, o, 1, big, nullptr) == PACK_RANGE, "range (%llu, %llu)", (unsigned long long)o[0], (unsigned long long)o[1]);
        const uint64_t zero[2][2] = {{big, 1}, {5, 0}};
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, zero[0], 2, big, nullptr) == PACK_ARG, "a range of no bytes comes before one that leaves the input");
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, nullptr, 0, big, nullptr) == PACK_ARG, "no ranges");
        // 2^20 one-byte ranges, all in block 1; one more is refused
        std::vector<uint64_t> many(2 * (PACK_MAX_RANGES + 1));
        for (uint64_t i = 0; i <= PACK_MAX_RANGES; i++) { many[2 * i] = H.B + i % 7; many[2 * i + 1] = 1; }
        std::vector<uint64_t> words;
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, many.data(), PACK_MAX_RANGES, big, &words) == PACK_OK, "2^20 ranges");
        CHECK(words.size() == 6 + 5 + 3 * PACK_MAX_RANGES && words[0] == 1 && words[1] == 1 && words[5] == PACK_MAX_RANGES && words[6] == 1 && words[7] == 1, "2^20 ranges cover one block");
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, many.data(), PACK_MAX_RANGES, PACK_MAX_RANGES - 1, nullptr) == PACK_SPACE, "2^20 bytes into less");
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, many.data(), PACK_MAX_RANGES + 1, big, nullptr) == PACK_RANGE, "2^20 + 1 ranges");
        // the whole input 2^20 times would be far more than 2^32 bytes only for a large n; here the sum is checked as it stands
        for (uint64_t i = 0; i < PACK_MAX_RANGES; i++) { many[2 * i] = 0; many[2 * i + 1] = n; }
        const int rc = judge_copy(valid.data(), valid.size(), valid_in_bytes, many.data(), PACK_MAX_RANGES, big, nullptr);
        CHECK(rc == (n * PACK_MAX_RANGES > PACK_MAX_RANGE_BYTES ? PACK_RANGE : PACK_OK), "the sum of 2^20 whole reads: %d", rc);
    }

    if (failures) { printf("%d checks FAILED\n", failures); return 1; }
    printf("%zu cases, checks ok\n", cases);
    return 0;
}
