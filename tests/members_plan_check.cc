// members_plan_check.cc -- the predicates and the range plan of members_plan.h as a host program of its own, for the sanitizers
// (tests/test_pack_members_model.py builds it with -fsanitize=address,undefined and runs it as a child process).
//
// argv[1]: a file of cases in the layout of pack_range_check.cc, each { i32 the code the checks must give, u32 head_bytes, u64 in_bytes,
// u64 out_cap, u32 count, u32 words, head_bytes bytes: the frame's header and directory (all of the frame where those are refused),
// count (offset, bytes) pairs of u64, `words` u64 the model's plan }.  Frame head and ranges are judged from heap blocks of exactly
// their length, so a read past either is caught.  The first case is a valid member frame of several members; it is cut here at every
// length below 128 and paired with hostile ranges and indices.
// argv[2]: the cases file of pack_range_check.cc ("BWTZ" frames), each planned by division and by bisection (both_ways_cases).
#include "members_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int failures = 0;
static size_t both_ways = 0;        // plans of "BWTZ" frames made by division and by bisection, and compared
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the library's order: header, directory, ranges (or indices), plan; the plan as the words of the cases file
static int judge(const uint8_t *head, uint64_t in_bytes, const PackRange *r, const uint64_t *indices, uint64_t count, uint64_t out_cap,
                 std::vector<uint64_t> *words)
{
    Frame H;
    uint64_t sum = 0;
    PackRangesPlan P;
    std::vector<PackRange> whole;
    const PackRange *rs = nullptr;
    const int rc = frame_ranges_plan(head, in_bytes, r, indices, count, out_cap, &H, &sum, &whole, &rs, &P);
    if (rc != PACK_OK) return rc;
    const uint64_t fixed = H.fixed;
    // the same ranges through the other way of finding a byte's block: the bisection of the offsets where the frame's blocks are
    // uniform (B switched off); for a member frame there is no other way, and the plan must simply repeat
    {
        Frame G = H;
        G.B = 0;
        PackRangesPlan Q;
        ranges_plan(G, rs, count, &Q);
        bool same = Q.covered_bytes == P.covered_bytes && Q.stream_bytes == P.stream_bytes && Q.coded_bytes == P.coded_bytes && Q.out_bytes == P.out_bytes &&
                    Q.blocks == P.blocks && Q.runs.size() == P.runs.size() && Q.streams.size() == P.streams.size() && Q.out.size() == P.out.size();
        for (size_t i = 0; same && i < P.runs.size(); i++)
            same = Q.runs[i].first == P.runs[i].first && Q.runs[i].blocks == P.runs[i].blocks && Q.streams[i].src == P.streams[i].src &&
                   Q.streams[i].dst == P.streams[i].dst && Q.streams[i].bytes == P.streams[i].bytes;
        for (size_t i = 0; same && i < P.out.size(); i++) same = Q.out[i].src == P.out[i].src && Q.out[i].dst == P.out[i].dst && Q.out[i].bytes == P.out[i].bytes;
        CHECK(same, "the plan by division and the plan by bisection differ");
        if (!H.members) both_ways++;
    }
    CHECK(P.out_bytes == sum && P.out.size() == count && P.runs.size() == P.streams.size(), "the plan's own sums");
    uint64_t blocks = 0, gathered = 0;
    for (size_t i = 0; i < P.runs.size(); i++) {
        CHECK(P.runs[i].blocks >= 1 && P.runs[i].first + P.runs[i].blocks <= H.count, "run %zu inside the frame", i);
        if (i) CHECK(P.runs[i - 1].first + P.runs[i - 1].blocks < P.runs[i].first, "runs %zu and %zu sorted and maximal", i - 1, i);
        CHECK(P.streams[i].dst == gathered && P.streams[i].src >= fixed && P.streams[i].src + P.streams[i].bytes <= in_bytes, "stream piece %zu", i);
        blocks += P.runs[i].blocks;
        gathered += P.streams[i].bytes;
    }
    CHECK(blocks == P.blocks.size() && gathered == P.stream_bytes && P.covered_bytes <= H.n && P.coded_bytes <= P.covered_bytes, "covered sums");
    for (size_t i = 0; i < P.out.size(); i++)
        CHECK(P.out[i].bytes == rs[i].bytes && P.out[i].src + P.out[i].bytes <= P.covered_bytes && P.out[i].dst + P.out[i].bytes <= sum, "output piece %zu", i);
    if (words) {
        *words = {(uint64_t)P.blocks.size(), (uint64_t)P.runs.size(), P.covered_bytes, P.stream_bytes, P.coded_bytes, P.out_bytes};
        for (const PackRun &x : P.runs) { words->push_back(x.first); words->push_back(x.blocks); }
        for (const PackPiece &x : P.streams) { words->push_back(x.src); words->push_back(x.dst); words->push_back(x.bytes); }
        for (const PackPiece &x : P.out) { words->push_back(x.src); words->push_back(x.dst); words->push_back(x.bytes); }
    }
    return PACK_OK;
}

// pairs: count ranges, or with by_index count indices
static int judge_copy(const uint8_t *head, uint64_t head_bytes, uint64_t in_bytes, const uint64_t *pairs, uint64_t count, bool by_index, uint64_t out_cap,
                      std::vector<uint64_t> *words)
{
    const size_t each = by_index ? 8 : 16;
    uint8_t *h = (uint8_t *)malloc(head_bytes ? head_bytes : 1);
    uint64_t *r = (uint64_t *)malloc(count ? count * each : 1);
    memcpy(h, head, head_bytes);
    if (count) memcpy(r, pairs, count * each);
    static const uint64_t none = 0;
    const int rc = by_index ? judge(h, in_bytes, nullptr, count ? r : &none, count, out_cap, words)
                            : judge(h, in_bytes, count ? (const PackRange *)r : nullptr, nullptr, count, out_cap, words);
    free(r);
    free(h);
    return rc;
}

static bool read_file(const char *path, std::vector<uint8_t> *file)
{
    FILE *fp = fopen(path, "rb");
    if (!fp) { printf("cannot open %s\n", path); return false; }
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fp)) > 0) file->insert(file->end(), buf, buf + got);
    fclose(fp);
    return true;
}

// The cases of pack_range_check.cc ("BWTZ" frames, the same layout): every one judged and planned here too, where judge() plans it
// a second time through the offsets path and holds the two plans against each other word for word.  The merged loop can be wrong
// there without a frame test noticing: no "BWTZ" call ever bisects.
static int both_ways_cases(const std::vector<uint8_t> &file)
{
    size_t at = 0, cases = 0;
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
        const int rc = judge_copy(head, head_bytes, in_bytes, pairs.data(), count, false, out_cap, &words);
        CHECK(rc == want, "\"BWTZ\" case %zu: %d, the model says %d", cases, rc, (int)want);
        if (rc == PACK_OK && want == PACK_OK) CHECK(words == model, "\"BWTZ\" case %zu: the plan is not the model's", cases);
        at += head_bytes + 16 * (size_t)count + 8 * (size_t)nwords;
        cases++;
    }
    CHECK(cases >= 160 && both_ways >= 100, "%zu \"BWTZ\" cases, %zu planned both ways", cases, both_ways);
    return 0;
}

int main(int argc, char **argv)
{
    static_assert(sizeof(PackRange) == 16, "two words");
    if (argc != 3) { printf("usage: members_plan_check <cases> <cases of pack_range_check>\n"); return 2; }
    std::vector<uint8_t> file, bwtz;
    if (!read_file(argv[1], &file) || !read_file(argv[2], &bwtz)) return 2;
    if (both_ways_cases(bwtz) != 0) return 2;

    // the cut of a call at mixed widths (planes_plan.h)
    CHECK(planes_tiles_w(1, 1) == 1 && planes_tiles_w(PLANES_COPY_T, 1) == 1 && planes_tiles_w(PLANES_COPY_T + 1, 1) == 2, "tiles of a copied segment");
    CHECK(planes_copy_bytes(PLANES_COPY_T + 5, 0) == PLANES_COPY_T && planes_copy_bytes(PLANES_COPY_T + 5, 1) == 5 && planes_copy_bytes(5, 1) == 0, "bytes of a copied tile");
    for (uint32_t w = 2; w <= 8; w *= 2)
        for (uint64_t L : {1ull, 7ull, 8193ull, 32775ull, 65537ull}) CHECK(planes_tiles_w(L, w) == planes_tiles(L, w), "the split widths keep their tiles");
    {
        const uint64_t off[5] = {0, 1, 8194, 8194 + 32775, 8194 + 32775 + 70000};
        const uint32_t ws[4] = {8, 2, 8, 1};
        uint64_t first[5];
        CHECK(planes_cut_w(off, ws, 4, first) == 1 + 2 + 2 + 3 && first[0] == 0 && first[1] == 1 && first[2] == 3 && first[3] == 5 && first[4] == 8, "first tiles");
    }
    CHECK(members_least_bytes(3) == 32 + 96 + 3 * ec_least_bytes(1) && members_fixed_bytes(1u << 20) == 32 + (32ull << 20), "sizes");

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
        const int rc = judge_copy(head, head_bytes, in_bytes, pairs.data(), count, false, out_cap, &words);
        CHECK(rc == want, "case %zu: %d, the model says %d", cases, rc, (int)want);
        if (rc == PACK_OK && want == PACK_OK) {
            CHECK(words == model, "case %zu: the plan is not the model's", cases);
            planned++;
            if (valid.empty()) { valid.assign(head, head + head_bytes); valid_in_bytes = in_bytes; }
        }
        // the header and directory predicates alone give the same answer where they refuse
        if (head_bytes >= MEMBERS_HEADER_BYTES && members_magic(head) && want != PACK_OK && want != PACK_ARG && want != PACK_SPACE) {
            MembersHeader M;
            uint64_t frame = 0;
            int rc2 = members_header_check(head, in_bytes, &M);
            if (rc2 == PACK_OK) rc2 = members_directory_check(head + MEMBERS_HEADER_BYTES, M, in_bytes, true, &frame);
            CHECK(rc2 == want || rc2 == PACK_OK, "case %zu: the predicates alone say %d", cases, rc2);      // (PACK_OK: the ranges were refused)
        }
        at += head_bytes + 16 * (size_t)count + 8 * (size_t)nwords;
        cases++;
    }
    CHECK(cases >= 50 && planned >= 10 && !valid.empty(), "%zu cases, %zu planned", cases, planned);

    if (!valid.empty()) {
        MembersHeader M;
        CHECK(members_header_check(valid.data(), valid_in_bytes, &M) == PACK_OK && M.count >= 4 && valid.size() == members_fixed_bytes(M.count) && valid.size() >= 128,
              "the first case is a member frame of four members or more");
        const uint64_t big = ~0ull, n = M.n, one[2] = {0, 1};
        // the valid frame cut at every length below 128: refused, and nothing read past the cut
        for (uint64_t L = 0; L < 128; L++) {
            CHECK(judge_copy(valid.data(), L, L, one, 1, false, big, nullptr) == PACK_FORMAT, "cut at %llu", (unsigned long long)L);
            uint8_t *h = (uint8_t *)malloc(L ? L : 1);
            memcpy(h, valid.data(), L);
            MembersHeader C;
            CHECK(members_header_check(h, L, &C) == PACK_FORMAT, "the header check alone, cut at %llu", (unsigned long long)L);
            free(h);
        }
        // ... and told to be longer than it is by less than its streams: the directory is all that is read
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes - 16, one, 1, false, big, nullptr) == PACK_FORMAT, "in_bytes 16 short");
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes + 16, one, 1, false, big, nullptr) == PACK_FORMAT, "in_bytes 16 long");
        // not exact: a frame may end before in_bytes (bwts_unpack_size)
        uint64_t frame = 0;
        CHECK(members_directory_check(valid.data() + MEMBERS_HEADER_BYTES, M, valid_in_bytes + 160, false, &frame) == PACK_OK && frame == valid_in_bytes, "stepping");
        CHECK(members_directory_check(valid.data() + MEMBERS_HEADER_BYTES, M, valid_in_bytes - 16, false, &frame) == PACK_FORMAT, "stepping, cut");
        // hostile ranges
        const uint64_t overflow[][2] = {{big, 1}, {big, 2}, {1, big}, {big, big}, {big - 1, 2}, {n, 1}, {0, n + 1}, {n - 1, 2}, {1ull << 63, 1ull << 63}, {0, big}};
        for (const auto &o : overflow) CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, o, 1, false, big, nullptr) == PACK_RANGE, "range (%llu, %llu)", (unsigned long long)o[0], (unsigned long long)o[1]);
        const uint64_t zero[2][2] = {{big, 1}, {5, 0}};
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, zero[0], 2, false, big, nullptr) == PACK_ARG, "a range of no bytes comes before one that leaves the input");
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, nullptr, 0, false, big, nullptr) == PACK_ARG, "no ranges");
        // indices: any order, repeats; one that names no member; too many
        Frame V;
        CHECK(frame_head_check(valid.data(), valid_in_bytes, &V) == PACK_OK && frame_dir_check(valid.data() + MEMBERS_HEADER_BYTES, V, valid_in_bytes, true, &frame) == PACK_OK &&
              V.members && V.count == M.count && V.off.size() == M.count + 1 && V.off[M.count] == n, "the judged frame");
        const std::vector<uint64_t> &off = V.off;
        const uint64_t idx[4] = {M.count - 1, 0, M.count - 1, 1};
        std::vector<uint64_t> words;
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, idx, 4, true, big, &words) == PACK_OK && words[0] == (M.count > 3 ? 3u : M.count), "indices");
        CHECK(words[5] == 2 * (off[M.count] - off[M.count - 1]) + off[1] + off[2] - off[1], "the members' bytes, the repeat counted twice");
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, idx, 4, true, words[5] - 1, nullptr) == PACK_SPACE, "indices into less");
        const uint64_t bad[3] = {0, M.count, big};
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, bad, 2, true, big, nullptr) == PACK_RANGE, "index = count");
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, bad + 2, 1, true, big, nullptr) == PACK_RANGE, "index 2^64 - 1");
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, bad, 0, true, big, nullptr) == PACK_ARG, "no indices");
        std::vector<uint64_t> many(2 * (PACK_MAX_RANGES + 1), 2);
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, many.data(), PACK_MAX_RANGES + 1, true, big, nullptr) == PACK_RANGE, "2^20 + 1 indices");
        const int rc = judge_copy(valid.data(), valid.size(), valid_in_bytes, many.data(), PACK_MAX_RANGES, true, big, &words);
        CHECK(rc == ((off[3] - off[2]) * PACK_MAX_RANGES > PACK_MAX_RANGE_BYTES ? PACK_RANGE : PACK_OK), "member 2, 2^20 times: %d", rc);
        if (rc == PACK_OK) CHECK(words[0] == 1 && words[1] == 1 && words[2] == off[3] - off[2], "... is decoded once");
        // 2^20 one-byte ranges, all in member 1
        for (uint64_t i = 0; i <= PACK_MAX_RANGES; i++) { many[2 * i] = off[1] + i % 7; many[2 * i + 1] = 1; }
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, many.data(), PACK_MAX_RANGES, false, big, &words) == PACK_OK, "2^20 ranges");
        CHECK(words.size() == 6 + 5 + 3 * PACK_MAX_RANGES && words[0] == 1 && words[1] == 1 && words[5] == PACK_MAX_RANGES && words[6] == 1 && words[7] == 1, "2^20 ranges cover one member");
        CHECK(judge_copy(valid.data(), valid.size(), valid_in_bytes, many.data(), PACK_MAX_RANGES + 1, false, big, nullptr) == PACK_RANGE, "2^20 + 1 ranges");
    }

    // what a pack may be asked for
    {
        uint64_t n = 0;
        const uint64_t ls[3] = {5, 1ull << 32, 7}, ok[3] = {5, (1ull << 32) - 12, 7}, z[2] = {4, 0}, wrap[2] = {~0ull, 2};
        const uint32_t ws[3] = {1, 8, 2}, wbad[3] = {1, 3, 2};
        CHECK(members_args_check(ok, ws, 3, &n) == PACK_OK && n == 1ull << 32 && members_args_check(ok, nullptr, 3, &n) == PACK_OK, "2^32 bytes");
        CHECK(members_args_check(ls, ws, 3, &n) == PACK_RANGE && members_args_check(wrap, nullptr, 2, &n) == PACK_RANGE, "more");
        CHECK(members_args_check(ok, wbad, 3, &n) == PACK_ARG && members_args_check(z, nullptr, 2, &n) == PACK_ARG && members_args_check(ok, ws, 0, &n) == PACK_ARG &&
              members_args_check(nullptr, ws, 3, &n) == PACK_ARG, "bad arguments");
        CHECK(members_args_check(ok, ws, MEMBERS_MAX_COUNT + 1, &n) == PACK_RANGE, "too many members, decided before a length is read");
        CHECK(members_bound_bytes(ok, 2) == 32 + 64 + ec_bound_bytes(5) + ec_bound_bytes((1ull << 32) - 12) && members_bound_bytes(z, 2) == 0, "the bound");
    }

    if (failures) { printf("%d checks FAILED\n", failures); return 1; }
    printf("%zu cases, checks ok\n", cases);
    return 0;
}
