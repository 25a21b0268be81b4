// estimate_plan_check.cc -- stand-alone host program over bijective-bwt_amd/csrc/estimate_plan.h, the arithmetic that the estimator's
// kernel shares with the host, and over the AUTO predicates and the bound of members_plan.h.  tests/test_pack_members_auto_model.py
// builds it with -fsanitize=address,undefined and runs it with one argument: a file of lg(1) .. lg(2^18) as little-endian u32, which
// the test has computed in Python integers.  Every buffer below is a heap block of exactly the size the checked function may touch.
// Prints "est <w> <len> <est_none> <est_delta>" for members it makes itself (the test holds the model against these lines), then the
// number of checks and "ok"; exits 1 with the failing line otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "estimate_plan.h"
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

// lg against the table, at the powers of two, and its growth
static void lg_checks(const char *path)
{
    const uint32_t top = 1u << 18;
    std::vector<uint32_t> want(top);
    FILE *f = fopen(path, "rb");
    CHECK(f != nullptr);
    CHECK(fread(want.data(), 4, top, f) == top);
    fclose(f);
    for (uint32_t x = 1; x <= top; x++) CHECK(estimate_lg(x) == want[x - 1]);
    for (uint32_t k = 0; k < 32; k++) CHECK(estimate_lg(1u << k) == k << ESTIMATE_FRAC);
    for (uint32_t x = 2; x <= top; x++) CHECK(estimate_lg(x) >= estimate_lg(x - 1));
    for (uint32_t k = 1; k < 32; k++) {
        const uint32_t x = 1u << k;
        CHECK(estimate_lg(x - 1) <= estimate_lg(x) && estimate_lg(x) <= estimate_lg(x + 1) && estimate_lg(x - 1) >= (k - 1) << ESTIMATE_FRAC);
    }
    CHECK(estimate_lg(0xFFFFFFFFu) < 32u << ESTIMATE_FRAC && estimate_lg(0xFFFFFFFFu) >= (32u << ESTIMATE_FRAC) - 2u);
    CHECK(estimate_lg(3) == 103872);      // floor(2^16 log2(3)) = 103872
    CHECK(estimate_term(0) == 0 && estimate_term(1) == 0 && estimate_term(2) == 2u << ESTIMATE_FRAC);
}

// costs: never negative (the subtraction saturates), 0 for one symbol, N bytes for 256 symbols alike, and the sum of the terms grows
// when two symbols are merged
static void cost_checks()
{
    uint32_t c[256];
    memset(c, 0, sizeof c);
    CHECK(estimate_hist_bytes(c) == 0);
    for (uint32_t N : {1u, 2u, 3u, 4095u, 4096u, 262143u, 262144u}) {
        memset(c, 0, sizeof c);
        c[77] = N;
        CHECK(estimate_hist_bytes(c) == 0);
        c[77] = N - N / 2; c[3] = N / 2;
        // two symbols: one bit an entry at most, and exactly that where they are alike
        CHECK(estimate_hist_bytes(c) <= (N + 7) / 8 + 1);
        if (N % 2 == 0 && (N & (N - 1)) == 0) CHECK(estimate_hist_bytes(c) == (N + 7) / 8);
    }
    for (int s = 0; s < 256; s++) c[s] = 1024;
    CHECK(estimate_hist_bytes(c) == 262144);
    CHECK(estimate_bytes(262144, estimate_term(262144)) == 0 && estimate_bytes(5, ~0ull) == 0 && estimate_bytes(1, 0) == 0);
    CHECK(estimate_bytes(2, 0) == 1 && estimate_bytes(262144, 0) == 262144ull * 18 / 8);
    uint64_t x = 88172645463325252ull;
    for (int round = 0; round < 2000; round++) {
        uint32_t N = 0;
        uint64_t terms = 0;
        for (int s = 0; s < 256; s++) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            c[s] = (round & 1) ? (uint32_t)(x % 1025) : ((x >> 20) % 7 == 0 ? (uint32_t)(x % 1025) : 0u);
            N += c[s];
            terms += estimate_term(c[s]);
        }
        const uint64_t bytes = estimate_hist_bytes(c);
        CHECK(bytes <= N);                      // (at most eight bits an entry)
        // merging two symbols never makes a histogram dearer: (a + b) lg(a + b) >= a lg(a) + b lg(b) up to lg's rounding, below two units an entry
        const uint32_t a = c[round % 256], b = c[(round * 7 + 1) % 256];
        if (a && b && (round % 256) != (round * 7 + 1) % 256) CHECK(estimate_term(a + b) + 2 * (a + b) >= estimate_term(a) + estimate_term(b));
        CHECK(estimate_bytes(N, terms) == bytes);
    }
}

// the units of a member, and the cut of a call
static void unit_checks()
{
    for (uint32_t w : WIDTHS) {
        for (uint64_t len = 0; len < w; len++) CHECK(estimate_units(len, w) == 0 && estimate_unit_elems(len, w, 0) == 0);
        CHECK(estimate_units(w, w) == 1 && estimate_unit_elems(w, w, 0) == 1 && estimate_units(2 * w - 1, w) == 1);
        const uint64_t U = (uint64_t)ESTIMATE_UNIT * w;
        CHECK(estimate_units(U - 1, w) == 1 && estimate_unit_elems(U - 1, w, 0) == ESTIMATE_UNIT - 1);
        CHECK(estimate_units(U, w) == 1 && estimate_unit_elems(U, w, 0) == ESTIMATE_UNIT && estimate_unit_elems(U, w, 1) == 0);
        CHECK(estimate_units(U + w - 1, w) == 1);
        CHECK(estimate_units(U + w, w) == 2 && estimate_unit_elems(U + w, w, 1) == 1 && estimate_unit_elems(U + w, w, 0) == ESTIMATE_UNIT);
        CHECK(estimate_units(1ull << 32, w) == (1ull << 32) / U);
        CHECK(estimate_units((1ull << 32) - 1, w) == (1ull << 32) / U && estimate_unit_elems((1ull << 32) - 1, w, (1ull << 32) / U - 1) == ESTIMATE_UNIT - 1);
    }
    CHECK(ESTIMATE_UNIT_TILES == 64);
    const uint64_t off[6] = {0, 3, 3 + 2 * (uint64_t)ESTIMATE_UNIT * 4 + 5, 3 + 2 * (uint64_t)ESTIMATE_UNIT * 4 + 12, 3 + 2 * (uint64_t)ESTIMATE_UNIT * 4 + 13, 3 + 2 * (uint64_t)ESTIMATE_UNIT * 4 + 21};
    const uint32_t widths[5] = {4, 4, 8, 1, 8};
    uint64_t first[6];
    CHECK(estimate_cut(off, widths, nullptr, 5, first) == 5);       // 0 (three bytes at width 4), 3, 0 (seven at width 8), 1, 1
    CHECK(first[0] == 0 && first[1] == 0 && first[2] == 3 && first[3] == 3 && first[4] == 4 && first[5] == 5);
    const uint8_t take[5] = {1, 0, 1, 1, 0};
    CHECK(estimate_cut(off, widths, take, 5, first) == 1 && first[3] == 0 && first[4] == 1 && first[5] == 1);
}

// the rule that makes a filter of two estimates
static void filter_checks()
{
    CHECK(estimate_filter(0, 0) == DELTA_FILTER_NONE && estimate_filter(65514, 65511) == DELTA_FILTER_NONE);
    CHECK(estimate_filter(6400, 6300) == DELTA_FILTER_NONE && estimate_filter(6400, 6299) == DELTA_FILTER_DELTA);
    CHECK(estimate_filter(63, 62) == DELTA_FILTER_DELTA && estimate_filter(64, 63) == DELTA_FILTER_NONE && estimate_filter(5, 9) == DELTA_FILTER_NONE);
}

// the serial statement on members made here; the test holds tests/estimate_model.py against the lines
static void serial_checks()
{
    uint64_t x = 0x2545F4914F6CDD1Dull;
    const uint64_t lens[6] = {1, 7, 4096, 70001, (uint64_t)ESTIMATE_UNIT + 9, 2 * (uint64_t)ESTIMATE_UNIT + 3};
    for (uint32_t w : WIDTHS) {
        for (uint64_t len : lens) {
            Exact m(len);
            // a walk in the low byte of every element under noise that thins out: compressible planes, and differences that wrap
            for (uint64_t i = 0; i < len; i++) {
                x = x * 6364136223846793005ull + 1442695040888963407ull;
                m.p[i] = (i % w) == 0 ? (uint8_t)(i / w + ((x >> 60) & 3u)) : (uint8_t)((x >> 56) & ((i / w) % 3 == 0 ? 0xFFu : 0x03u));
            }
            uint64_t est[2] = {~0ull, ~0ull};
            estimate_serial(m.p, len, w, est);
            CHECK(est[0] <= len && est[1] <= len);
            if (len < w) CHECK(est[0] == 0 && est[1] == 0);
            printf("est %u %llu %llu %llu\n", w, (unsigned long long)len, (unsigned long long)est[0], (unsigned long long)est[1]);
        }
        // one value repeated: nothing to code under either filter but the first difference, one entry among q <= 40000 of every plane:
        // lg(q) + 1.45 bits at most, three bytes
        Exact m(8 * 5000);
        memset(m.p, 0xA5, 8 * 5000);
        uint64_t est[2];
        estimate_serial(m.p, 8 * 5000, w, est);
        CHECK(est[0] == 0 && est[1] >= 1 && est[1] <= 3 * w);
    }
}

// the arguments and the bound of a pack that chooses
static void auto_checks()
{
    const uint64_t lengths[5] = {65536, 3, 16384 * 2, 16384 * 2 - 2, 100000 * 8 + 5};
    const uint32_t widths[5] = {4, 4, 2, 2, 8};
    uint32_t methods[5], chain[5] = {0, 0, 0, 0, 0}, direct[5] = {1, 1, 1, 1, 1};
    uint64_t n = 0;
    for (uint32_t bits = 0; bits < 243; bits++) {        // every mix of 0, 1 and AUTO over the five members
        uint32_t lo[5], hi[5], b = bits;
        bool any = false;
        for (int k = 0; k < 5; k++, b /= 3) {
            methods[k] = b % 3 == 2 ? MEMBERS_AUTO : b % 3;
            any = any || methods[k] == MEMBERS_AUTO;
            lo[k] = methods[k] == MEMBERS_AUTO ? 0u : methods[k];
            hi[k] = methods[k] == MEMBERS_AUTO ? 1u : methods[k];
        }
        const uint64_t a = members_bound_bytes_a(lengths, widths, methods, 5);
        CHECK(a >= members_bound_bytes_m(lengths, widths, lo, 5) && a >= members_bound_bytes_m(lengths, widths, hi, 5));
        if (!any) CHECK(a == members_bound_bytes_m(lengths, widths, methods, 5));
        CHECK(members_args_check_a(lengths, widths, methods, methods, 5, &n) == PACK_OK && n == 65536 + 3 + 32768 + 32766 + 800005);
        CHECK((members_args_check_m(lengths, widths, nullptr, methods, 5, &n) == PACK_OK) == !any);
    }
    for (int k = 0; k < 5; k++) methods[k] = MEMBERS_AUTO;
    CHECK(members_bound_bytes_a(lengths, widths, methods, 5) >= members_bound_bytes_m(lengths, widths, chain, 5));
    CHECK(members_bound_bytes_a(lengths, widths, methods, 5) >= members_bound_bytes_m(lengths, widths, direct, 5));
    CHECK(members_bound_bytes_a(lengths, nullptr, nullptr, 5) == members_bound_bytes(lengths, 5));
    CHECK(members_any_auto(methods, 5) && !members_any_auto(chain, 5) && !members_any_auto(nullptr, 5));
    methods[2] = 2;
    CHECK(members_bound_bytes_a(lengths, widths, methods, 5) == 0 && members_args_check_a(lengths, widths, nullptr, methods, 5, &n) == PACK_ARG);
    CHECK(members_args_check_a(lengths, widths, methods, nullptr, 5, &n) == PACK_ARG && members_args_check_a(lengths, widths, nullptr, nullptr, 0, &n) == PACK_ARG);
    methods[2] = 254;
    CHECK(members_args_check_a(lengths, widths, nullptr, methods, 5, &n) == PACK_ARG);
    const uint64_t zero[2] = {5, 0};
    CHECK(members_bound_bytes_a(zero, nullptr, nullptr, 2) == 0);
    // the cost of a method and the choice: the table's words count, and a tie goes to the chain
    CHECK(members_method_cost(1000, 65536, 4, MEMBERS_METHOD_CHAIN) == 1000 && members_method_cost(1000, 65536, 4, MEMBERS_METHOD_ORDER0) == 1032);
    CHECK(members_method_cost(1000, 3, 4, MEMBERS_METHOD_ORDER0) == 1000 && members_method_cost(1000, 65536, 1, MEMBERS_METHOD_ORDER0) == 1000);
    CHECK(members_method_choice(1000, 1000) == MEMBERS_METHOD_CHAIN && members_method_choice(1000, 999) == MEMBERS_METHOD_ORDER0);
    CHECK(members_method_choice(999, 1000) == MEMBERS_METHOD_CHAIN);
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: estimate_plan_check <table of lg(1) .. lg(2^18), u32 little-endian>\n"); return 2; }
    lg_checks(argv[1]);
    cost_checks();
    unit_checks();
    filter_checks();
    serial_checks();
    auto_checks();
    printf("%ld checks ok\n", checks);
    return 0;
}
