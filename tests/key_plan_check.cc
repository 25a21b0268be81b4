// key_plan_check.cc -- stand-alone host program over bijective-bwt_amd/csrc/key_plan.h, the arithmetic that picks the layout of a
// sort's round-0 keys.  tests/test_key_plan.py builds it with -fsanitize=address,undefined and runs it: histograms of every alphabet
// size in five shapes, lengths from 1 to 2^36, both sort forms and every kind of knob value go through the header, and what the
// kernels rely on is held on each answer.  Prints the longest code word met, the number of checks and "ok"; exits 1 with the failing
// line otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "key_plan.h"

static long checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        checks++;                                                                \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, where); exit(1); } \
    } while (0)
static char where[256];

enum { UNIFORM, GEOMETRIC, FIBONACCI, DOMINANT_FIRST, DOMINANT_MIDDLE, FAMILIES };
static const char *family_name[FAMILIES] = {"uniform", "geometric", "fibonacci", "dominant-first", "dominant-middle"};

// sigma present byte values spread over 0..255, counts in the family's shape, every present count >= 1, all of them summing to n
// exactly (n >= sigma).  A heap block of exactly 256 words: the sanitizer sees its end.
static uint64_t *make_hist(int family, int sigma, uint64_t n)
{
    uint64_t *hist = (uint64_t *)calloc(256, sizeof(uint64_t));
    std::vector<long double> w(sigma);
    long double a = 1, b = 1, W = 0;
    for (int i = 0; i < sigma; i++) {
        switch (family) {
        case UNIFORM: w[i] = 1; break;
        case GEOMETRIC: w[i] = a; a *= 0.5L; break;
        case FIBONACCI: { w[i] = a; const long double c = a + b; a = b; b = c; break; }
        case DOMINANT_FIRST: w[i] = i == 0 ? 1 : 0; break;
        default: w[i] = i == sigma / 2 ? 1 : 0; break;
        }
        W += w[i];
    }
    uint64_t sum = 0;
    int top = 0;
    const uint64_t spare = n - (uint64_t)sigma;          // what is left once every symbol has its one
    for (int i = 0; i < sigma; i++) {
        const int c = (int)((long)i * 256 / sigma);
        long double share = (long double)spare * (w[i] / W);
        uint64_t v = 1 + (share >= (long double)spare ? spare : (uint64_t)share);
        hist[c] = v; sum += v;
        if (w[i] > w[top]) top = i;
    }
    const int ctop = (int)((long)top * 256 / sigma);
    while (sum > n) {                                     // (rounding: the shares may overshoot by a few)
        for (int i = 0; i < sigma && sum > n; i++) { const int c = (int)((long)i * 256 / sigma); if (hist[c] > 1) { hist[c]--; sum--; } }
    }
    hist[ctop] += n - sum;
    return hist;
}

static int longest_seen = 0, longest_sigma = 0, longest_family = 0;
static uint64_t longest_n = 0;

// what every answer must satisfy, whatever was asked
static void check_plan(const KeyPlan &P, const uint64_t *hist, uint64_t n, bool reserve_pad)
{
    const Alphabet &al = P.al;
    int sigma = 0;
    uint64_t sum = 0;
    for (int c = 0; c < 256; c++) { sigma += hist[c] != 0; sum += hist[c]; }
    CHECK(sum == n);
    CHECK(al.sigma == sigma);
    CHECK(al.bits >= 1 && al.bits <= 9 && (al.bits == 9) == (sigma == 256 && reserve_pad) && al.pad_add == (al.bits == 9 ? 1 : 0));
    CHECK(al.msym >= 1 && al.msym * al.bits <= 64);
    CHECK(al.hstep >= 1);
    CHECK(al.key_bits >= 1 && al.key_bits <= 64);
    CHECK(P.stack_high <= KEY_WALK_STACK);
    CHECK(P.passes_fixed >= 1 && P.passes_fixed <= 8 && P.passes_var <= 8);
    if (!al.varlen) {
        CHECK(al.key_bits == al.msym * al.bits && al.hstep == al.msym && al.patch_span == al.msym - 1);
    } else {
        CHECK(!reserve_pad && sigma > 1 && P.code_built);
        CHECK(al.key_bits >= P.lmax && al.key_bits >= 8 && al.patch_span == 64);
        CHECK(al.hstep == (al.key_bits / P.lmax < 1 ? 1 : al.key_bits / P.lmax) && al.msym == al.hstep);
    }
    if (reserve_pad || sigma == 1) CHECK(!P.code_built && P.lmax == 0 && !al.varlen);
    if (!P.code_built) {
        for (int c = 0; c < 256; c++) CHECK(P.vtab[c] == 0);
        CHECK(P.kb_iid == 0 && P.kb == 0 && P.passes_var == 0);
        return;
    }
    // the code table: every present byte has a word of 1 .. VL_MAXLEN <= 31 bits, absent bytes none; Kraft sum exactly 1; the words
    // of neighbouring present bytes increase when left-aligned, and neither is a prefix of the other
    CHECK(P.lmax >= 1 && P.lmax <= VL_MAXLEN && VL_MAXLEN <= 31);
    uint64_t kraft = 0, prev = 0;
    int longest = 0, prev_len = 0;
    for (int c = 0; c < 256; c++) {
        const int l = (int)(P.vtab[c] >> 32);
        const uint64_t code = (uint32_t)P.vtab[c];
        if (!hist[c]) { CHECK(P.vtab[c] == 0); continue; }
        CHECK(l >= 1 && l <= 31 && code < (1ull << l));
        kraft += 1ull << (31 - l);
        if (l > longest) longest = l;
        const uint64_t left = code << (32 - l);
        if (prev_len) {
            CHECK(left > prev);
            const int s = l < prev_len ? l : prev_len;
            CHECK((left >> (32 - s)) != (prev >> (32 - s)));
        }
        prev = left; prev_len = l;
    }
    CHECK(kraft == 1ull << 31);
    CHECK(longest == P.lmax);
    CHECK(P.kb_iid >= 32 && P.kb_iid <= 64 && P.kb_iid % 8 == 0);
    CHECK(P.kb >= 8 && P.kb >= P.lmax && P.kb <= 64 && P.passes_var == (P.kb + 7) / 8);
    for (int b = 1; b <= 64; b++) CHECK(P.share[b] >= 0.0 && P.share[b] <= P.share[b - 1] * (1.0 + 1e-12));
}

int main()
{
    const uint64_t lengths[] = {0 /* = sigma: every symbol once */, 1ull << 10, (1ull << 17) + 5, 1ull << 22, 1ull << 30, 1ull << 36};
    KeyPlan P;
    // every alphabet size, every shape, every length, both forms: no knob, no sample
    for (int sigma = 1; sigma <= 256; sigma++)
        for (int family = 0; family < FAMILIES; family++)
            for (uint64_t len : lengths) {
                const uint64_t n = len ? len : (uint64_t)sigma;
                if (n < (uint64_t)sigma) continue;
                uint64_t *hist = make_hist(family, sigma, n);
                for (int pad = 0; pad < 2; pad++) {
                    snprintf(where, sizeof where, "%s sigma %d n %llu pad %d", family_name[family], sigma, (unsigned long long)n, pad);
                    key_plan(hist, n, pad != 0, KeyKnobs(), KeySample(), &P);
                    check_plan(P, hist, n, pad != 0);
                    CHECK(P.lmax != KEY_CODE_REFUSED);
                    if (P.lmax > longest_seen) { longest_seen = P.lmax; longest_sigma = sigma; longest_family = family; longest_n = n; }
                }
                free(hist);
            }
    // every kind of knob value, legal and not, and a sample that asks for every width, on a few alphabets
    const int sigmas[] = {1, 2, 5, 16, 40, 256};
    const int ksym[] = {KEY_KNOB_ABSENT, -1, 0, 1, 7, 8, 21, 64, 65, 1000000};
    const int kvl[] = {KEY_KNOB_ABSENT, 0, 1, 2};
    const int kbits[] = {KEY_KNOB_ABSENT, -8, 0, 7, 8, 9, 15, 16, 17, 32, 33, 40, 41, 64, 65, 1 << 30};
    const int kemp[] = {0, 32, 40, 48, 56, 64};
    unsigned turn = 0;
    for (int sigma : sigmas)
        for (int family : {UNIFORM, GEOMETRIC, DOMINANT_MIDDLE})
            {
                const uint64_t n = (sigma + family) % 2 ? (1ull << 17) + 5 : 1ull << 22;
                uint64_t *hist = make_hist(family, sigma, n);
                for (int pad = 0; pad < 2; pad++)
                    for (int s : ksym)
                        for (int v : kvl)
                            for (int kb : kbits) {
                                const int emp = kemp[turn++ % 6u];
                                snprintf(where, sizeof where, "%s sigma %d n %llu pad %d knobs %d %d %d sample %d", family_name[family], sigma,
                                         (unsigned long long)n, pad, s, v, kb, emp);
                                KeyKnobs kn;
                                kn.key_symbols = s; kn.varlen = v; kn.key_bits = kb;
                                KeySample sm;
                                sm.kb_emp = emp;
                                if (emp) for (int b = 32; b <= 56; b += 8) sm.partners_of[b] = b < emp ? 1.0 : 1e-6;
                                key_plan(hist, n, pad != 0, kn, sm, &P);
                                check_plan(P, hist, n, pad != 0);
                                const int maxsym = 64 / P.al.bits;
                                if (!P.al.varlen && s >= 1 && s <= maxsym && !(P.code_built && emp > P.kb_iid && 40 / P.lmax < 4)) CHECK(P.al.msym == s);
                                if (v == 0 || (s != KEY_KNOB_ABSENT && v == KEY_KNOB_ABSENT)) CHECK(!P.al.varlen && !P.code_built);
                                if (v == 1 && !pad && sigma > 1) CHECK(P.al.varlen);
                                if (P.code_built && kb >= 8 && kb >= P.lmax && kb <= 64) CHECK(P.kb == kb);
                                if (P.code_built && !(kb >= 8 && kb >= P.lmax && kb <= 64)) CHECK(P.kb == P.kb_iid || (emp > P.kb_iid && (P.kb == 40 || P.kb == emp)));
                            }
                free(hist);
            }
    // the tree walk's own guard: without the smoothing Fibonacci weights make a tree as deep as the alphabet is large; the builder
    // refuses it beyond 31 levels and never hands out a longer word
    for (int sigma = 2; sigma <= 256; sigma += (sigma < 40 ? 1 : 27)) {
        uint64_t *hist = make_hist(FIBONACCI, sigma, 1ull << 36);
        uint32_t code[256]; uint8_t len[256];
        double avg = 0, ent = 0;
        int high = 0;
        snprintf(where, sizeof where, "unsmoothed fibonacci sigma %d", sigma);
        const int lmax = build_alphabetic_code(hist, 1ull << 36, code, len, &avg, &ent, 0.0, &high);
        CHECK(high <= KEY_WALK_STACK);
        CHECK(lmax == KEY_CODE_REFUSED || (lmax >= 1 && lmax <= 31));
        for (int c = 0; c < 256; c++) CHECK(len[c] <= 31);
        free(hist);
    }
    printf("longest code %d bits (%s, %d symbols, n = %llu)\n%ld checks ok\n", longest_seen, family_name[longest_family], longest_sigma,
           (unsigned long long)longest_n, checks);
    return 0;
}
