// key_plan.h -- the layout of a sort's round-0 keys as host arithmetic: the single statement of the rules that turn a byte histogram
// into an alphabet, a code table and a key width.  Fixed-width codes and the symbols per key (pick_key_symbols), the optimal alphabetic
// code (build_alphabetic_code), the width a variable-length key needs (iid_key_bits), the knobs BWTS_KEY_SYMBOLS, BWTS_VARLEN and
// BWTS_KEY_BITS, and the choice between the two layouts by their radix passes.  Plain C++ with no dependency, no context and no device:
// set_alphabet (forward.hip) calls it and only adds the sampled measurement and the copies to the device; bwts_debug_key_plan
// (api_test.hip) and a stand-alone host program (tests/key_plan_check.cc, built with the sanitizers) compile the same file.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

// Longest code word the variable-length key builder accepts (its bit stream in LDS holds KB_SYMS words of this length).  The refusal
// `lmax <= VL_MAXLEN` in key_plan_begin is a guard that no histogram reaches: the smoothing gives every present symbol a weight of at
// least n / 2^14 + 1 out of a total below n + 256 (n / 2^14 + 1), and a leaf of an optimal alphabetic tree cannot lie deep under so
// little weight.  The longest word that tests/test_key_plan.py::test_longest_code finds over the histogram families (uniform,
// geometric series of ratios 0.45 .. 0.79, Fibonacci weights, one dominant symbol first or in the middle, geometric series with a rare
// symbol between every two members; 2 .. 256 symbols; n = 2^10 .. 2^36) is 17 bits, for n = 2^17 and 32 byte values 0, 8, 16, ... of
// which the even-numbered ones follow a geometric series of ratio 0.6 (52 436, 31 459, 18 876, ...) and the ones between them occur once;
// the plain geometric series over 16 symbols gives 15.  tests/key_plan_check.cc holds every histogram it walks against the 24.
#define VL_MAXLEN 24
#define KEY_CODE_REFUSED 99             // build_alphabetic_code: the tree went deeper than 31 levels, no table was made
#define KEY_WALK_STACK 512              // entries of the tree walk's stack
#define KEY_KNOB_ABSENT INT_MIN         // a knob that is not set

struct Alphabet {
    int sigma;      // distinct byte values present
    int bits;       // bits per symbol code
    int msym;       // symbols packed into a round-0 key
    int key_bits;   // bits * msym (fixed-width codes) or the chosen key width (variable-length codes)
    int pad_add;    // added to a table code by the kernels (9-bit padded alphabet only)
    bool varlen;    // order-preserving variable-length codes (optimal alphabetic tree) instead of fixed-width ones
    int hstep;      // symbols every key is guaranteed to cover: the step of round 1 (msym, or key_bits / longest code)
    int patch_span; // positions in front of a factor's end whose key wraps around (msym - 1, or 64)
    bool few_ties;  // the model of this key, and the key sample where one was taken, expect at most n / 64 positions tied after round 0
};

// The three knobs as numbers.  key_symbols and key_bits: atoi of the knob's text.  varlen: 0 for a text that starts with '0' (never),
// 1 for one that starts with '1' (always), 2 for any other text (set, and says neither).
struct KeyKnobs {
    int key_symbols = KEY_KNOB_ABSENT, varlen = KEY_KNOB_ABSENT, key_bits = KEY_KNOB_ABSENT;
};
static inline int key_knob_int(const char *text) { return text ? atoi(text) : KEY_KNOB_ABSENT; }
static inline int key_knob_varlen(const char *text) { return !text ? KEY_KNOB_ABSENT : text[0] == '0' ? 0 : text[0] == '1' ? 1 : 2; }

static inline int bitlen_u64(uint64_t x) { int b = 0; while (x) { b++; x >>= 1; } return b; }

// Symbols per round-0 key.  A key only has to separate most positions: for an i.i.d. source with collision entropy
// H2 bits per symbol, about n * 2^(log2 n - m * H2) positions stay tied after m symbols.  Taking the smallest m that
// keeps that below ~0.4 % of n saves whole radix passes on high-entropy inputs (uniform bytes: 40 instead of 64 key
// bits at 2^28); a wrong guess (real text is not i.i.d.) only moves work into the later rounds, never changes the result.
static inline int pick_key_symbols(const uint64_t *hist, uint64_t n, int bits, int max_sym)
{
    double sum2 = 0.0;
    for (int c = 0; c < 256; c++) { const double p = (double)hist[c] / (double)n; sum2 += p * p; }
    if (sum2 >= 1.0) return max_sym;                            // one symbol: nothing separates
    const double H2 = -log2(sum2);
    const double need = log2((double)n) + 8.0;                  // bits of collision entropy wanted in a key
    // a hair of slack: exactly-uniform alphabets land on the boundary ((log2 n + 8) / log2 sigma a whole number, as for 2^k symbols
    // at n = 2^(j k - 8): m = j, not j + 1)
    const double want = ceil(need / H2 - 0.05);
    if (!(want <= (double)max_sym)) return max_sym;             // (also where the quotient is beyond an int: a histogram all but constant)
    int m = (int)want;
    // whole passes are what counts: use every symbol that fits in the same number of 8-bit passes
    if (m < 1) m = 1;
    const int passes = (m * bits + 7) / 8;
    while (m < max_sym && ((m + 1) * bits + 7) / 8 <= passes) m++;
    return m;
}

// Optimal alphabetic (order-preserving prefix) code for the byte histogram: the classic interval DP with Knuth's
// monotone-root bound, O(sigma^2).  Order-preserving means that comparing concatenated code words bit by bit is
// comparing the symbol strings, so packed code bits sort like the text does -- but frequent symbols take fewer bits,
// so a key of B bits separates positions about as well as B bits of entropy would.  Returns the longest code length, or
// KEY_CODE_REFUSED.  stack_high (may be null): the most entries the walk's stack held.
static inline int build_alphabetic_code(const uint64_t *hist, uint64_t n, uint32_t *code, uint8_t *len, double *avg_len, double *entropy,
                                        double smooth_scale = 1.0, int *stack_high = nullptr)
{
    // (heap, not static: contexts on different host threads may be here at the same time)
    std::vector<double> Cv(256 * 256);
    std::vector<uint16_t> Rv(256 * 256);
    double (*C)[256] = (double (*)[256])Cv.data();
    uint16_t (*R)[256] = (uint16_t (*)[256])Rv.data();
    int sym[256], sigma = 0;
    double w[256], pre[257];
    for (int c = 0; c < 256; c++) { code[c] = 0; len[c] = 0; if (hist[c]) sym[sigma++] = c; }
    if (stack_high) *stack_high = 0;
    // keeps rare symbols' codes short enough for the key builder; a larger scale flattens the tree (shorter longest code)
    const double smooth = ((double)(n >> 14) + 1.0) * smooth_scale;
    pre[0] = 0;
    for (int i = 0; i < sigma; i++) { w[i] = (double)hist[sym[i]] + smooth; pre[i + 1] = pre[i] + w[i]; }
    if (sigma == 1) { len[sym[0]] = 1; *avg_len = 1; *entropy = 0; return 1; }
    for (int i = 0; i < sigma; i++) { C[i][i] = 0; R[i][i] = (uint16_t)i; }
    for (int L = 2; L <= sigma; L++) {
        for (int i = 0; i + L - 1 < sigma; i++) {
            const int j = i + L - 1;
            int lo = R[i][j - 1], hi = R[i + 1][j];
            if (lo < i) lo = i;
            if (hi > j - 1) hi = j - 1;
            if (hi < lo) hi = lo;
            double best = 1e300; int arg = lo;
            for (int k = lo; k <= hi; k++) {
                const double v = C[i][k] + C[k + 1][j];
                if (v < best) { best = v; arg = k; }
            }
            C[i][j] = best + (pre[j + 1] - pre[i]);
            R[i][j] = (uint16_t)arg;
        }
    }
    // walk the tree: left = 0, right = 1
    struct Item { int i, j, depth; uint32_t prefix; } stack[KEY_WALK_STACK];
    int sp = 0, lmax = 0;
    stack[sp++] = Item{0, sigma - 1, 0, 0u};
    while (sp) {
        const Item it = stack[--sp];
        if (it.i == it.j) {
            len[sym[it.i]] = (uint8_t)it.depth; code[sym[it.i]] = it.prefix;
            if (it.depth > lmax) lmax = it.depth;
            continue;
        }
        if (it.depth >= 31) return KEY_CODE_REFUSED;
        const int k = R[it.i][it.j];
        stack[sp++] = Item{k + 1, it.j, it.depth + 1, (it.prefix << 1) | 1u};
        stack[sp++] = Item{it.i, k, it.depth + 1, it.prefix << 1};
        if (stack_high && sp > *stack_high) *stack_high = sp;
    }
    double al = 0, h = 0;
    for (int i = 0; i < sigma; i++) {
        const double p = (double)hist[sym[i]] / (double)n;
        al += p * len[sym[i]];
        h -= p * log2(p);
    }
    *avg_len = al; *entropy = h;
    return lmax;
}

// Fixed-width codes: the byte -> code table, sigma, bits per code.  The cyclic sort uses codes 0..sigma-1; the suffix (non-cyclic)
// sort reserves code 0 for "past the end" and uses 1..sigma (reserve_pad).
static inline void fixed_codes(const uint64_t *hist, bool reserve_pad, uint8_t codes[256], Alphabet *al)
{
    int sigma = 0;
    for (int c = 0; c < 256; c++) codes[c] = hist[c] ? (uint8_t)(sigma++ + (reserve_pad ? 1 : 0)) : (uint8_t)0;   // sigma == 256 with pad handled below
    const int ncodes = sigma + (reserve_pad ? 1 : 0);
    al->sigma = sigma;
    al->bits = bitlen_u64((uint64_t)(ncodes > 1 ? ncodes - 1 : 1));
    al->pad_add = 0;
    if (al->bits > 8) {
        // 256 symbols + pad: 9-bit codes; the u8 table cannot hold code 256, so the kernels add
        // the +1 themselves (the table then holds 0..255)
        for (int c = 0, s = 0; c < 256; c++) if (hist[c]) codes[c] = (uint8_t)(s++);
        al->pad_add = 1;
    }
}

// Width of a variable-length key: the smallest whole number of bytes B for which an i.i.d. source with this histogram leaves at most
// ~0.8 % of the positions tied.  share[b] = probability that two independent positions agree on the first b
// bits of their code streams: both start with the same symbol and agree on the rest, or their first code
// words are both longer than b bits and agree on those b bits.  share[0..64] is left for the caller.
static inline int iid_key_bits(const uint64_t *hist, const uint8_t *vlen, const uint32_t *vcode, uint64_t n, double share[65])
{
    double p[256];
    for (int c = 0; c < 256; c++) p[c] = (double)hist[c] / (double)n;
    share[0] = 1.0;
    for (int b = 1; b <= 64; b++) {
        double s = 0.0;
        for (int c = 0; c < 256; c++)
            if (vlen[c] && vlen[c] <= b) s += p[c] * p[c] * share[b - vlen[c]];
        // code words longer than b bits that share their first b bits are neighbours in symbol order
        // (alphabetic and prefix-free), so the partial term is a sum of squared run masses
        double mass = 0.0; uint32_t cur = 0; bool open = false;
        for (int c = 0; c < 256; c++) {
            if (!vlen[c] || vlen[c] <= b) continue;
            const uint32_t pc = vcode[c] >> (vlen[c] - b);
            if (open && pc == cur) mass += p[c];
            else { s += mass * mass; mass = p[c]; cur = pc; open = true; }
        }
        s += mass * mass;
        share[b] = s;
    }
    for (int b = 32; b <= 64; b += 8)
        if ((double)n * share[b] <= 1.0 / 128.0) return b;
    return 64;
}

// What a key sample says (set_alphabet's sampled measurement): kb_emp, the narrowest width of 32, 40, 48, 56 or 64 bits at which the
// sample expects few ties, and partners_of[b] (b = 32, 40, 48, 56; < 0 elsewhere): the equal keys of b bits a position is expected to
// meet, by the sample where it saw enough, else by the model.  Absent: kb_emp = 0.
struct KeySample {
    int kb_emp = 0;
    double partners_of[65];
    KeySample() { for (int b = 0; b <= 64; b++) partners_of[b] = -1.0; }          // (no sample, or none at this width: the model)
};
// a position that expects `partners` others with its key is tied with probability 1 - exp(-partners): few ties = at most 1 / 64
static inline bool key_few_ties(double partners) { return 1.0 - exp(-partners) <= 1.0 / 64.0; }

struct KeyPlan {
    // what was asked
    const uint64_t *hist; uint64_t n; bool reserve_pad; KeyKnobs knobs;
    // the answer
    Alphabet al;
    uint8_t codes[256];         // byte -> fixed-width code (all layouts carry it: the suffix sort and the Lyndon search read it)
    uint64_t vtab[256];         // (length << 32) | code of each byte value; all 0 where no alphabetic code was built
    // how it was reached
    bool code_built;            // an alphabetic code was built and accepted (lmax <= VL_MAXLEN): the variable-length key is a candidate
    int lmax;                   // its longest word, 0 when none was built (KEY_CODE_REFUSED: built and refused)
    int stack_high;             // most entries the tree walk's stack held
    double avg, entropy;        // mean code length and entropy of the histogram, bits per symbol
    double share[65];           // iid_key_bits' model
    int kb_iid;                 // iid_key_bits' own width, 0 when no code was built
    int kb;                     // the variable-length key's width after sample and knob, 0 when no code was built
    int passes_fixed, passes_var;   // radix passes of both alternatives (passes_var = 0: there is no alternative)
};

// tied after round 0, as pick_key_symbols models it: a position meets n * (sum of p^2)^msym others with its key
static inline double key_fixed_partners(const uint64_t *hist, uint64_t n, int m)
{
    double sum2 = 0.0;
    for (int c = 0; c < 256; c++) { const double p = (double)hist[c] / (double)n; sum2 += p * p; }
    return (double)n * pow(sum2, (double)m);
}

// First half: the fixed-width layout, and the alphabetic code with the model's key width where one is to be tried.  hist must stay
// valid until key_plan_finish.  What a sample needs (vtab, share) is ready afterwards when P->code_built.
static inline void key_plan_begin(const uint64_t *hist, uint64_t n, bool reserve_pad, const KeyKnobs &knobs, KeyPlan *P)
{
    P->hist = hist; P->n = n; P->reserve_pad = reserve_pad; P->knobs = knobs;
    Alphabet *al = &P->al;
    fixed_codes(hist, reserve_pad, P->codes, al);
    const int bits = al->bits;
    int msym = pick_key_symbols(hist, n, bits, 64 / bits);
    // BWTS_KEY_SYMBOLS, tuning / test knob: force the symbol count (0 = maximum)
    if (knobs.key_symbols != KEY_KNOB_ABSENT) {
        const int v = knobs.key_symbols;
        if (v >= 1 && v <= 64 / bits) msym = v; else if (v == 0) msym = 64 / bits;
    }
    al->msym = al->hstep = msym; al->key_bits = bits * msym; al->varlen = false; al->patch_span = msym - 1;
    al->few_ties = key_few_ties(key_fixed_partners(hist, n, msym));
    // variable-length codes when they save whole radix passes (skewed alphabets: text); the suffix sort of the general
    // Lyndon path keeps fixed-width codes with the pad symbol.  BWTS_VARLEN: 0 = never, 1 = always (tests), unset = when it pays;
    // BWTS_KEY_SYMBOLS alone asks for the fixed-width key it sizes
    const bool try_vl = !reserve_pad && al->sigma > 1 && knobs.varlen != 0 &&
                        !(knobs.key_symbols != KEY_KNOB_ABSENT && knobs.varlen == KEY_KNOB_ABSENT);
    uint32_t vcode[256]; uint8_t vlen[256];
    P->avg = P->entropy = 0; P->stack_high = 0;
    P->lmax = try_vl ? build_alphabetic_code(hist, n, vcode, vlen, &P->avg, &P->entropy, 1.0, &P->stack_high) : 0;
    P->code_built = try_vl && P->lmax <= VL_MAXLEN;
    memset(P->vtab, 0, sizeof P->vtab);
    for (int b = 0; b <= 64; b++) P->share[b] = 0.0;
    P->kb_iid = P->kb = 0; P->passes_fixed = (al->key_bits + 7) / 8; P->passes_var = 0;
    if (P->code_built) {
        for (int c = 0; c < 256; c++) P->vtab[c] = ((uint64_t)vlen[c] << 32) | vcode[c];
        P->kb_iid = iid_key_bits(hist, vlen, vcode, n, P->share);
    }
}

// Second half: the sample's say, BWTS_KEY_BITS, and the choice by radix passes.
static inline void key_plan_finish(KeyPlan *P, const KeySample &sample)
{
    Alphabet *al = &P->al;
    if (!P->code_built) return;
    const uint64_t *hist = P->hist; const uint64_t n = P->n;
    const int bits = al->bits, lmax = P->lmax;
    int kb = P->kb_iid;
    if (sample.kb_emp > kb) {
        // Repeats, not entropy, tie these positions, and no key width separates the copies of a long repeat: the
        // rounds on the tied list will.  Wider keys then only pay where they lengthen the first step (key bits /
        // longest code word) -- with short code words five digits (the packed passes) already give a step
        // of four symbols, and three fewer n-sized passes beat the few per cent of extra list elements (text 2^30,
        // longest code 9 bits: 64 / 48 / 40 / 32 key bits = 169 / 160 / 143 / 159 ms); with long code words (real
        // text: 205 symbols, 16 bits) every key bit counts (53.6 MiB: 16.1 / 18.5 / 20.6 / 23.3 ms).
        // (five packed digits whatever the model asks for at this n: text 2^31 / 2^32 with 48 against 40 bits = 334 / 660
        // against 295 / 590 ms)
        const int keep = 40;
        if (keep / lmax >= 4) kb = keep;
        else {
            kb = sample.kb_emp;
            // the fixed-width alternative was sized by the same model: let it use every symbol that fits
            al->msym = al->hstep = 64 / bits; al->key_bits = bits * al->msym; al->patch_span = al->msym - 1;
            al->few_ties = key_few_ties(key_fixed_partners(hist, n, al->msym));
        }
    }
    // BWTS_KEY_BITS (a key must hold its first symbol whole: the first step is >= 1)
    if (P->knobs.key_bits != KEY_KNOB_ABSENT) { const int v = P->knobs.key_bits; if (v >= 8 && v >= lmax && v <= 64) kb = v; }
    const int passes_fixed = (al->key_bits + 7) / 8, passes_var = (kb + 7) / 8;
    P->kb = kb; P->passes_fixed = passes_fixed; P->passes_var = passes_var;
    // equal pass counts: the variable-length key still holds more symbols when its words are shorter on average
    if (P->knobs.varlen == 1 || passes_var < passes_fixed || (passes_var == passes_fixed && P->avg < (double)bits - 0.25)) {
        al->varlen = true; al->key_bits = kb; al->patch_span = 64;
        al->few_ties = key_few_ties(sample.partners_of[kb] >= 0.0 ? sample.partners_of[kb] : (double)n * P->share[kb]);
        al->msym = al->hstep = kb / lmax < 1 ? 1 : kb / lmax;
    }
}

// Both halves: the engine's answer wherever it takes no sample (n < 2^22, and every sort but the cyclic one of a narrow forward).
static inline void key_plan(const uint64_t *hist, uint64_t n, bool reserve_pad, const KeyKnobs &knobs, const KeySample &sample, KeyPlan *P)
{
    key_plan_begin(hist, n, reserve_pad, knobs, P);
    key_plan_finish(P, sample);
}
