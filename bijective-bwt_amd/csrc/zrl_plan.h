// zrl_plan.h -- the arithmetic of the zero-run coded form (include/bwts_zrl.h) that host and device share: how an input is cut, how
// many digits a run has, the decoder's step over one coded byte with its validity checks, and the serial statements of encoder and
// decoder.  Plain C++ with no dependency, like ec_plan.h: the kernels of zrl.hip, the host side of the calls and a stand-alone host
// program (tests/zrl_plan_check.cc, built with the sanitizers) all compile this file.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ZRL_HD __host__ __device__ static inline
#else
#define ZRL_HD static inline
#endif

#define ZRL_LOG_T 14u                    // tile: T = 16384 bytes of the side that is cut (the ranks of an encode, the coded bytes of a decode)
#define ZRL_T (1u << ZRL_LOG_T)
#define ZRL_MAX_DIGITS 36u               // a digit of index 35 stands for up to 2^36 zeros: the longest input
#define ZRL_MAX_N (1ull << 36)

// what a decoder can find wrong with a coded input
#define ZRL_BAD_PAYLOAD 1u               // the byte behind a 255 is neither 0 nor 1
#define ZRL_BAD_DIGIT 2u                 // a digit of index >= 36
#define ZRL_BAD_END 4u                   // a 255 as the last byte
#define ZRL_BAD_SUM 8u                   // the weights do not sum to n

ZRL_HD uint64_t zrl_tiles(uint64_t bytes) { return (bytes + ZRL_T - 1u) >> ZRL_LOG_T; }

// digits of a run of L >= 1 zeros: k = floor(log2(L + 1)).  L + 1 in binary is a 1 followed by the digits d[k-1] .. d[0], so
// digit i is bit i of L + 1.
ZRL_HD uint32_t zrl_digits(uint64_t L) { return 63u - (uint32_t)__builtin_clzll(L + 1u); }
ZRL_HD uint32_t zrl_digit(uint64_t L, uint32_t i) { return (uint32_t)((L + 1u) >> i) & 1u; }
// bytes a rank v >= 1 becomes
ZRL_HD uint32_t zrl_literal_bytes(uint32_t v) { return v >= 254u ? 2u : 1u; }

// The decoder's state in front of a coded byte: prev is 255 where the byte is a payload (and anything else where it is not), i the
// number of digits directly in front, pos the zeros and ranks that all bytes so far stand for.  The step returns the rank the byte
// puts at the old pos (1 .. 255), or 0 where it puts none: a digit moves pos over its zeros, a 255 waits for its payload.
struct zrl_state { uint32_t prev, i, err; uint64_t pos; };

ZRL_HD uint32_t zrl_step(zrl_state &s, uint32_t b)
{
    uint32_t v = 0;
    if (s.prev == 255u) {
        if (b > 1u) s.err |= ZRL_BAD_PAYLOAD;
        v = 254u + (b & 1u);
        s.pos++; s.i = 0; s.prev = 0;
    } else if (b == 255u) {
        s.i = 0; s.prev = 255u;
    } else if (b <= 1u) {
        if (s.i >= ZRL_MAX_DIGITS) s.err |= ZRL_BAD_DIGIT;
        else s.pos += (uint64_t)(b + 1u) << s.i;
        s.i++; s.prev = b;
    } else {
        v = b - 1u;
        s.pos++; s.i = 0; s.prev = b;
    }
    return v;
}

// The digits directly in front of position p of a coded input z (no other byte between), counted up to ZRL_MAX_DIGITS: what a decoder
// that starts at p must know, and all it must know besides whether z[p - 1] is 255.  It reads at most 37 bytes in front of p.
ZRL_HD uint32_t zrl_digits_before(const uint8_t *z, uint64_t p)
{
    uint32_t i = 0;
    while (i < ZRL_MAX_DIGITS && p > 0 && z[p - 1] <= 1u && !(p > 1 && z[p - 2] == 255u)) { i++; p--; }
    return i;
}

// the decoder's state in front of position p, for a decoder that starts there
ZRL_HD zrl_state zrl_state_at(const uint8_t *z, uint64_t p)
{
    zrl_state s;
    s.prev = p > 0 ? z[p - 1] : 0u;
    s.err = 0; s.pos = 0;
    s.i = s.prev == 255u ? 0u : zrl_digits_before(z, p);
    return s;
}

// The serial decoder's validation of a coded input of in_bytes < n bytes: 0, or the ZRL_BAD_* bits of what is wrong.  (The sum stops
// growing once it is past n: no weight is larger than 2^36, so it cannot wrap.)
ZRL_HD uint32_t zrl_check(const uint8_t *z, uint64_t in_bytes, uint64_t n)
{
    zrl_state s = {0u, 0u, 0u, 0u};
    for (uint64_t p = 0; p < in_bytes && s.pos <= n; p++) (void)zrl_step(s, z[p]);
    if (s.pos > n) return s.err | ZRL_BAD_SUM;
    if (s.prev == 255u) s.err |= ZRL_BAD_END;
    if (s.pos != n) s.err |= ZRL_BAD_SUM;
    return s.err;
}

// The serial decoder: out[0 .. n) from a coded input that zrl_check has passed.
ZRL_HD void zrl_decode_serial(const uint8_t *z, uint64_t in_bytes, uint8_t *out, uint64_t n)
{
    for (uint64_t p = 0; p < n; p++) out[p] = 0;
    zrl_state s = {0u, 0u, 0u, 0u};
    for (uint64_t p = 0; p < in_bytes; p++) {
        const uint64_t at = s.pos;
        const uint32_t v = zrl_step(s, z[p]);
        if (v && at < n) out[at] = (uint8_t)v;
    }
}

// The serial encoder: the m bytes the ranks r[0 .. n) become (out may be null: the count alone; it needs room for m bytes, at most
// 2 n + 36).  The caller stores the input instead where m >= n.
ZRL_HD uint64_t zrl_encode_serial(const uint8_t *r, uint64_t n, uint8_t *out)
{
    uint64_t m = 0, L = 0;
    for (uint64_t p = 0; p <= n; p++) {
        const uint32_t v = p < n ? r[p] : 256u;      // (256: the end closes a run like a rank does)
        if (v == 0) { L++; continue; }
        if (L) {
            const uint32_t k = zrl_digits(L);
            if (out) for (uint32_t i = 0; i < k; i++) out[m + i] = (uint8_t)zrl_digit(L, i);
            m += k; L = 0;
        }
        if (v == 256u) break;
        if (out) {
            if (v >= 254u) { out[m] = 255u; out[m + 1] = (uint8_t)(v - 254u); }
            else out[m] = (uint8_t)(v + 1u);
        }
        m += zrl_literal_bytes(v);
    }
    return m;
}
