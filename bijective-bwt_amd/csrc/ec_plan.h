// ec_plan.h -- the arithmetic of the entropy-coded stream (include/bwts_ec.h, version 1) that host and device share: how an input
// is cut, what the fixed parts weigh, the bound, what makes a header, a table and a tile directory valid, and the exact reciprocal
// the encoder divides with.  Plain C++ with no dependency: the kernels of ec.hip, the host side of the calls and a stand-alone host
// program (tests/ec_plan_check.cc, built with the sanitizers) all compile this file.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define EC_HD __host__ __device__ static inline
#else
#define EC_HD static inline
#endif

#define EC_LOG_T 14u                     // tile: T = 16384 bytes, one wave
#define EC_LOG_K 4u                      // K = 16 tiles share one frequency table (a block of 256 KiB)
#define EC_PROB_BITS 12u
#define EC_T (1u << EC_LOG_T)
#define EC_K (1u << EC_LOG_K)
#define EC_M (1u << EC_PROB_BITS)
#define EC_L 65536u                      // lower end of the state interval; renormalisation moves 16 bits
#define EC_ROW 1024u                     // a lane owns 16 consecutive bytes of every row
#define EC_MAGIC 0x43455742u             // "BWEC"
#define EC_PARAMS (EC_LOG_T | EC_LOG_K << 8 | EC_PROB_BITS << 16)
#define EC_HEADER_BYTES 16u
#define EC_TABLE_BYTES 512u
#define EC_STATE_BYTES 256u
#define EC_MAX_N (1ull << 36)

EC_HD uint64_t ec_pad16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
EC_HD uint64_t ec_tiles(uint64_t n) { return (n + EC_T - 1u) >> EC_LOG_T; }
EC_HD uint64_t ec_blocks(uint64_t tiles) { return (tiles + EC_K - 1u) >> EC_LOG_K; }
// bytes of tile t of an input of n bytes (t < ec_tiles(n))
EC_HD uint32_t ec_tile_len(uint64_t n, uint64_t t)
{
    const uint64_t left = n - (t << EC_LOG_T);
    return left < EC_T ? (uint32_t)left : EC_T;
}
EC_HD uint32_t ec_rows(uint32_t len) { return (len + EC_ROW - 1u) / EC_ROW; }
// header, tables and padded directory: everything in front of the payloads
EC_HD uint64_t ec_fixed_bytes(uint64_t n)
{
    const uint64_t nt = ec_tiles(n);
    return EC_HEADER_BYTES + (uint64_t)EC_TABLE_BYTES * ec_blocks(nt) + ec_pad16(4u * nt);
}
// no step emits more than one word per symbol: 2 n bytes of words, and per tile 256 bytes of states and less than 16 of padding
EC_HD uint64_t ec_bound_bytes(uint64_t n) { return ec_fixed_bytes(n) + 272u * ec_tiles(n) + 2u * n; }
// the smallest stream an input of n bytes can have (every tile only its states)
EC_HD uint64_t ec_least_bytes(uint64_t n) { return ec_fixed_bytes(n) + (uint64_t)EC_STATE_BYTES * ec_tiles(n); }
// payload bytes of a tile that emitted `words` words
EC_HD uint32_t ec_payload_bytes(uint32_t words) { return (uint32_t)ec_pad16(EC_STATE_BYTES + 2u * (uint64_t)words); }

EC_HD uint32_t ec_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
EC_HD void ec_put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

EC_HD void ec_header_write(uint8_t h[16], uint64_t n)
{
    ec_put32(h, EC_MAGIC); ec_put32(h + 4, EC_PARAMS); ec_put32(h + 8, (uint32_t)n); ec_put32(h + 12, (uint32_t)(n >> 32));
}

// 0 and *n, or -1: wrong magic or parameters, n == 0
EC_HD int ec_header_parse(const uint8_t h[16], uint64_t *n)
{
    if (ec_le32(h) != EC_MAGIC || ec_le32(h + 4) != EC_PARAMS) return -1;
    const uint64_t v = (uint64_t)ec_le32(h + 8) | (uint64_t)ec_le32(h + 12) << 32;
    if (v == 0) return -1;
    *n = v;
    return 0;
}

// a payload of a tile of len bytes: its states, whole 16-byte units, and no more words than symbols
EC_HD bool ec_size_ok(uint64_t size, uint32_t len)
{
    return size >= EC_STATE_BYTES && (size & 15u) == 0 && size <= ec_pad16(EC_STATE_BYTES + 2u * (uint64_t)len);
}

// the frequencies of one block: 256 x u16, little-endian, summing to 4096
EC_HD bool ec_table_ok(const uint8_t *tab)
{
    uint32_t sum = 0;
    for (int s = 0; s < 256; s++) sum += (uint32_t)tab[2 * s] | (uint32_t)tab[2 * s + 1] << 8;
    return sum == EC_M;
}

// The directory of an input of n bytes (dir: nt x u32 and the zero padding behind them) in front of payload_bytes bytes of payloads:
// every size valid for its tile, none reaching past the end, all of them together exactly payload_bytes, the padding zero.
// offsets (nt + 1 entries, may be null) receives where each payload starts, counted from the first, and the total.
EC_HD int ec_dir_check(const uint8_t *dir, uint64_t n, uint64_t payload_bytes, uint64_t *offsets)
{
    const uint64_t nt = ec_tiles(n);
    uint64_t at = 0;
    for (uint64_t t = 0; t < nt; t++) {
        const uint64_t size = ec_le32(dir + 4u * t);
        if (offsets) offsets[t] = at;
        if (!ec_size_ok(size, ec_tile_len(n, t)) || size > payload_bytes - at) return -1;
        at += size;
    }
    if (offsets) offsets[nt] = at;
    if (at != payload_bytes) return -1;
    for (uint64_t i = 4u * nt; i < ec_pad16(4u * nt); i++)
        if (dir[i]) return -1;
    return 0;
}

// Everything of a stream that can be judged without decoding a payload.  0 and *n, or -1.
EC_HD int ec_stream_check(const uint8_t *stream, uint64_t in_bytes, uint64_t *n)
{
    uint64_t v;
    if (in_bytes < EC_HEADER_BYTES || (in_bytes & 15u) || ec_header_parse(stream, &v) != 0 || v > EC_MAX_N) return -1;
    if (in_bytes < ec_least_bytes(v)) return -1;
    const uint64_t nb = ec_blocks(ec_tiles(v));
    for (uint64_t b = 0; b < nb; b++)
        if (!ec_table_ok(stream + EC_HEADER_BYTES + b * EC_TABLE_BYTES)) return -1;
    if (ec_dir_check(stream + EC_HEADER_BYTES + nb * EC_TABLE_BYTES, v, in_bytes - ec_fixed_bytes(v), nullptr) != 0) return -1;
    *n = v;
    return 0;
}

// floor(x / f) for every 32-bit x and 1 <= f <= 4096 without a divide (Granlund and Montgomery, "Division by invariant integers using
// multiplication", figure 4.1): with l = ceil(log2 f) and m = floor(2^32 (2^l - f) / f) + 1, t = high word of m x and
// q = (t + ((x - t) >> min(l, 1))) >> max(l - 1, 0).  x - t does not underflow (t <= x) and t + ((x - t) >> 1) fits 32 bits.
struct ec_recip { uint32_t m, sh1, sh2; };

EC_HD ec_recip ec_recip_make(uint32_t f)
{
    uint32_t l = 0;
    while ((1u << l) < f) l++;
    ec_recip r;
    r.m = (uint32_t)((((uint64_t)((1u << l) - f)) << 32) / f) + 1u;
    r.sh1 = l < 1u ? l : 1u;
    r.sh2 = l > 1u ? l - 1u : 0u;
    return r;
}

EC_HD uint32_t ec_div(uint32_t x, uint32_t m, uint32_t sh1, uint32_t sh2)
{
    const uint32_t t = (uint32_t)(((uint64_t)x * m) >> 32);
    return (t + ((x - t) >> sh1)) >> sh2;
}

// One encoder step on a state that has been renormalised for f (x < f 2^20): x = floor(x / f) 4096 + x mod f + c.
EC_HD uint32_t ec_encode_step(uint32_t x, uint32_t f, uint32_t c, uint32_t m, uint32_t sh1, uint32_t sh2)
{
    const uint32_t q = ec_div(x, m, sh1, sh2);
    return x + q * (EC_M - f) + c;
}

// Frequencies of one block from its byte counts (the stream's rule, in order): f = 0 where h = 0, else max(1, floor(4096 h / m)); the
// difference to 4096 goes, once, to the largest f when it is missing, and comes off the then largest f one at a time when it is too
// much (lowest symbol on ties).  The serial statement of what the normalising kernel does a wave wide.
EC_HD void ec_normalise(const uint64_t h[256], uint16_t f[256])
{
    uint64_t m = 0;
    for (int s = 0; s < 256; s++) m += h[s];
    int64_t d = EC_M;
    for (int s = 0; s < 256; s++) {
        uint64_t v = h[s] ? h[s] * EC_M / m : 0;
        if (h[s] && v == 0) v = 1;
        f[s] = (uint16_t)v;
        d -= (int64_t)v;
    }
    while (d != 0) {
        int best = 0;
        for (int s = 1; s < 256; s++)
            if (f[s] > f[best]) best = s;
        if (d > 0) { f[best] = (uint16_t)(f[best] + d); d = 0; }
        else { f[best]--; d++; }
    }
}
