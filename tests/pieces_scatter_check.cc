// pieces_scatter_check.cc -- the edge arithmetic of scatter_pieces_kernel (csrc/pieces.hip) as pack_plan.h states it, driven on the
// host under the sanitizers: pieces_tile_at, scatter_tile_plan and scatter_edge_byte over every pairing of source and destination
// misalignment and lengths 1 .. 49, PIECES_T - 1, PIECES_T, PIECES_T + 1 and 2 PIECES_T + 1, at two places of the destination in its
// 256-byte line.  The kernel's accesses are rendered one after the other: every load and store is checked against the piece's own
// bytes and its own width, the copy is made with them from heap blocks of exactly the piece's length behind its misalignment, and
// every destination byte must have been written once, with the source's value.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pack_plan.h"

static uint64_t checks = 0;
#define CHECK(c)                                                                   \
    do {                                                                           \
        checks++;                                                                  \
        if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } \
    } while (0)

struct Piece {
    const uint8_t *src; uint8_t *dst; uint64_t bytes;
    std::vector<uint8_t> *written;       // how often a destination byte has been stored
};

static void load(const Piece &p, const uint8_t *at, uint32_t width, uint8_t *to)
{
    CHECK(((uintptr_t)at & (width - 1u)) == 0u);
    CHECK(at >= p.src && at + width <= p.src + p.bytes);
    memcpy(to, at, width);
}

static void store(const Piece &p, uint8_t *at, uint32_t width, const uint8_t *from)
{
    CHECK(((uintptr_t)at & (width - 1u)) == 0u);
    CHECK(at >= p.dst && at + width <= p.dst + p.bytes);
    memcpy(at, from, width);
    for (uint32_t i = 0; i < width; i++) (*p.written)[(size_t)(at - p.dst) + i]++;
}

// the kernel's loop over one piece, one access after the other
static void render(const Piece &p)
{
    const uint64_t ps = (uint64_t)(uintptr_t)p.src, pd = (uint64_t)(uintptr_t)p.dst, lead = pd & (PIECES_LINE - 1u);
    const uint64_t tiles = pieces_tiles(p.bytes, lead);
    uint64_t seen = 0;
    for (uint64_t j = 0; j < tiles; j++) {
        uint64_t at = 0;
        const uint32_t len = pieces_tile_at(p.bytes, lead, j, &at);
        CHECK(at == seen && len >= 1u && len <= PIECES_T && at + len <= p.bytes);
        CHECK(j == 0 || ((pd + at) & (PIECES_LINE - 1u)) == 0u);
        seen += len;
        const ScatterTile k = scatter_tile_plan(ps + at, pd + at, len, ps, ps + p.bytes);
        CHECK(k.head <= 15u && k.head + 16u * k.vecs <= len && len - (k.head + 16u * k.vecs) <= 15u);
        CHECK(k.v_lo <= k.v_hi && k.v_hi <= k.vecs && k.v_lo <= 1u && k.vecs - k.v_hi <= 1u);
        // the edge rule: a store is lost only where an aligned source piece of its own would leave the piece
        const uint64_t a = ps + at + k.head - k.sh;
        if (k.v_lo) CHECK(a < ps);
        if (k.v_hi < k.vecs) CHECK(k.sh && a + 16u * ((uint64_t)k.vecs + 1u) > ps + p.bytes);
        const uint8_t *s = p.src + at;
        uint8_t *d = p.dst + at;
        for (uint32_t lane = 0; lane < 64; lane++) {
            uint32_t i = 0;
            if (!scatter_edge_byte(k, len, lane, &i)) continue;
            CHECK(i < len);
            uint8_t b;
            load(p, s + i, 1, &b);
            store(p, d + i, 1, &b);
        }
        for (uint32_t v = k.v_lo; v < k.v_hi; v++) {
            uint8_t xy[32], out[16];
            load(p, s + k.head - k.sh + 16u * v, 16, xy);
            if (k.sh) load(p, s + k.head - k.sh + 16u * v + 16u, 16, xy + 16);
            memcpy(out, xy + k.sh, 16);
            store(p, d + k.head + 16u * v, 16, out);
        }
    }
    CHECK(seen == p.bytes);
}

static void one_piece(uint32_t sm, uint32_t dm, uint64_t bytes, uint32_t line_at)
{
    // the piece ends where its heap block ends; in front of it lie only the bytes of its misalignment
    void *sblock = nullptr, *dblock = nullptr;
    if (posix_memalign(&sblock, 16, (size_t)(sm + bytes)) || posix_memalign(&dblock, 256, (size_t)(line_at + dm + bytes))) exit(2);
    CHECK(sblock && dblock);
    uint8_t *src = (uint8_t *)sblock + sm, *dst = (uint8_t *)dblock + line_at + dm;
    CHECK(((uintptr_t)src & 15u) == sm && ((uintptr_t)dst & 15u) == dm);
    for (uint64_t i = 0; i < bytes; i++) src[i] = (uint8_t)(i * 131u + sm * 7u + dm + (i >> 8));
    memset(dst, 0xC7, (size_t)bytes);
    std::vector<uint8_t> written((size_t)bytes, 0);
    const Piece p = {src, dst, bytes, &written};
    render(p);
    for (uint64_t i = 0; i < bytes; i++) CHECK(written[(size_t)i] == 1u && dst[i] == src[i]);
    free(sblock);
    free(dblock);
}

int main()
{
    std::vector<uint64_t> lengths;
    for (uint64_t n = 1; n <= 49; n++) lengths.push_back(n);
    lengths.push_back(PIECES_T - 1u); lengths.push_back(PIECES_T); lengths.push_back(PIECES_T + 1u); lengths.push_back(2u * PIECES_T + 1u);
    for (uint32_t line_at : {0u, 224u})
        for (uint32_t sm = 0; sm < 16; sm++)
            for (uint32_t dm = 0; dm < 16; dm++)
                for (uint64_t n : lengths) one_piece(sm, dm, n, line_at);
    // a tile inside its piece loses nothing: bytes of the piece lie on both sides of every aligned piece it reads
    for (uint32_t sm = 0; sm < 16; sm++) {
        const uint64_t ps = 4096u + sm, bytes = 3u * PIECES_T;
        uint64_t at = 0;
        const uint32_t len = pieces_tile_at(bytes, 0, 1, &at);
        const ScatterTile k = scatter_tile_plan(ps + at, (1u << 20) + at, len, ps, ps + bytes);
        CHECK(len == PIECES_T && k.head == 0u && k.v_lo == 0u && k.v_hi == k.vecs && k.vecs == PIECES_T / 16u);
    }
    printf("%llu checks ok\n", (unsigned long long)checks);
    return 0;
}
