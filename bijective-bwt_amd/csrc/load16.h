// load16.h -- 16 bytes from any address with aligned accesses only, for the kernels whose inputs are aligned but by luck (planes.hip,
// pieces.hip): the two aligned 16-byte pieces around the address are read and the bytes shifted into place in registers.  No access
// wider than a byte is made at an address that is not a multiple of its width, and nothing outside [lo, hi) is read.  Behind it, what
// planes.hip and delta.hip share on the way out: a tile's bytes in padded LDS units, and their store at any alignment.
#pragma once
#include "internal.h"
#include "planes_plan.h"

// the 16 bytes at byte sh (0 .. 15) of the 32 bytes a, b
__device__ __forceinline__ uint4 planes_funnel(uint4 a, uint4 b, u32 sh)
{
    const u32 D[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const u32 bytes = sh & 3u, words = sh >> 2;
    u32 e[7], o[4];
#pragma unroll
    for (int j = 0; j < 7; j++) e[j] = __builtin_amdgcn_alignbyte(D[j + 1], D[j], bytes);
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = words == 0 ? e[j] : (words == 1 ? e[j + 1] : (words == 2 ? e[j + 2] : e[j + 3]));
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// the aligned 16-byte piece at a, of which only bytes inside [lo, hi) are read (the others are 0)
__device__ __forceinline__ uint4 planes_piece(const u8 *a, const u8 *lo, const u8 *hi)
{
    const uintptr_t x = (uintptr_t)a, l = (uintptr_t)lo, h = (uintptr_t)hi;
    if (x >= l && x + 16 <= h) return *(const uint4 *)a;
    u32 w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i++)
        if (x + i >= l && x + i < h) w[i >> 2] |= (u32)a[i] << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the 16 bytes at p, at any alignment; what lies outside [lo, hi) reads as 0
__device__ __forceinline__ uint4 planes_load16(const u8 *p, const u8 *lo, const u8 *hi)
{
    const u32 sh = (u32)((uintptr_t)p & 15);
    const u8 *a = p - sh;
    const uint4 x = planes_piece(a, lo, hi);
    if (sh == 0) return x;
    return planes_funnel(x, planes_piece(a + 16, lo, hi), sh);
}

// ---- a tile's bytes through the LDS, out at any alignment (planes.hip, delta.hip) ----
// The LDS unit (16 bytes) of unit u of a stream: one unit of padding behind every eight, so that the eight lanes whose 16-byte stores
// the LDS takes together (units w apart in a join) fall on different banks.
#define PLANES_SLOT(u) ((u) + ((u) >> 3))

// byte i of a stream in LDS
__device__ __forceinline__ u32 planes_lds_byte(u32 i) { return 16u * PLANES_SLOT(i >> 4) + (i & 15u); }

// len bytes of a stream in LDS (unit u at PLANES_SLOT(u), one more unit readable behind the last) to dst, the whole workgroup
__device__ __forceinline__ void planes_stream_store(const uint4 *lds, u8 *dst, u32 len)
{
    const u32 tid = threadIdx.x;
    const u8 *bytes = (const u8 *)lds;
    u32 head = (16u - (u32)((uintptr_t)dst & 15)) & 15u;
    if (head > len) head = len;
    const u32 vecs = (len - head) / 16u, done = head + 16u * vecs;
    if (tid < head) dst[tid] = bytes[planes_lds_byte(tid)];
    // store v holds the stream's bytes [head + 16 v, head + 16 v + 16): from the units v and v + 1
    for (u32 v = tid; v < vecs; v += 256) {
        uint4 x = lds[PLANES_SLOT(v)];
        if (head) x = planes_funnel(x, lds[PLANES_SLOT(v + 1u)], head);
        ((uint4 *)(dst + head))[v] = x;
    }
    if (tid < len - done) dst[done + tid] = bytes[planes_lds_byte(done + tid)];
}

// tile j of a segment of width 1: PLANES_COPY_T bytes at most, copied through the LDS under the same discipline (planes_load16 in,
// planes_stream_store out); a thread takes every 256th unit of 16 bytes
__device__ __forceinline__ void planes_copy_tile(const u8 *__restrict__ in, u64 n, u64 seg, u64 len, u64 j, uint4 *lds, u8 *__restrict__ out)
{
    const u32 bytes = planes_copy_bytes(len, j), units = (bytes + 15u) / 16u;
    const u64 at = seg + j * PLANES_COPY_T;
    for (u32 u = threadIdx.x; u < units; u += 256) lds[PLANES_SLOT(u)] = planes_load16(in + at + 16u * u, in, in + n);
    __syncthreads();
    planes_stream_store(lds, out + at, bytes);
}

// the segment of tile t: the last one whose first tile is not behind t (every segment has a tile, so the firsts differ)
__device__ __forceinline__ u64 planes_tile_segment(const u64 *first, u64 count, u64 t)
{
    u64 lo = 0, hi = count;
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (first[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}
