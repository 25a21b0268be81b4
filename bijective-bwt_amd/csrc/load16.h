// load16.h -- 16 bytes from any address with aligned accesses only, for the kernels whose inputs are aligned but by luck (planes.hip,
// pieces.hip): the two aligned 16-byte pieces around the address are read and the bytes shifted into place in registers.  No access
// wider than a byte is made at an address that is not a multiple of its width, and nothing outside [lo, hi) is read.
#pragma once
#include "internal.h"

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
