// delta_words.h -- a thread's 16 elements of w bytes in registers, for the kernels that walk delta.hip's tiles (delta.hip, estimate.hip):
// the word an element is worked on in, element i of the little-endian words of W 16-byte loads, and delta_plan.h's zigzag at a
// constant width.
#pragma once
#include "internal.h"
#include "load16.h"
#include "delta_plan.h"

// elements are worked on in 32 bits, 8-byte ones in 64
template <int W> struct DeltaWord { typedef u32 T; };
template <> struct DeltaWord<8> { typedef u64 T; };

template <int W>
__device__ __forceinline__ typename DeltaWord<W>::T delta_mask_t()
{
    if constexpr (W == 8) return ~0ull;
    else if constexpr (W == 4) return ~0u;
    else return (1u << (8 * W)) - 1u;
}

// element i of the little-endian words D (i a constant after unrolling), and its place in words that were zero
template <int W>
__device__ __forceinline__ typename DeltaWord<W>::T delta_get(const u32 *D, int i)
{
    if constexpr (W == 8) return (u64)D[2 * i] | ((u64)D[2 * i + 1] << 32);
    else if constexpr (W == 4) return D[i];
    else if constexpr (W == 2) return (D[i >> 1] >> (16 * (i & 1))) & 0xffffu;
    else return (D[i >> 2] >> (8 * (i & 3))) & 0xffu;
}

template <int W>
__device__ __forceinline__ void delta_put(u32 *O, int i, typename DeltaWord<W>::T v)
{
    if constexpr (W == 8) { O[2 * i] = (u32)v; O[2 * i + 1] = (u32)(v >> 32); }
    else if constexpr (W == 4) O[i] = v;
    else if constexpr (W == 2) O[i >> 1] |= v << (16 * (i & 1));
    else O[i >> 2] |= v << (8 * (i & 3));
}

// delta_plan.h's delta_zigzag and delta_unzigzag at a constant width
template <int W>
__device__ __forceinline__ typename DeltaWord<W>::T delta_zig(typename DeltaWord<W>::T d)
{
    typedef typename DeltaWord<W>::T T;
    return ((T)(d << 1) ^ (T)(0 - ((d >> (8 * W - 1)) & 1u))) & delta_mask_t<W>();
}

template <int W>
__device__ __forceinline__ typename DeltaWord<W>::T delta_unzig(typename DeltaWord<W>::T z)
{
    typedef typename DeltaWord<W>::T T;
    return ((z >> 1) ^ (T)(0 - (z & 1u))) & delta_mask_t<W>();
}

// the 16 elements at p (element `at` of a tile whose thread holds them): W 16-byte loads at any alignment; what lies outside the
// call's input [in, in + n) reads as 0
template <int W>
__device__ __forceinline__ void delta_load16(const u8 *p, const u8 *__restrict__ in, u64 n, u32 *D)
{
#pragma unroll
    for (int v = 0; v < W; v++) {
        const uint4 x = planes_load16(p + 16 * v, in, in + n);
        D[4 * v] = x.x; D[4 * v + 1] = x.y; D[4 * v + 2] = x.z; D[4 * v + 3] = x.w;
    }
}
