// x266_lanes.hpp -- the one copy of the cross-lane reductions and scans of a 64-lane wave, and the tail the frame-totals kernels share
// (device only, gfx950).  Two mechanisms, by what the value is: a 32-bit sum inside a row of 16 lanes is DPP (no LDS traffic); whatever
// crosses rows or is 64 bits wide is a butterfly of __shfl_xor (ds_bpermute: address arithmetic, an LDS instruction and its latency), a
// 64-bit value as two 32-bit exchanges.  Integer sums, minima and maxima commute, so the order of a butterfly's steps never shows in a
// result; each order below is the one its first user had.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace x266 {

// ---- 32-bit sums without LDS traffic ---------------------------------------------------------------------------------------------------------
// x + (lane ^ 32's x): gfx950's v_permlane32_swap exchanges the upper half of one register with the lower half of another
__device__ __forceinline__ uint32_t sum_with_other_half(uint32_t x)
{
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);   // r[0] = {lo, lo}, r[1] = {hi, hi}
    return r[0] + r[1];
}
// sum over the lane's aligned group of SPAN = 2, 4, 8 or 16 lanes (every lane of the group ends up with it; SPAN = 1: x itself): two quad
// permutes, then the two row mirrors
template <int SPAN>
__device__ __forceinline__ uint32_t sum_over_span(uint32_t x)
{
    static_assert(SPAN == 1 || SPAN == 2 || SPAN == 4 || SPAN == 8 || SPAN == 16, "DPP reaches a row of 16 lanes");
    if (SPAN >= 2) x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, true);     // quad_perm [1,0,3,2]
    if (SPAN >= 4) x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, true);     // quad_perm [2,3,0,1]
    if (SPAN >= 8) x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x141, 0xF, 0xF, true);    // row_half_mirror
    if (SPAN >= 16) x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x140, 0xF, 0xF, true);   // row_mirror
    return x;
}
__device__ __forceinline__ uint32_t sum_over_row16(uint32_t x) { return sum_over_span<16>(x); }
// the sum over the wave, as a wave-uniform value: the four rows' sums added on the scalar side
__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
    x = sum_over_row16(x);
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 0) + (uint32_t)__builtin_amdgcn_readlane((int)x, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)x, 32) + (uint32_t)__builtin_amdgcn_readlane((int)x, 48);
}

// ---- 32-bit maximum and exclusive prefix sum -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_max(uint32_t x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t y = (uint32_t)__shfl_xor((int)x, o);
        x = x > y ? x : y;
    }
    return x;
}
// the sum of x over the lanes below this one
__device__ __forceinline__ uint32_t wave_exclusive_sum(uint32_t x, unsigned lane)
{
    uint32_t s = x;
#pragma unroll
    for (unsigned o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)s, o);
        if (lane >= o) s += t;
    }
    return s - x;
}

// ---- 64-bit values: two 32-bit exchanges ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t shfl_up64(uint64_t x, unsigned o)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, o), hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), o);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t x, unsigned o)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, (int)o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), (int)o);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t x, unsigned src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, (int)src), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), (int)src);
    return (uint64_t)hi << 32 | lo;
}
// The sum over the lanes that differ from this one in the bits `first` and above; every such lane ends up with it.  first = 1: the whole
// wave; first = 2: the lanes of this lane's parity (the source analysis' totals, whose even and odd lanes hold different sums).
template <typename T>
__device__ __forceinline__ T wave_sum(T x, unsigned first = 1)
{
    static_assert(sizeof(T) == 8, "uint64_t or int64_t; a 32-bit sum is wave_sum(uint32_t)");
#pragma unroll
    for (unsigned o = first; o < 64; o <<= 1) x += (T)shfl_xor64((uint64_t)x, o);
    return x;
}
// the least over the wave, in T's own order (signed for int64_t); every lane ends up with it.  Keys {cost : position} make the first of equal costs win.
template <typename T>
__device__ __forceinline__ T wave_min(T x)
{
    static_assert(sizeof(T) == 8, "uint64_t keys or int64_t");
#pragma unroll
    for (unsigned o = 32; o >= 1; o >>= 1) {
        const T y = (T)shfl_xor64((uint64_t)x, o);
        x = y < x ? y : x;
    }
    return x;
}

// ---- the tail of a frame-totals kernel ---------------------------------------------------------------------------------------------------------
// Every lane of a workgroup of kWaves waves brings N accumulators; lane tid < N * FIRST gets the whole workgroup's sum of slot tid (the other
// lanes 0).  FIRST = 1: slot k is accumulator k.  FIRST = 2: the even lanes' accumulator k is slot k, the odd lanes' slot N + k.  Each wave's
// sums go through LDS and are added in the fixed order 0 .. kWaves - 1: no atomics.  Every lane of the workgroup calls it (it holds a barrier).
template <unsigned kWaves, unsigned FIRST = 1, typename T, unsigned N>
__device__ __forceinline__ T workgroup_totals(const T (&acc)[N], unsigned tid)
{
    __shared__ T part[kWaves][N * FIRST];
    const unsigned lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (unsigned k = 0; k < N; ++k) {
        const T v = wave_sum(acc[k], FIRST);
        if (lane < FIRST) part[wave][N * lane + k] = v;
    }
    __syncthreads();
    T all = 0;
    if (tid < N * FIRST) {
#pragma unroll
        for (unsigned w = 0; w < kWaves; ++w) all += part[w][tid];
    }
    return all;
}

}  // namespace x266
