// x266_quant.hpp -- the flat scalar quantiser of include/x266hip.h (xQuantRegionsGpu), shared by the region kernel of
// quant_kernels.hip and the fused CTU kernel of dct32_kernels.hip: both call the same two functions on the same parameters, so
// "the fused call is bit-identical to the chain" holds by construction.
//
// For an N x N block, n = log2 N in 2..5, qp in 0..51, rounding in 0..511 (units of 1/512):
//     f[6] = {26214, 23302, 20560, 18396, 16384, 14564}      g[6] = {40, 45, 51, 57, 64, 72}
//     qbits = 14 + qp/6 + (7 - n)
//     level = sign(c) * ((|c| * f[qp%6] + (rounding << (qbits - 9))) >> qbits)
//     coef' = clip_int16((level * (g[qp%6] << (qp/6)) + (1 << (n - 2))) >> (n - 1))         (arithmetic shift)
// The constants are those of HEVC / VVC at 8-bit depth as recalled, unverified offline; the arithmetic here is the contract.
// What follows from it, and what the code below relies on:
//   * qbits >= 16, so qbits - 9 >= 7 and the rounding offset is a left shift;
//   * |c| <= 32768 gives |level| <= 13108: the forward direction needs no clip;
//   * |c| * f + offset < 2^30 and |level| * (g << qp/6) < 2^30 for every int16 level: 32-bit arithmetic is exact, and |c|, f, the
//     level and g << qp/6 each fit in 16 bits, so both products are the 24-bit multiply-add forms (v_mad_u32_u24 / v_mad_i32_i24,
//     full rate) and not the quarter-rate 32-bit multiply;
//   * the dequantiser does need its int16 clip: level 13107 at qp 0, n = 5 gives (13107 * 40 + 8) >> 4 = 32768.
// Everything in QuantParams depends on (n, qp, rounding) only, which are uniform per region: the kernels read the class and qp
// bytes with uniform_byte (x266_device.hpp), so a wave computes the parameters once, on the scalar side.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"

namespace x266 {

struct QuantParams {
    unsigned f, offset, qbits;      // forward: (|c| * f + offset) >> qbits
    int scale, add, shift;          // inverse: (level * scale + add) >> shift, then the int16 clip
};

__device__ __forceinline__ QuantParams quant_params(unsigned n, unsigned qp, unsigned rounding)
{
    const unsigned per = qp / 6u, rem = qp - per * 6u;
    // f[rem] | g[rem] << 16, selected without a table in memory
    const unsigned fg = rem == 0 ? (26214u | 40u << 16) : rem == 1 ? (23302u | 45u << 16) : rem == 2 ? (20560u | 51u << 16) :
                        rem == 3 ? (18396u | 57u << 16) : rem == 4 ? (16384u | 64u << 16) : (14564u | 72u << 16);
    QuantParams p;
    p.f = fg & 0xFFFFu;
    p.qbits = 14u + per + (7u - n);
    p.offset = rounding << (p.qbits - 9u);
    p.scale = (int)((fg >> 16) << per);
    p.add = 1 << (n - 2u);
    p.shift = (int)n - 1;
    return p;
}

// one coefficient (any int16 value, sign-extended) -> its level
__device__ __forceinline__ int quantise(int c, const QuantParams &p)
{
    const int s = c >> 31;
    const unsigned a = (unsigned)((c ^ s) - s);
    const int lvl = (int)((__umul24(a, p.f) + p.offset) >> p.qbits);
    return (lvl ^ s) - s;
}

// one level (any int16 value, sign-extended) -> its coefficient
__device__ __forceinline__ int dequantise(int level, const QuantParams &p)
{
    const int v = (__mul24(level, p.scale) + p.add) >> p.shift;
    return v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
}

// two int16 samples in a dword
__device__ __forceinline__ uint32_t quantise_pair(uint32_t w, const QuantParams &p, unsigned &nonzero)
{
    const int lo = quantise((int)(int16_t)(w & 0xFFFFu), p), hi = quantise((int)w >> 16, p);
    nonzero += (lo != 0) + (hi != 0);
    return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
}

__device__ __forceinline__ uint32_t dequantise_pair(uint32_t w, const QuantParams &p)
{
    const int lo = dequantise((int)(int16_t)(w & 0xFFFFu), p), hi = dequantise((int)w >> 16, p);
    return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
}

}  // namespace x266
