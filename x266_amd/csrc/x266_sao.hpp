// x266_sao.hpp -- sample adaptive offset: the one copy of the per-sample arithmetic and of the per-bin offset search that the kernels
// of sao_kernels.hip share (statistics, decision, the fused search, apply).  The statement is include/x266hip.h's (xSaoStatsGpu ...).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace x266 {

constexpr int kSaoBins = 48;                // per CTU and component: 4 EO classes x 4 categories, then 32 bands
constexpr int kSaoMaxOffset = 7;

__device__ __forceinline__ int sao_sign(int d) { return (d > 0) - (d < 0); }

// sign(c - a) + sign(c - b) in -2..2
__device__ __forceinline__ int sao_edge_sum(int c, int a, int b) { return sao_sign(c - a) + sao_sign(c - b); }

// the category of an edge sum: -2 -> 1 (valley), -1 -> 2, 0 -> 0, +1 -> 3, +2 -> 4 (peak)
__device__ __forceinline__ int sao_category_of_sum(int s) { return s == 0 ? 0 : (s < 0 ? s + 3 : s + 2); }

__device__ __forceinline__ int sao_category(int c, int a, int b) { return sao_category_of_sum(sao_edge_sum(c, a, b)); }

__device__ __forceinline__ int sao_band(int c) { return c >> 3; }

__device__ __forceinline__ int sao_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// R(h) = min(|h| + 1, 7), plus the sign bit of a non-zero band offset
__device__ __forceinline__ int sao_rate(int h, bool band)
{
    const int a = h < 0 ? -h : h;
    return (a + 1 < 7 ? a + 1 : 7) + ((band && h != 0) ? 1 : 0);
}

// The offset of one bin (count n, sum e of org - dec) in [lo, hi] and its cost J(h) = 16 (n h^2 - 2 h e) + lambda_q4 R(h): start at
// h0 = clamp(sign(e) ((2 |e| + n) / (2 n)), lo, hi) and walk towards 0; least J wins, among equal costs the smaller |h|.
// 32 bits: n <= 4096, |e| <= 4096 * 255, |h| <= 7 give |16 (n h^2 - 2 h e)| < 2.4e8 and lambda_q4 R <= 65535 * 8.
__device__ __forceinline__ int sao_offset_search(int n, int e, int lo, int hi, int lambda_q4, bool band, int &best_cost)
{
    int h0 = 0;
    if (n > 0) {
        const unsigned mag = (2u * (unsigned)(e < 0 ? -e : e) + (unsigned)n) / (2u * (unsigned)n);
        h0 = e < 0 ? -(int)mag : (int)mag;                               // |e| <= 255 n: mag <= 255
        h0 = h0 < lo ? lo : (h0 > hi ? hi : h0);
    }
    const int step = sao_sign(h0), steps = h0 < 0 ? -h0 : h0;
    int best = h0;
    best_cost = 16 * (n * h0 * h0 - 2 * h0 * e) + lambda_q4 * sao_rate(h0, band);
#pragma unroll
    for (int i = 1; i <= kSaoMaxOffset; ++i) {
        const int h = h0 - step * i;
        const int cost = 16 * (n * h * h - 2 * h * e) + lambda_q4 * sao_rate(h, band);
        if (i <= steps && cost <= best_cost) {                            // later candidates are nearer 0: they win ties
            best = h;
            best_cost = cost;
        }
    }
    return best;
}

// the range of bin e of a component: EO categories 1, 2 add, 3, 4 subtract; a band goes either way
__device__ __forceinline__ int sao_bin_search(int bin, int n, int e, int lambda_q4, int &best_cost)
{
    const bool band = bin >= 16;
    const int lo = (band || (bin & 2)) ? -kSaoMaxOffset : 0, hi = (band || !(bin & 2)) ? kSaoMaxOffset : 0;
    return sao_offset_search(n, e, lo, hi, lambda_q4, band, best_cost);
}

// EO of one sample from its edge sum and the record's four offsets: `lo` holds off[0], off[1], 0, off[2] as bytes, off3 is off[3]
__device__ __forceinline__ int sao_apply_edge(int c, int a, int b, uint32_t lo, int off3)
{
    const int idx = sao_edge_sum(c, a, b) + 2;                            // 0..4 = categories 1, 2, 0, 3, 4
    const int o = idx == 4 ? off3 : (int)(int8_t)(lo >> (8 * (idx & 3)));
    return sao_clip8(c + o);
}

// BO of one sample: the four offsets as the bytes of `offs`, from band `pos` on, wrapping at 32
__device__ __forceinline__ int sao_apply_band(int c, int pos, uint32_t offs)
{
    const int j = (sao_band(c) - pos) & 31;
    const int o = j < 4 ? (int)(int8_t)(offs >> (8 * (j & 3))) : 0;
    return sao_clip8(c + o);
}

}  // namespace x266
