// x266_levels.hpp -- the compact level stream: the one copy of the scan tables and of the coefficient-group arithmetic that the kernels
// of levels_kernels.hip and the host helper xLevelScan share, and the offset scan that the level stream and the motion stream
// (motion_kernels.hip) share.  The statement is include/x266hip.h's (xLevelsPackGpu ...).
// The tables are plain C++ (a host-only driver includes them through x266_entropy.hpp); the scan kernel exists under hipcc alone.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/x266hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "x266_lanes.hpp"
#define X266_HD __host__ __device__
#else
#define X266_HD
#endif

namespace x266 {

constexpr unsigned kLevelsRegionWords = 1024;      // levels of a region
constexpr unsigned kLevelsMaxWords = 64 + 1024;    // a region's payload at most: 64 maps and 1024 levels
constexpr unsigned kLevelsScanChunk = 1024;        // regions the offset scan's one workgroup takes per step (xLevelsScanChunk)

// Diagonal scan of an M x M grid: positions ordered by x + y, then by x.  x and y of scan index i.
struct LevelDiag {
    uint8_t x[64], y[64];
};
constexpr LevelDiag level_diag(unsigned m)
{
    LevelDiag d = {};
    unsigned i = 0;
    for (unsigned s = 0; s + 1 < 2 * m; ++s)
        for (unsigned x = 0; x < m; ++x)
            if (s >= x && s - x < m) {
                d.x[i] = (uint8_t)x;
                d.y[i] = (uint8_t)(s - x);
                ++i;
            }
    return d;
}

// origin[k][g]: the index inside its region of the top-left level of CG bit g of a region of N = 4 << k blocks, g = blk (N / 4)^2 + s
// with s the CG's scan position in block blk; scan4[i]: y * 4 + x of scan position i of a CG
struct LevelTab {
    uint16_t origin[4][64];
    uint8_t scan4[16];
};
constexpr LevelTab make_level_tab()
{
    LevelTab t = {};
    for (unsigned k = 0; k < 4; ++k) {
        const unsigned n = 4u << k, m = n / 4, per_block = m * m;
        const LevelDiag d = level_diag(m);
        for (unsigned g = 0; g < 64; ++g) {
            const unsigned blk = g / per_block, s = g % per_block;
            t.origin[k][g] = (uint16_t)(blk * n * n + 4u * d.y[s] * n + 4u * d.x[s]);
        }
    }
    const LevelDiag d4 = level_diag(4);
    for (unsigned i = 0; i < 16; ++i) t.scan4[i] = (uint8_t)(d4.y[i] * 4 + d4.x[i]);
    return t;
}

// k = class & 3 (N = 4 << k), g = 0..63
X266_HD inline unsigned level_cg_origin(unsigned k, unsigned g)
{
    constexpr LevelTab t = make_level_tab();
    return t.origin[k & 3u][g & 63u];
}
// y * 4 + x of scan position i of a 4x4 CG
X266_HD constexpr unsigned level_scan4(unsigned i)
{
    constexpr LevelTab t = make_level_tab();
    return t.scan4[i & 15u];
}

#if defined(__HIPCC__)
// The offset scan of a compact stream's records: offset[r] = the sum of n_words over the records before r; total[0] = the sum over all,
// total[1] = the leading records whose payload fits.  One workgroup.  Record is x266_level_region_t (levels_kernels.hip) or
// x266_motion_ctu_t (motion_kernels.hip) or x266_entropy_region_t (entropy_kernels.hip), which share their first 20 bytes: only n_words is read and only offset written.
template <typename Record>
__global__ __launch_bounds__(kLevelsScanChunk) void levels_scan_kernel(Record *region, size_t n_regions, uint64_t cap_words, uint64_t *total)
{
    constexpr unsigned kWaves = kLevelsScanChunk / 64;
    __shared__ uint32_t wave_words[kWaves], wave_fit[kWaves];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t carry = 0, fit = 0;
    uint32_t ahead = tid < n_regions ? region[tid].n_words : 0u;
    for (size_t base = 0; base < n_regions; base += kLevelsScanChunk) {
        const size_t i = base + tid;
        uint32_t n_words = ahead;
        size_t next = i + kLevelsScanChunk;
        asm volatile("" : "+v"(n_words), "+v"(next));                       // this step's value has landed BEFORE the next load is issued: the wait
        ahead = next < n_regions ? region[next].n_words : 0u;               // for it is not a wait for that one, which flies over this step's barriers
        const uint32_t below = wave_exclusive_sum(n_words, lane);
        if (lane == 63) wave_words[wave] = below + n_words;
        __syncthreads();
        uint32_t before = 0, chunk = 0;
#pragma unroll
        for (unsigned w = 0; w < kWaves; ++w) {
            const uint32_t v = wave_words[w];
            before += w < wave ? v : 0u;
            chunk += v;
        }
        const uint64_t offset = carry + before + below;
        const bool fits = i < n_regions && offset <= cap_words && n_words <= cap_words - offset;
        if (i < n_regions) region[i].offset = offset;
        const uint64_t fitting = __ballot(fits);
        if (lane == 0) wave_fit[wave] = (uint32_t)__popcll(fitting);
        __syncthreads();
        uint32_t f = 0;
#pragma unroll
        for (unsigned w = 0; w < kWaves; ++w) f += wave_fit[w];
        carry += chunk;
        fit += f;
        __syncthreads();                                                    // the two arrays are written again in the next step
    }
    if (tid == 0) {
        total[0] = carry;
        total[1] = fit;
    }
}
#endif

}  // namespace x266
