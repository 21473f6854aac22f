// x266_levels.hpp -- the compact level stream: the one copy of the scan tables and of the coefficient-group arithmetic that the kernels
// of levels_kernels.hip and the host helper xLevelScan share.  The statement is include/x266hip.h's (xLevelsPackGpu ...).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

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
__host__ __device__ inline unsigned level_cg_origin(unsigned k, unsigned g)
{
    constexpr LevelTab t = make_level_tab();
    return t.origin[k & 3u][g & 63u];
}
// y * 4 + x of scan position i of a 4x4 CG
__host__ __device__ constexpr unsigned level_scan4(unsigned i)
{
    constexpr LevelTab t = make_level_tab();
    return t.scan4[i & 15u];
}

}  // namespace x266
