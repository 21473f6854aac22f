// x266_subpel_blocks.hpp -- the per-group pieces of quarter-sample prediction and scoring on tiled frames, ONE copy for
// subpel_kernels.hip (motion compensation, the bi-directional costs, the refinements) and partition_kernels.hip (the inter partition
// decision): the 16 bytes of a clamped window row, where a block's window row lies, the vertical stage of a lane's four outputs over
// the group's LDS slot, and the 8x8 Hadamard over a group of 16 lanes.  The filters and their rounding are x266_interp.hpp's.
#pragma once

#include <cstddef>
#include <cstdint>

#include "x266_device.hpp"
#include "x266_interp.hpp"

namespace x266 {

// The 16 bytes of one clamped plane row from element xs on (luma: samples, chroma: (U, V) pairs), `row` = the row's bytes in tile
// column 0; a row of either plane is `width` bytes, 16 per tile.  Spans inside the frame are five aligned dwords (each within one
// 16-byte tile row; one that would start past the row is moved back and holds nothing that is used) and funnel shifts, spans that
// cross the left or right edge are read element by element with clamped x.
template <bool CHROMA>
__device__ __forceinline__ void load_window_row(const uint8_t *row, int xs, int width, uint32_t (&w)[4])
{
    const int pw = CHROMA ? width >> 1 : width, used = CHROMA ? 7 : 15;
    if (xs >= 0 && xs + used - 1 <= pw - 1) {
        const int x0 = CHROMA ? 2 * xs : xs, xa = x0 & ~3;
        uint32_t d[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int x = xa + 4 * k < width - 4 ? xa + 4 * k : width - 4;
            d[k] = *reinterpret_cast<const uint32_t *>(row + (size_t)(x >> 4) * 512 + (x & 15));
        }
        const unsigned sh = (unsigned)(x0 & 3) * 8;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = __builtin_amdgcn_alignbit(d[k + 1], d[k], sh);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = 0;
#pragma unroll
        for (int j = 0; j < (CHROMA ? 8 : 16); ++j) {
            int x = xs + j;
            x = x < 0 ? 0 : (x > pw - 1 ? pw - 1 : x);
            if (CHROMA) w[j >> 1] |= (uint32_t)*reinterpret_cast<const uint16_t *>(row + (size_t)(x >> 3) * 512 + (x & 7) * 2) << (16 * (j & 1));
            else        w[j >> 2] |= (uint32_t)row[(size_t)(x >> 4) * 512 + (x & 15)] << (8 * (j & 3));
        }
    }
}

// Where window row l of block `blk` (0..3, raster) of tile (tx, ty) lies under the vector r: the row's bytes in tile column 0 (the row
// index clamped into the plane), the element its first tap reads, and the two phases.
template <bool CHROMA>
struct WindowRow { const uint8_t *row; int xs, fx, fy; };

template <bool CHROMA>
__device__ __forceinline__ WindowRow<CHROMA> window_row(const x266_ref_block_t *ref, x266_me_result_t r, int height, int tiles_x, int tx, int ty, int blk, int l)
{
    typedef Interp<CHROMA> I;
    constexpr int edge = CHROMA ? 4 : 8, lg = I::kLog2Phases;
    const int ph = CHROMA ? height >> 1 : height;
    int sy = (ty * 2 + (blk >> 1)) * edge + (r.mvy >> lg) - I::kBefore + l;
    sy = sy < 0 ? 0 : (sy > ph - 1 ? ph - 1 : sy);
    WindowRow<CHROMA> s;
    s.row = reinterpret_cast<const uint8_t *>(ref) + (CHROMA ? 256 : 0) + (size_t)(sy >> (CHROMA ? 3 : 4)) * (size_t)tiles_x * 512 + (sy & (CHROMA ? 7 : 15)) * 16;
    s.xs = (tx * 2 + (blk & 1)) * edge + (r.mvx >> lg) - I::kBefore;
    s.fx = r.mvx & ((1 << lg) - 1);
    s.fy = r.mvy & ((1 << lg) - 1);
    return s;
}

// the vertical stage of the lane's four outputs (row l >> 1, half l & 1 of the block) over the group's slot, unrounded
template <bool CHROMA>
__device__ __forceinline__ void vertical_v4(const v4i *slot, int fy, int l, int (&v)[4])
{
    typedef Interp<CHROMA> I;
    int t[8];
    interp_taps<CHROMA>(fy, t);
    const int y = l >> 1, half = l & 1;
    uint2 rows[I::kTaps];
#pragma unroll
    for (int k = 0; k < I::kTaps; ++k) {
        const v4i r = slot[y + k];
        rows[k] = half ? make_uint2((uint32_t)r[2], (uint32_t)r[3]) : make_uint2((uint32_t)r[0], (uint32_t)r[1]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int col[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < I::kTaps; ++k) col[k] = hsum_of(c < 2 ? rows[k].x : rows[k].y, c & 1);
        v[c] = interp_vertical_v<CHROMA>(col, t);
    }
}

// index of 8x8 luma block `blk` of tile `tile` in the raster order of blocks
__device__ __forceinline__ size_t block_of_tile(size_t tile, int tiles_x, int blk, int *tx, int *ty)
{
    const size_t y = tile / (size_t)tiles_x, x = tile - y * (size_t)tiles_x;
    *tx = (int)x;
    *ty = (int)y;
    return (y * 2 + (size_t)(blk >> 1)) * (size_t)(2 * tiles_x) + x * 2 + (size_t)(blk & 1);
}

// The four bytes of the current frame that lane l of a block's group of 16 holds: row l >> 1, half l & 1 of block `blk` of the tile.
__device__ __forceinline__ uint32_t cur_block_word(const x266_ref_block_t *tile, int blk, int l)
{
    return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(tile) + ((blk >> 1) * 8 + (l >> 1)) * 16 + (blk & 1) * 8 + (l & 1) * 4);
}

// satd8x8 of an 8x8 block of differences held by a group of 16 lanes, four of one row half per lane (lane l: row l >> 1, half l & 1):
// two Hadamard stages inside the lane, one with lane ^ 1 (the other half of the row), three with lane ^ 2, 4, 8 (the rows).  The sum of
// |coefficients| depends on neither the order nor the signs of the butterflies; (sum + 2) >> 2 as satd8x8, in every lane of the group.
__device__ __forceinline__ uint32_t satd8x8_group16(int (&d)[4], int l)
{
    const int a0 = d[0] + d[1], a1 = d[0] - d[1], a2 = d[2] + d[3], a3 = d[2] - d[3];
    d[0] = a0 + a2;
    d[1] = a1 + a3;
    d[2] = a0 - a2;
    d[3] = a1 - a3;
#pragma unroll
    for (int m = 1; m <= 8; m <<= 1)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int o = __shfl_xor(d[c], m);
            d[c] = (l & m) ? o - d[c] : d[c] + o;
        }
    uint32_t sum = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) sum += (uint32_t)(d[c] < 0 ? -d[c] : d[c]);
#pragma unroll
    for (int m = 1; m <= 8; m <<= 1) sum += (uint32_t)__shfl_xor((int)sum, m);
    return (sum + 2) >> 2;
}

}  // namespace x266
