// x266_ctu_tiles.hpp -- where a 64x64 CTU's 32x32 regions live in a tiled frame (x266_ref_block_t: 16x16 luma, 8 rows of
// interleaved U,V pairs per tile, tiles in raster order, tiles_x per row).  Shared by the CTU kernels of dct32_kernels.hip
// (the DCT32 forms) and transform_kernels.hip (the mixed transform set).
//
// A wave handles a region as 32 rows x 2 halves: lane (c, h) = (lane & 31, lane >> 5) holds row c, columns 16h .. 16h+15.
//   luma quadrant `part` (0..3: top-left, top-right, bottom-left, bottom-right): one 16-byte m_Y row, (c & 15) of ctu_luma_tile;
//   chroma (U and V at once): the 16-byte m_C rows (c & 7) of ctu_chroma_tile and the tile after it -- their even bytes are U
//   columns 16h .. 16h+15, the odd bytes V.
#pragma once

#include <cstddef>

namespace x266 {

// tile row / column of lane (c, h) in luma quadrant `part` of CTU (cy, cx)
__device__ __forceinline__ size_t ctu_luma_tile_row(size_t cy, unsigned part, unsigned c) { return cy * 4 + (part >> 1) * 2 + (c >> 4); }
__device__ __forceinline__ size_t ctu_luma_tile_col(size_t cx, unsigned part, unsigned h) { return cx * 4 + (part & 1) * 2 + h; }
__device__ __forceinline__ size_t ctu_luma_tile(size_t cy, size_t cx, unsigned part, unsigned c, unsigned h, int tiles_x)
{
    return ctu_luma_tile_row(cy, part, c) * (size_t)tiles_x + ctu_luma_tile_col(cx, part, h);
}

// the first of the two tiles that hold chroma row c, columns 16h .. 16h+15 of CTU (cy, cx); the second is the next tile
__device__ __forceinline__ size_t ctu_chroma_tile_row(size_t cy, unsigned c) { return cy * 4 + (c >> 3); }
__device__ __forceinline__ size_t ctu_chroma_tile_col(size_t cx, unsigned h) { return cx * 4 + 2 * h; }
__device__ __forceinline__ size_t ctu_chroma_tile(size_t cy, size_t cx, unsigned c, unsigned h, int tiles_x)
{
    return ctu_chroma_tile_row(cy, c) * (size_t)tiles_x + ctu_chroma_tile_col(cx, h);
}

// byte offsets of those rows inside a tile
__device__ __forceinline__ unsigned ctu_luma_row_offset(unsigned c) { return (c & 15) * 16; }
__device__ __forceinline__ unsigned ctu_chroma_row_offset(unsigned c) { return 256 + (c & 7) * 16; }

}  // namespace x266
