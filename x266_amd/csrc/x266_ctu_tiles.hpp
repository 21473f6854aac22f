// x266_ctu_tiles.hpp -- where a 64x64 CTU's 32x32 regions live in a tiled frame (x266_ref_block_t: 16x16 luma, 8 rows of
// interleaved U,V pairs per tile, tiles in raster order, tiles_x per row).  Shared by the CTU kernels of dct32_kernels.hip
// (the DCT32 forms) and transform_kernels.hip (the mixed transform set).  At the end: the frame geometry and the 16-lanes-per-CTU map of the
// analysis kernels (aq_kernels.hip, lookahead_kernels.hip, quality_kernels.hip).
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

// A frame as the analysis kernels see it (source analysis, lookahead, quality): tiles, and CTUs of 4 x 4 tiles whose last column and row
// may be cut by the frame's edge.
struct TileFrame {
    unsigned tiles_w, tiles_h, ctus_w;
    size_t n_ctu;
};

inline TileFrame tile_frame(int width, int height)
{
    TileFrame f;
    f.tiles_w = (unsigned)(width / 16);
    f.tiles_h = (unsigned)(height / 16);
    f.ctus_w = (f.tiles_w + 3) / 4;
    f.n_ctu = (size_t)f.ctus_w * ((f.tiles_h + 3) / 4);
    return f;
}

// A row of 16 lanes per CTU, lane i its tile (i & 3, i >> 2): the CTU and the tile index t of thread `thread` of workgroup `block` in a
// one-dimensional grid of waves_per_wg waves each.  t is meaningful where in_frame holds.
struct CtuLane {
    size_t ctu, t;
    bool ctu_ok, in_frame;      // the CTU is one of the frame's; and the tile lies inside the frame
};

__device__ __forceinline__ CtuLane ctu_lane(unsigned thread, unsigned block, unsigned waves_per_wg, const TileFrame &f)
{
    const unsigned i = thread & 15;
    CtuLane m;
    m.ctu = ((size_t)block * (64 * waves_per_wg) + thread) >> 4;
    m.ctu_ok = m.ctu < f.n_ctu;
    const size_t cy = m.ctu / f.ctus_w, cx = m.ctu % f.ctus_w;
    const size_t tx = cx * 4 + (i & 3), ty = cy * 4 + (i >> 2);
    m.in_frame = m.ctu_ok && tx < f.tiles_w && ty < f.tiles_h;
    m.t = ty * f.tiles_w + tx;
    return m;
}

}  // namespace x266
