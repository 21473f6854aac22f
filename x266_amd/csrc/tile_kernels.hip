// tile_kernels.hip -- frame container conversion and residual formation for gfx950
// (the data formats either side of the transform / SATD kernels).
//
// Reference: ref_block_t (src/x266.cpp:56-63): a frame is a raster of 512-byte tiles,
//   m_Y[16*16] luma, m_C[2*8*8] chroma as 8 rows of interleaved U,V pairs, m_I[128] info;
// xConvInputFmt (src/x266.cpp:415-453) packs planar YUV 4:2:0 into tiles (chroma stride =
// luma stride / 2), xConvOutput420 (src/x266.cpp:455-492) unpacks.  m_I is never written by
// either and is left untouched here as well.  Residual formation (cur - pred on the luma of two
// tiled frames, emitted as the row-major int16 blocks the DCT32 / SATD kernels consume) has no
// upstream counterpart -- upstream stops before the residual stage (xEncodeFrame,
// src/x266.cpp:526-555) -- and is defined in include/x266hip.h.
// Reconstruction (recon = clip8(pred + residual) back into m_Y / m_C) is its mirror image, likewise defined there.
//
// Pure data movement, HBM-bound.  One thread per 16-byte luma row of a tile; the first 8 rows of
// a tile also carry its chroma row (8 U + 8 V bytes <-> 16 interleaved bytes).  A wave takes eight
// horizontally adjacent tiles x eight rows (lane = 8 * row + tile): on the planar side eight lanes
// then cover one whole 128-byte line of a picture row, on the tile side the eight rows of a tile are
// one whole line, and the residual rows of a block pair are contiguous -- every load and store
// instruction consumes whole lines, which is what lets the streaming cache hints pay.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_mfma_blocks.hpp"

namespace x266 {
namespace {

// wave -> (tile row ty, group of 8 tiles, upper / lower half of the tiles); lane -> (row, tile)
struct TileRow {
    size_t tile;      // tile index in the frame raster
    size_t ty, tx;
    int i;            // luma row inside the tile, 0..15
    bool live;        // this lane's tile exists
    bool unit_live;   // the wave's (tile row, group, half) exists: false for the whole wave at once
};

// A wave takes K consecutive units (template parameter), all of their loads issued before the first store.

__device__ __forceinline__ TileRow tile_row_of_unit(size_t unit, int lane, int tiles_x, int groups_x, size_t n_units)
{
    TileRow r;
    r.unit_live = unit < n_units;
    r.live = r.unit_live;
    const size_t u = r.live ? unit : 0;
    const int half = (int)(u & 1);
    const size_t gq = u >> 1;
    r.ty = gq / groups_x;
    r.tx = (gq - r.ty * groups_x) * 8 + (lane & 7);
    r.i = 8 * half + (lane >> 3);
    r.live = r.live && r.tx < (size_t)tiles_x;
    if (r.tx >= (size_t)tiles_x) r.tx = tiles_x - 1;
    r.tile = r.ty * tiles_x + r.tx;
    return r;
}

// PACK: planar -> tiles, else tiles -> planar
template <bool PACK, int kUnitsPerWave>
__global__ __launch_bounds__(256) void tile_convert_kernel(x266_ref_block_t *tiles, uint8_t *y, uint8_t *u, uint8_t *v,
                                                           long long strd_y, long long strd_c, int tiles_x, int groups_x,
                                                           size_t n_units)
{
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    TileRow r[kUnitsPerWave];
    v4i luma[kUnitsPerWave], cc[kUnitsPerWave];
    uint2 ua[kUnitsPerWave], ub[kUnitsPerWave];
#pragma unroll
    for (int k = 0; k < kUnitsPerWave; ++k) {
        r[k] = tile_row_of_unit(wave * kUnitsPerWave + k, lane, tiles_x, groups_x, n_units);
        luma[k] = cc[k] = v4i{0, 0, 0, 0};
        ua[k] = ub[k] = make_uint2(0, 0);
        if (!r[k].live) continue;
        const int i = r[k].i;
        uint8_t *t = reinterpret_cast<uint8_t *>(tiles + r[k].tile);
        uint8_t *py = y + (long long)(r[k].ty * 16 + i) * strd_y + r[k].tx * 16;
        luma[k] = PACK ? load16<true>(py) : load16<true>(t + i * 16);
        if (i < 8) {
            if (PACK) {
                ua[k] = *reinterpret_cast<const uint2 *>(u + (long long)(r[k].ty * 8 + i) * strd_c + r[k].tx * 8);
                ub[k] = *reinterpret_cast<const uint2 *>(v + (long long)(r[k].ty * 8 + i) * strd_c + r[k].tx * 8);
            } else {
                cc[k] = load16<true>(t + 256 + i * 16);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kUnitsPerWave; ++k) {
        if (!r[k].live) continue;
        const int i = r[k].i;
        uint8_t *t = reinterpret_cast<uint8_t *>(tiles + r[k].tile);
        uint8_t *py = y + (long long)(r[k].ty * 16 + i) * strd_y + r[k].tx * 16;
        if (PACK) store16_sc1nt(t + i * 16, luma[k]);
        else      store16_sc1nt(py, luma[k]);
        if (i < 8) {
            uint8_t *pu = u + (long long)(r[k].ty * 8 + i) * strd_c + r[k].tx * 8;
            uint8_t *pv = v + (long long)(r[k].ty * 8 + i) * strd_c + r[k].tx * 8;
            uint32_t *c = reinterpret_cast<uint32_t *>(t + 256 + i * 16);
            if (PACK) {
                const uint2 a = ua[k], b = ub[k];
                const v4i o = {(int)bperm(b.x, a.x, 0x05010400u),      // u0 v0 u1 v1
                               (int)bperm(b.x, a.x, 0x07030602u),      // u2 v2 u3 v3
                               (int)bperm(b.y, a.y, 0x05010400u), (int)bperm(b.y, a.y, 0x07030602u)};
                store16_sc1nt(c, o);
            } else {
                const uint32_t c0 = (uint32_t)cc[k][0], c1 = (uint32_t)cc[k][1], c2 = (uint32_t)cc[k][2], c3 = (uint32_t)cc[k][3];
                *reinterpret_cast<uint2 *>(pu) = make_uint2(bperm(c1, c0, 0x06040200u), bperm(c3, c2, 0x06040200u));
                *reinterpret_cast<uint2 *>(pv) = make_uint2(bperm(c1, c0, 0x07050301u), bperm(c3, c2, 0x07050301u));
            }
        }
    }
}

// residual[block][r][c] = cur - pred on tile luma; one thread per 16-pixel row segment.
// LOGB = log2(block edge): 3 (8x8, the SATD blocks) or 5 (32x32, the DCT blocks)
template <int LOGB, int kUnitsPerWave>
__global__ __launch_bounds__(256) void residual_luma_kernel(const x266_ref_block_t *__restrict__ cur,
                                                            const x266_ref_block_t *__restrict__ pred,
                                                            int16_t *__restrict__ res, int tiles_x, int groups_x, size_t n_units)
{
    constexpr int B = 1 << LOGB;
    __shared__ __attribute__((aligned(16))) unsigned char stage[B == 32 ? 4 * 2048 : 16];
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    TileRow r[kUnitsPerWave];
    v4i a[kUnitsPerWave], b[kUnitsPerWave];
#pragma unroll
    for (int k = 0; k < kUnitsPerWave; ++k) {
        r[k] = tile_row_of_unit(wave * kUnitsPerWave + k, lane, tiles_x, groups_x, n_units);
        a[k] = b[k] = v4i{0, 0, 0, 0};
        // B = 32 stores cooperatively: lanes whose tile lies beyond the frame edge (clamped to the last tile, so
        // their loads are valid) stay in the unit; their runs are skipped at the store
        if (B == 32 ? !r[k].unit_live : !r[k].live) continue;
        a[k] = load16<true>(reinterpret_cast<const uint8_t *>(cur + r[k].tile) + r[k].i * 16);
        b[k] = load16<true>(reinterpret_cast<const uint8_t *>(pred + r[k].tile) + r[k].i * 16);
    }
    const size_t width = (size_t)tiles_x * 16;
#pragma unroll
    for (int k = 0; k < kUnitsPerWave; ++k) {
        if (B == 32 ? !r[k].unit_live : !r[k].live) continue;                // B = 32: wave-uniform
        uint32_t d[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t x = (uint32_t)a[k][q], z = (uint32_t)b[k][q];
            const int d0 = (int)(x & 255) - (int)(z & 255), d1 = (int)((x >> 8) & 255) - (int)((z >> 8) & 255);
            const int d2 = (int)((x >> 16) & 255) - (int)((z >> 16) & 255), d3 = (int)(x >> 24) - (int)(z >> 24);
            d[2 * q] = ((uint32_t)d0 & 0xFFFFu) | ((uint32_t)d1 << 16);
            d[2 * q + 1] = ((uint32_t)d2 & 0xFFFFu) | ((uint32_t)d3 << 16);
        }
        const size_t py = r[k].ty * 16 + r[k].i, px = r[k].tx * 16;         // pixel coordinates of this segment
        if (B == 32) {
            // A unit's 2 KiB of residual are four 512-byte runs (8 rows x 64 bytes of four 32x32 blocks), but a
            // lane's 32 bytes are only a quarter line: written straight, every store instruction would touch half
            // of each line.  Through a wave-private 2 KiB LDS slot the wave stores its runs with two 1 KiB-linear
            // instructions instead.
            unsigned char *slot = stage + (threadIdx.x >> 6) * 2048;
            const int t = lane & 7, rr = lane >> 3;
            unsigned char *mine = slot + (t >> 1) * 512 + rr * 64 + (t & 1) * 32;
            *reinterpret_cast<v4i *>(mine) = v4i{(int)d[0], (int)d[1], (int)d[2], (int)d[3]};
            *reinterpret_cast<v4i *>(mine + 16) = v4i{(int)d[4], (int)d[5], (int)d[6], (int)d[7]};
            __builtin_amdgcn_wave_barrier();
            const size_t unit = wave * kUnitsPerWave + k;
            const size_t tx0 = (unit >> 1) % (size_t)groups_x * 8;          // first tile of the unit's group
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = lane + 64 * j, run = c >> 5;                  // 16-byte chunk of the 2 KiB, its 512-byte run
                const size_t bx = (tx0 >> 1) + run;                         // block column of that run
                if (bx * 2 < (size_t)tiles_x) {
                    const size_t blk = (py >> 5) * (width >> 5) + bx;
                    char *dst = reinterpret_cast<char *>(res + blk * 1024 + ((py & 31) & ~7) * 32) + (c & 31) * 16;
                    store16_sc1nt(dst, *reinterpret_cast<const v4i *>(slot + c * 16));
                }
            }
            __builtin_amdgcn_wave_barrier();                                // the slot is reused by the next unit
        } else {                                                           // two 8x8 blocks side by side
            const size_t blk = (py >> 3) * (width >> 3) + (px >> 3);
            int16_t *dst = res + blk * 64 + (py & 7) * 8;
            store16_sc1nt(dst, v4i{(int)d[0], (int)d[1], (int)d[2], (int)d[3]});
            store16_sc1nt(dst + 64, v4i{(int)d[4], (int)d[5], (int)d[6], (int)d[7]});
        }
    }
}


// ---- chroma residual --------------------------------------------------------------------------------------------------
// A tile's chroma is ONE 128-byte line (m_C, src/x266.cpp:60: 8 rows of 8 interleaved U,V pairs, packed at :441-449).  One lane
// takes one 16-byte row of it from both frames and emits 8 U and 8 V residuals (16 bytes each) -- the de-interleave is two
// masks and two packed 16-bit subtractions per dword.  A wave takes eight tiles x eight rows, lane = 8 * tile + row, so that a
// tile's eight lanes read its whole line:
//   LOGB = 3 (one 8x8 U and one 8x8 V block per tile): eight horizontally adjacent tiles; a tile's lanes write its two blocks'
//            128 bytes each -- with block_pitch 1 the wave's U (and V) store is 1 KiB linear;
//   LOGB = 5 (one 32x32 U and V block per 64x64 CTU = 4 x 4 tiles): 4 tiles x 2 tile rows = 16 rows of ONE block, re-ordered
//            through a wave-private LDS slot into that block's row order -- again one 1 KiB-linear store per plane.
// Both forms read whole lines and write whole lines, 1 KiB per instruction.
typedef short v2s __attribute__((ext_vector_type(2)));

template <int LOGB>
__global__ __launch_bounds__(256) void residual_chroma_kernel(const x266_ref_block_t *__restrict__ cur,
                                                              const x266_ref_block_t *__restrict__ pred,
                                                              int16_t *__restrict__ res_u, int16_t *__restrict__ res_v,
                                                              size_t block_pitch, int tiles_x, int groups_x, size_t n_units)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];  // LOGB = 5: 2 KiB per wave; the rest of the charge caps the resident waves
    const size_t unit = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (unit >= n_units) return;
    const int lane = threadIdx.x & 63;
    const size_t uy = unit / (size_t)groups_x, g = unit - uy * (size_t)groups_x;
    const int t = lane >> 3, row = lane & 7;                              // lane = 8 * tile + row: a tile's eight lanes read its whole line
    // LOGB = 3: the unit is 8 tiles of one tile row.  LOGB = 5: 4 tiles of two tile rows = a quarter-height slab of ONE block
    // (tiles_x and the tile row count are multiples of 4 there: no ragged units)
    const size_t ty = LOGB == 3 ? uy : uy * 2 + (size_t)(t >> 2);
    size_t tx = LOGB == 3 ? g * 8 + (size_t)t : g * 4 + (size_t)(t & 3);
    const bool live = tx < (size_t)tiles_x;
    if (!live) tx = (size_t)tiles_x - 1;                                 // lanes past the frame edge re-read its last tile, store nothing
    const size_t tile = ty * (size_t)tiles_x + tx;
    const v4i a = load16<true>(reinterpret_cast<const uint8_t *>(cur + tile) + 256 + row * 16);
    const v4i b = load16<true>(reinterpret_cast<const uint8_t *>(pred + tile) + 256 + row * 16);
    v4i du, dv;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t x = (uint32_t)a[q], z = (uint32_t)b[q];           // u v u v
        const uint32_t xu = x & 0x00FF00FFu, zu = z & 0x00FF00FFu, xv = (x >> 8) & 0x00FF00FFu, zv = (z >> 8) & 0x00FF00FFu;
        const v2s eu = __builtin_bit_cast(v2s, xu) - __builtin_bit_cast(v2s, zu);      // v_pk_sub_i16: two residuals at once
        const v2s ev = __builtin_bit_cast(v2s, xv) - __builtin_bit_cast(v2s, zv);
        du[q] = __builtin_bit_cast(int, eu);
        dv[q] = __builtin_bit_cast(int, ev);
    }
    if (LOGB == 5) {
        // The loads want a tile's rows in adjacent lanes, the stores a block row's four tiles: the 2 x 1 KiB change hands through a wave-private
        // LDS slot.  16-byte chunk (tile row j, row, tile) sits at j*32 + row*4 + (tile ^ ((row >> 1) & 3)): both sides conflict-free, and the
        // slab leaves as ONE 1 KiB-linear store per plane (16 block rows of 64 bytes).
        unsigned char *slot = stage + (threadIdx.x >> 6) * 2048;
        const unsigned wr = (unsigned)((t >> 2) * 32 + row * 4 + ((t & 3) ^ ((row >> 1) & 3)));
        *reinterpret_cast<v4i *>(slot + wr * 16) = du;
        *reinterpret_cast<v4i *>(slot + 1024 + wr * 16) = dv;
        __builtin_amdgcn_wave_barrier();
        const unsigned rd = (unsigned)((lane & ~3) + ((lane & 3) ^ ((lane >> 3) & 3)));
        const v4i su = *reinterpret_cast<const v4i *>(slot + rd * 16), sv = *reinterpret_cast<const v4i *>(slot + 1024 + rd * 16);
        const size_t blk = (uy >> 1) * (size_t)(tiles_x >> 2) + g;
        const size_t off = blk * block_pitch * 1024 + (uy & 1) * 512 + (size_t)lane * 8;
        store16_sc1nt(res_u + off, su);
        store16_sc1nt(res_v + off, sv);
        return;
    }
    if (!live) return;
    const size_t off = tile * block_pitch * 64 + (size_t)row * 8;         // tiles and 8x8 chroma blocks share their raster
    store16_sc1nt(res_u + off, du);
    store16_sc1nt(res_v + off, dv);
}


// ---- reconstruction: recon = clip8(pred + residual) into tiles --------------------------------------------------------
// The mirror of the two residual kernels: the same units and lane mappings with loads and stores swapped, so that every
// instruction still covers whole 128-byte lines on both sides.  Only m_Y (luma) or m_C (chroma) of the output tiles is
// written.  pred and recon are NOT __restrict__: recon == pred is allowed (an encoder reconstructs over its prediction),
// and every pred byte is read by the lane that later writes it.
template <int LOGB>
__global__ __launch_bounds__(256) void recon_luma_kernel(const x266_ref_block_t *pred, const int16_t *__restrict__ res,
                                                         x266_ref_block_t *recon, int tiles_x, int groups_x, size_t n_units)
{
    constexpr int B = 1 << LOGB;
    __shared__ __attribute__((aligned(16))) unsigned char stage[B == 32 ? 4 * 2048 : 16];
    const size_t unit = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const TileRow r = tile_row_of_unit(unit, lane, tiles_x, groups_x, n_units);
    if (!r.unit_live) return;                                               // wave-uniform
    const size_t width = (size_t)tiles_x * 16;
    const size_t py = r.ty * 16 + r.i, px = r.tx * 16;                      // pixel coordinates of this lane's segment
    // pred first, so that it is in flight with the residual (lanes past the frame edge read the clamped last tile: valid,
    // read in the same instruction as its own lane's read, and they store nothing)
    const v4i p = load16<true>(reinterpret_cast<const uint8_t *>(pred + r.tile) + r.i * 16);
    v4i d0, d1;                                                             // its 16 residuals
    if (B == 32) {
        // the unit's 2 KiB of residual (four 512-byte runs of 8 rows x 64 bytes) arrive with two 1 KiB-linear loads and are
        // re-ordered through the wave's LDS slot into the lanes' 32-byte row segments (residual_luma_kernel backwards)
        unsigned char *slot = stage + (threadIdx.x >> 6) * 2048;
        const size_t tx0 = (unit >> 1) % (size_t)groups_x * 8;
        v4i g[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {                                       // both loads in flight before the first wait
            const int c = lane + 64 * j, run = c >> 5;
            size_t bx = (tx0 >> 1) + run;
            if (bx * 2 >= (size_t)tiles_x) bx = tx0 >> 1;                   // a run beyond the frame edge re-reads the group's first: no lane uses it
            const size_t blk = (py >> 5) * (width >> 5) + bx;
            g[j] = load16<true>(reinterpret_cast<const char *>(res + blk * 1024 + ((py & 31) & ~7) * 32) + (c & 31) * 16);
        }
        *reinterpret_cast<v4i *>(slot + lane * 16) = g[0];
        *reinterpret_cast<v4i *>(slot + 1024 + lane * 16) = g[1];
        __builtin_amdgcn_wave_barrier();
        const int t = lane & 7, rr = lane >> 3;
        const unsigned char *mine = slot + (t >> 1) * 512 + rr * 64 + (t & 1) * 32;
        d0 = *reinterpret_cast<const v4i *>(mine);
        d1 = *reinterpret_cast<const v4i *>(mine + 16);
        if (!r.live) return;
    } else {                                                                // two 8x8 blocks side by side
        if (!r.live) return;
        const size_t blk = (py >> 3) * (width >> 3) + (px >> 3);
        const int16_t *src = res + blk * 64 + (py & 7) * 8;
        d0 = load16<true>(src);
        d1 = load16<true>(src + 64);
    }
    store16_sc1nt(reinterpret_cast<uint8_t *>(recon + r.tile) + r.i * 16, recon_luma16(p, d0, d1));
}

// chroma: residual_chroma_kernel backwards.  LOGB = 3: a tile's 8x8 U and V rows straight from the block streams;
// LOGB = 5: the unit's quarter-height slab of one 32x32 block arrives as ONE 1 KiB-linear load per plane and changes hands
// through the wave's LDS slot (the same swizzled positions as the residual kernel, read and written the other way round).
template <int LOGB>
__global__ __launch_bounds__(256) void recon_chroma_kernel(const x266_ref_block_t *pred, const int16_t *__restrict__ res_u,
                                                           const int16_t *__restrict__ res_v, size_t block_pitch,
                                                           x266_ref_block_t *recon, int tiles_x, int groups_x, size_t n_units)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];
    const size_t unit = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (unit >= n_units) return;
    const int lane = threadIdx.x & 63;
    const size_t uy = unit / (size_t)groups_x, g = unit - uy * (size_t)groups_x;
    const int t = lane >> 3, row = lane & 7;
    const size_t ty = LOGB == 3 ? uy : uy * 2 + (size_t)(t >> 2);
    const size_t tx = LOGB == 3 ? g * 8 + (size_t)t : g * 4 + (size_t)(t & 3);
    if (LOGB == 3 && tx >= (size_t)tiles_x) return;                         // LOGB = 5 has no ragged units
    const size_t tile = ty * (size_t)tiles_x + tx;
    const v4i p = load16<true>(reinterpret_cast<const uint8_t *>(pred + tile) + 256 + row * 16);   // in flight with the residual
    v4i du, dv;
    if (LOGB == 5) {
        unsigned char *slot = stage + (threadIdx.x >> 6) * 2048;
        const size_t blk = (uy >> 1) * (size_t)(tiles_x >> 2) + g;
        const size_t off = blk * block_pitch * 1024 + (uy & 1) * 512 + (size_t)lane * 8;
        const v4i su = load16<true>(res_u + off), sv = load16<true>(res_v + off);
        const unsigned rd = (unsigned)((lane & ~3) + ((lane & 3) ^ ((lane >> 3) & 3)));
        *reinterpret_cast<v4i *>(slot + rd * 16) = su;
        *reinterpret_cast<v4i *>(slot + 1024 + rd * 16) = sv;
        __builtin_amdgcn_wave_barrier();
        const unsigned wr = (unsigned)((t >> 2) * 32 + row * 4 + ((t & 3) ^ ((row >> 1) & 3)));
        du = *reinterpret_cast<const v4i *>(slot + wr * 16);
        dv = *reinterpret_cast<const v4i *>(slot + 1024 + wr * 16);
    } else {
        const size_t off = tile * block_pitch * 64 + (size_t)row * 8;       // tiles and 8x8 chroma blocks share their raster
        du = load16<true>(res_u + off);
        dv = load16<true>(res_v + off);
    }
    store16_sc1nt(reinterpret_cast<uint8_t *>(recon + tile) + 256 + row * 16, recon_chroma16(p, du, dv));
}

// Integer-pel luma motion compensation: pred[8by + y][8bx + x] = ref[clamp(8by + y + mvy, 0, H - 1)][clamp(8bx + x + mvx, 0, W - 1)]
// with (mvx, mvy) the x266_me_result_t record of 8x8 block (bx, by) (raster order of blocks, the searches' d_best layout).
// One lane per 16-byte row of an output tile -- the rows of the tile's left and right 8x8 blocks -- so sixteen lanes write a
// tile's m_Y and a wave four whole tiles (1 KiB of full lines).  The reads are a gather: a source row of 8 samples inside the
// frame is three aligned dwords (each within one 16-byte tile row, possibly of two tiles) and two funnel shifts; rows that
// reach past the left or right edge are read sample by sample.
// Row i (0..15) of m_Y of tile (tx, ty): shared by the luma kernel and the fused one.
__device__ __forceinline__ void mc_luma_row(const x266_ref_block_t *__restrict__ ref, const x266_me_result_t *__restrict__ mv,
                                            x266_ref_block_t *__restrict__ pred, int width, int height, int tiles_x, size_t tile, int i)
{
    const size_t ty = tile / (size_t)tiles_x, tx = tile - ty * (size_t)tiles_x;
    const x266_me_result_t *m = mv + (ty * 2 + (size_t)(i >> 3)) * (size_t)(2 * tiles_x) + tx * 2;
    const uint8_t *src = reinterpret_cast<const uint8_t *>(ref);
    uint32_t out[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const x266_me_result_t r = m[h];
        int sy = (int)(ty * 16) + i + r.mvy;
        sy = sy < 0 ? 0 : (sy > height - 1 ? height - 1 : sy);
        const uint8_t *row = src + (size_t)(sy >> 4) * (size_t)tiles_x * 512 + (sy & 15) * 16;
        const int sx = (int)(tx * 16) + 8 * h + r.mvx;
        if (sx >= 0 && sx + 7 <= width - 1) {
            const int xa = sx & ~3, xc = xa + 8 < width ? xa + 8 : xa + 4;     // the third dword is unused when sx is aligned
            const uint32_t d0 = *reinterpret_cast<const uint32_t *>(row + (size_t)(xa >> 4) * 512 + (xa & 15));
            const uint32_t d1 = *reinterpret_cast<const uint32_t *>(row + (size_t)((xa + 4) >> 4) * 512 + ((xa + 4) & 15));
            const uint32_t d2 = *reinterpret_cast<const uint32_t *>(row + (size_t)(xc >> 4) * 512 + (xc & 15));
            const int sh = (sx & 3) * 8;
            out[2 * h] = __builtin_amdgcn_alignbit(d1, d0, sh);
            out[2 * h + 1] = __builtin_amdgcn_alignbit(d2, d1, sh);
        } else {
            out[2 * h] = out[2 * h + 1] = 0;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                int x = sx + b;
                x = x < 0 ? 0 : (x > width - 1 ? width - 1 : x);
                out[2 * h + (b >> 2)] |= (uint32_t)row[(size_t)(x >> 4) * 512 + (x & 15)] << (8 * (b & 3));
            }
        }
    }
    store16_sc1nt(reinterpret_cast<uint8_t *>(pred + tile) + i * 16, v4i{(int)out[0], (int)out[1], (int)out[2], (int)out[3]});
}

__global__ __launch_bounds__(256) void motion_comp_luma_kernel(const x266_ref_block_t *__restrict__ ref, const x266_me_result_t *__restrict__ mv,
                                                               x266_ref_block_t *__restrict__ pred, int width, int height, int tiles_x,
                                                               size_t n_rows)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_rows) return;
    mc_luma_row(ref, mv, pred, width, height, tiles_x, g >> 4, (int)(g & 15));
}

// 4:2:0 chroma motion compensation (the convention of include/x266hip.h): the luma vector of 8x8 block (bx, by) moves the 4x4
// block (bx, by) of U and of V by (mv >> 1) whole samples, and an odd component adds the half-sample filter (-4, 36, 36, -4)
// along that axis.  U and V of a pair share position and taps, so a pair is filtered as one packed 2 x int16 value: the
// horizontal stage (-2040..18360) and the 1-D results fit int16, only the vertical stage of the 2-D case is widened to 32 bits.
typedef short v2s __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2s mc_half_taps(v2s a, v2s b, v2s c, v2s d)     // -4 a + 36 b + 36 c - 4 d
{
    return (b + c) * (short)36 - (a + d) * (short)4;
}

__device__ __forceinline__ v2s mc_round_clip8(v2s s)                         // clip8((s + 32) >> 6) on both halves
{
    const v2s lo = {0, 0}, hi = {255, 255};
    return __builtin_elementwise_min(__builtin_elementwise_max((s + (short)32) >> (short)6, lo), hi);
}

// The four (U, V) pairs from chroma x = cx of one clamped chroma row (`row` points at the row's bytes in tile column 0), each
// as a packed int16 pair: the samples themselves (fx = 0) or the unshifted horizontal filter sums (fx = 1, pairs cx - 1 .. cx + 5
// are read).  In-frame spans are aligned dwords (two pairs each, within one 16-byte m_C row) and funnel shifts; spans that cross
// the left or right edge are read pair by pair with clamped x.
__device__ __forceinline__ void mc_chroma_row4(const uint8_t *row, int cx, int fx, int cw, v2s out[4])
{
    const int xs = cx - fx, n = 4 + 3 * fx;
    uint32_t w[4];
    if (xs >= 0 && xs + n - 1 <= cw - 1) {
        const int xa = xs & ~1;
        uint32_t d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = xa + 2 * k < cw - 2 ? xa + 2 * k : cw - 2;        // a clamped dword holds no pair that is used
            d[k] = (k < 3 || fx) ? *reinterpret_cast<const uint32_t *>(row + (size_t)(x >> 3) * 512 + (x & 7) * 2) : 0u;
        }
        const int sh = (xs & 1) * 16;
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = __builtin_amdgcn_alignbit(d[k + 1], d[k], sh);
        w[3] = d[3] >> sh;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = 0;
#pragma unroll
        for (int b = 0; b < 7; ++b) {
            int x = xs + b;
            x = x < 0 ? 0 : (x > cw - 1 ? cw - 1 : x);
            if (b < 4 || fx) w[b >> 1] |= (uint32_t)*reinterpret_cast<const uint16_t *>(row + (size_t)(x >> 3) * 512 + (x & 7) * 2) << (16 * (b & 1));
        }
    }
    v2s q[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        q[2 * k] = __builtin_bit_cast(v2s, bperm(0u, w[k], 0x0c010c00u));      // u | v << 16 (sel 0x0c = zero byte)
        q[2 * k + 1] = __builtin_bit_cast(v2s, bperm(0u, w[k], 0x0c030c02u));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = fx ? mc_half_taps(q[k], q[k + 1], q[k + 2], q[k + 3]) : q[k];
}

// Half h (0 left, 1 right) of row j (0..7) of m_C of tile (tx, ty): row j & 3 of the 4x4 (U, V) blocks of one 8x8 luma block,
// 8 bytes.  One lane per half, not per 16-byte row: a lane of the 2-D class gathers four source rows, and at the size of a
// frame the call is bound by that chain of loads, not by bytes -- twice the lanes with half the chain each.
__device__ __forceinline__ void mc_chroma_half(const x266_ref_block_t *__restrict__ ref, const x266_me_result_t *__restrict__ mv,
                                               x266_ref_block_t *__restrict__ pred, int width, int height, int tiles_x, size_t tile, int j, int h)
{
    const size_t ty = tile / (size_t)tiles_x, tx = tile - ty * (size_t)tiles_x;
    const x266_me_result_t r = mv[(ty * 2 + (size_t)(j >> 2)) * (size_t)(2 * tiles_x) + tx * 2 + (size_t)h];
    const uint8_t *src = reinterpret_cast<const uint8_t *>(ref) + 256;
    const int cw = width >> 1, ch = height >> 1;
    const int fx = r.mvx & 1, fy = r.mvy & 1;
    const int cx = (int)(tx * 8) + 4 * h + (r.mvx >> 1), cy = (int)(ty * 8) + j + (r.mvy >> 1);
    v2s o[4];
    if (!fy) {
        const int sy = cy < 0 ? 0 : (cy > ch - 1 ? ch - 1 : cy);
        mc_chroma_row4(src + (size_t)(sy >> 3) * (size_t)tiles_x * 512 + (sy & 7) * 16, cx, fx, cw, o);
        if (fx) {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = mc_round_clip8(o[k]);
        }
    } else {
        v2s t[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            int sy = cy + a - 1;
            sy = sy < 0 ? 0 : (sy > ch - 1 ? ch - 1 : sy);
            mc_chroma_row4(src + (size_t)(sy >> 3) * (size_t)tiles_x * 512 + (sy & 7) * 16, cx, fx, cw, t[a]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!fx) {
                o[k] = mc_round_clip8(mc_half_taps(t[0][k], t[1][k], t[2][k], t[3][k]));
            } else {                                                        // the sum of sums needs 32 bits; >> floors
                int c[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int v = (36 * ((int)t[1][k][e] + (int)t[2][k][e]) - 4 * ((int)t[0][k][e] + (int)t[3][k][e])) >> 6;
                    const int s = (v + 32) >> 6;
                    c[e] = s < 0 ? 0 : (s > 255 ? 255 : s);
                }
                o[k] = v2s{(short)c[0], (short)c[1]};
            }
        }
    }
    const uint2 out = make_uint2(bperm(__builtin_bit_cast(uint32_t, o[1]), __builtin_bit_cast(uint32_t, o[0]), 0x06040200u),      // u0 v0 u1 v1
                                 bperm(__builtin_bit_cast(uint32_t, o[3]), __builtin_bit_cast(uint32_t, o[2]), 0x06040200u));
    __builtin_nontemporal_store(out.x | ((unsigned long long)out.y << 32),
                                reinterpret_cast<unsigned long long *>(reinterpret_cast<uint8_t *>(pred + tile) + 256 + j * 16 + h * 8));
}

// one lane per 8-byte half of an m_C row: sixteen lanes write a tile's 128 chroma bytes, a wave the whole lines of four tiles
__global__ __launch_bounds__(256) void motion_comp_chroma_kernel(const x266_ref_block_t *__restrict__ ref, const x266_me_result_t *__restrict__ mv,
                                                                 x266_ref_block_t *__restrict__ pred, int width, int height, int tiles_x,
                                                                 size_t n_halves)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_halves) return;
    mc_chroma_half(ref, mv, pred, width, height, tiles_x, g >> 4, (int)(g >> 1) & 7, (int)(g & 1));
}

// m_Y and m_C in one launch, the role fixed per WAVE: a workgroup of four waves takes eight tiles, waves 0 and 1 their 128 luma
// rows, waves 2 and 3 their 128 chroma halves -- no wave runs both code paths, every store instruction still covers whole
// lines, and the chroma waves' longer gather overlaps the luma waves' (profiles/r10_mc_chroma.txt: under the two calls back to back).
__global__ __launch_bounds__(256) void motion_comp_kernel(const x266_ref_block_t *__restrict__ ref, const x266_me_result_t *__restrict__ mv,
                                                          x266_ref_block_t *__restrict__ pred, int width, int height, int tiles_x,
                                                          size_t n_tiles)
{
    const int t = threadIdx.x & 127;
    const size_t tile = (size_t)blockIdx.x * 8 + (size_t)(t >> 4);
    if (tile >= n_tiles) return;
    if (threadIdx.x < 128) mc_luma_row(ref, mv, pred, width, height, tiles_x, tile, t & 15);
    else                   mc_chroma_half(ref, mv, pred, width, height, tiles_x, tile, (t >> 1) & 7, t & 1);
}

}  // namespace

// Units per wave, measured (tools/probes/gpu_tilefmt_probe.py, 32768^2 frame): unpacking gains 13 % from two units per wave (its planar
// stores are half lines per instruction; more of them in flight per wave), packing and the residual kernels lose 3-10 %.
constexpr int kUnitsPack = 1, kUnitsUnpack = 2, kUnitsResidual = 1;

hipError_t launch_tile_convert(bool pack, x266_ref_block_t *d_tiles, uint8_t *d_y, uint8_t *d_u, uint8_t *d_v,
                               long long strd_y, long long strd_c, int width, int height, hipStream_t stream)
{
    const int tiles_x = width / 16, groups_x = (tiles_x + 7) / 8;
    const size_t n_units = (size_t)groups_x * (height / 16) * 2;           // unit = (tile row, 8 tiles, half)
    if (n_units == 0) return hipSuccess;
    const size_t K = pack ? kUnitsPack : kUnitsUnpack;
    const size_t n_waves = (n_units + K - 1) / K;
    if ((n_waves + 3) / 4 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    dim3 grid((unsigned)((n_waves + 3) / 4)), block(256);
    if (pack) hipLaunchKernelGGL((tile_convert_kernel<true, kUnitsPack>), grid, block, 0, stream, d_tiles, d_y, d_u, d_v, strd_y, strd_c, tiles_x, groups_x, n_units);
    else      hipLaunchKernelGGL((tile_convert_kernel<false, kUnitsUnpack>), grid, block, 0, stream, d_tiles, d_y, d_u, d_v, strd_y, strd_c, tiles_x, groups_x, n_units);
    return hipGetLastError();
}

hipError_t launch_residual_luma(int block_edge, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int16_t *d_res,
                                int width, int height, hipStream_t stream)
{
    const int tiles_x = width / 16, groups_x = (tiles_x + 7) / 8;
    const size_t n_units = (size_t)groups_x * (height / 16) * 2;
    if (n_units == 0) return hipSuccess;
    const size_t n_waves = (n_units + kUnitsResidual - 1) / kUnitsResidual;
    // two-wave workgroups, 20 KiB of LDS charged per workgroup = 16 resident waves per CU: paired in one process against round 4's shape (four-wave
    // workgroups, no cap) 0.662 against 0.707 ms for the 32x32 order of a 32768^2 frame, 0.658 against 0.709 for the 8x8 order (-6.5 / -7 %:
    // 0.81 of 8 TB/s, 0.97-0.98 of the box's copy stream; tools/probes/gpu_residual_shapes.py, profiles/r05_from_tiles_dma.txt)
    constexpr unsigned kThreads = 128, kLdsPerWorkgroup = 20480;
    const size_t wgs = (n_waves + 1) / 2;
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    dim3 grid((unsigned)wgs), block(kThreads);
    if (block_edge == 32) hipLaunchKernelGGL((residual_luma_kernel<5, kUnitsResidual>), grid, block, kLdsPerWorkgroup - 4 * 2048, stream, d_cur, d_pred, d_res, tiles_x, groups_x, n_units);
    else                  hipLaunchKernelGGL((residual_luma_kernel<3, kUnitsResidual>), grid, block, kLdsPerWorkgroup, stream, d_cur, d_pred, d_res, tiles_x, groups_x, n_units);
    return hipGetLastError();
}

hipError_t launch_residual_chroma(int block_edge, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int16_t *d_res_u, int16_t *d_res_v,
                                  size_t block_pitch, int width, int height, hipStream_t stream)
{
    const int tiles_x = width / 16, tiles_y = height / 16;
    const int groups_x = block_edge == 32 ? tiles_x / 4 : (tiles_x + 7) / 8;
    const size_t n_units = (size_t)groups_x * (size_t)(block_edge == 32 ? tiles_y / 2 : tiles_y);     // one wave each: 8 tiles' chroma lines
    if (n_units == 0) return hipSuccess;
    // one-wave workgroups, 12 KiB of LDS charged = 13 resident waves per CU: paired in one process on a 32768^2 frame (tools/probes/gpu_chroma_shapes.py,
    // profiles/r06_chroma_shapes.txt) the 8x8 order runs at 0.977 of the box's copy of the same bytes (two-wave workgroups with 20 KiB, the luma shape: 0.96)
    constexpr unsigned kThreads = 64, kLdsPerWorkgroup = 12288;
    if (n_units > 0x7FFFFFFFull) return hipErrorInvalidValue;
    dim3 grid((unsigned)n_units), block(kThreads);
    if (block_edge == 32) hipLaunchKernelGGL(residual_chroma_kernel<5>, grid, block, kLdsPerWorkgroup, stream, d_cur, d_pred, d_res_u, d_res_v, block_pitch, tiles_x, groups_x, n_units);
    else                  hipLaunchKernelGGL(residual_chroma_kernel<3>, grid, block, kLdsPerWorkgroup, stream, d_cur, d_pred, d_res_u, d_res_v, block_pitch, tiles_x, groups_x, n_units);
    return hipGetLastError();
}

// the launch shapes of the residual kernels they mirror
hipError_t launch_recon_luma(int block_edge, const x266_ref_block_t *d_pred, const int16_t *d_res, x266_ref_block_t *d_recon,
                             int width, int height, hipStream_t stream)
{
    const int tiles_x = width / 16, groups_x = (tiles_x + 7) / 8;
    const size_t n_units = (size_t)groups_x * (height / 16) * 2;
    if (n_units == 0) return hipSuccess;
    constexpr unsigned kThreads = 128, kLdsPerWorkgroup = 20480;
    const size_t wgs = (n_units + 1) / 2;
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    dim3 grid((unsigned)wgs), block(kThreads);
    if (block_edge == 32) hipLaunchKernelGGL(recon_luma_kernel<5>, grid, block, kLdsPerWorkgroup - 4 * 2048, stream, d_pred, d_res, d_recon, tiles_x, groups_x, n_units);
    else                  hipLaunchKernelGGL(recon_luma_kernel<3>, grid, block, kLdsPerWorkgroup, stream, d_pred, d_res, d_recon, tiles_x, groups_x, n_units);
    return hipGetLastError();
}

hipError_t launch_recon_chroma(int block_edge, const x266_ref_block_t *d_pred, const int16_t *d_res_u, const int16_t *d_res_v, size_t block_pitch,
                               x266_ref_block_t *d_recon, int width, int height, hipStream_t stream)
{
    const int tiles_x = width / 16, tiles_y = height / 16;
    const int groups_x = block_edge == 32 ? tiles_x / 4 : (tiles_x + 7) / 8;
    const size_t n_units = (size_t)groups_x * (size_t)(block_edge == 32 ? tiles_y / 2 : tiles_y);
    if (n_units == 0) return hipSuccess;
    constexpr unsigned kThreads = 64, kLdsPerWorkgroup = 12288;
    if (n_units > 0x7FFFFFFFull) return hipErrorInvalidValue;
    dim3 grid((unsigned)n_units), block(kThreads);
    if (block_edge == 32) hipLaunchKernelGGL(recon_chroma_kernel<5>, grid, block, kLdsPerWorkgroup, stream, d_pred, d_res_u, d_res_v, block_pitch, d_recon, tiles_x, groups_x, n_units);
    else                  hipLaunchKernelGGL(recon_chroma_kernel<3>, grid, block, kLdsPerWorkgroup, stream, d_pred, d_res_u, d_res_v, block_pitch, d_recon, tiles_x, groups_x, n_units);
    return hipGetLastError();
}

hipError_t launch_motion_comp_luma(const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, x266_ref_block_t *d_pred,
                                   int width, int height, hipStream_t stream)
{
    const int tiles_x = width / 16;
    const size_t n_rows = (size_t)tiles_x * (size_t)(height / 16) * 16;     // one lane per 16-byte output row
    if (n_rows == 0) return hipSuccess;
    const size_t wgs = (n_rows + 255) / 256;
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(motion_comp_luma_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, d_ref, d_mv, d_pred, width, height, tiles_x, n_rows);
    return hipGetLastError();
}

hipError_t launch_motion_comp_chroma(const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, x266_ref_block_t *d_pred,
                                     int width, int height, hipStream_t stream)
{
    const int tiles_x = width / 16;
    const size_t n_halves = (size_t)tiles_x * (size_t)(height / 16) * 16;   // one lane per 8-byte half of an m_C row
    if (n_halves == 0) return hipSuccess;
    const size_t wgs = (n_halves + 255) / 256;
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(motion_comp_chroma_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, d_ref, d_mv, d_pred, width, height, tiles_x, n_halves);
    return hipGetLastError();
}

hipError_t launch_motion_comp(const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, x266_ref_block_t *d_pred,
                              int width, int height, hipStream_t stream)
{
    const int tiles_x = width / 16;
    const size_t n_tiles = (size_t)tiles_x * (size_t)(height / 16);
    if (n_tiles == 0) return hipSuccess;
    const size_t wgs = (n_tiles + 7) / 8;                                    // eight tiles per four-wave workgroup
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(motion_comp_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, d_ref, d_mv, d_pred, width, height, tiles_x, n_tiles);
    return hipGetLastError();
}

}  // namespace x266
