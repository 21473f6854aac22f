// deblock_kernels.hip -- in-loop deblocking of tiled frames (xDeblockLumaGpu / ChromaGpu / Gpu of include/x266hip.h).  The filter
// itself -- tables, boundary strength, parameters, the per-line arithmetic -- is x266_deblock.hpp's, one copy for the three kernels
// and both edge directions.
//
// The unit of work is a CTU-sized square moved by (-4, -4) samples and clipped at the frame: luma [64cx-4, 64cx+60) x [64cy-4, 64cy+60),
// chroma the same with 32 (in chroma samples, i.e. 64 interleaved bytes x 32 rows).  Such a unit is a union of the 8x8 areas centred
// on the grid crossings, which partition the plane and inside which the two-pass result depends on the area's own input only (the
// header derives this).  So a unit reads exactly the samples it writes, needs no halo, does not care in which order units run, and
// d_out == d_in is safe; the plane crosses HBM once in each direction.  There are ceil((W + 4) / 64) x ceil((H + 4) / 64) units for
// both planes; the last column and row of units are 4 (or 4 + 16k) samples wide.
//
// Inside a unit every edge line is aligned: a luma line p3..q3 of a vertical edge is the 8 bytes 8j..8j+7 of an LDS row, the four
// lines of a segment are four consecutive lanes (a DPP quad exchanges the terms of lines 0 and 3), and the same holds transposed
// for horizontal edges.  Phases, separated by workgroup barriers that every wave of every kernel passes the same number of times:
//   A  load the unit as dwords into LDS rows; the first threads derive the parameters of the unit's 8-sample edges into LDS
//   B  vertical edges: one lane per line, 8 bytes (chroma: p1 p0 q0 q1 of both planes) read and written back
//   C  horizontal edges: one lane per column, bytes read down the rows
//   D  store the unit's dwords
// The side arrays are read with per-lane byte loads, not on the scalar path: a moved unit touches up to four CTUs and nine luma
// regions, so no region byte is uniform over a wave.  Instead each 8-sample edge's parameters are derived ONCE, by one lane, and
// the filter passes read them back as LDS broadcasts.
// Luma is 256 lanes per unit, chroma one wave per unit; the fused kernel gives a unit's luma to waves 0..3 and its chroma to wave 4,
// the role fixed per wave as in mc_qpel_kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_deblock.hpp"
#include "x266_device.hpp"

namespace x266 {
namespace {

constexpr int kRowBytes = 72;               // LDS row pitch: 64 bytes of samples, padded so that a column of 8-byte reads spreads over the banks

struct LumaSlab {
    uint32_t rows[64 * kRowBytes / 4];
    uint32_t edge[2][8][9];                 // [direction][edge inside the unit][block across it]: deblock_luma_edge
};
struct ChromaSlab {
    uint32_t rows[32 * kRowBytes / 4];
    uint32_t edge[2][4][5];                 // deblock_chroma_edge
};

__device__ __forceinline__ int quad_lane(int x, int ctrl_lane)          // the value of lane `ctrl_lane` (0 or 3) of the caller's quad
{
    return ctrl_lane ? __builtin_amdgcn_mov_dpp(x, 0xFF, 0xF, 0xF, true) : __builtin_amdgcn_mov_dpp(x, 0x00, 0xF, 0xF, true);
}

// ---- luma: t = 0..255 ----------------------------------------------------------------------------------------------------------
// dword i of the unit: row i >> 4, bytes 4 (i & 15) ..; its address in a frame, or nullptr outside the frame
__device__ __forceinline__ size_t luma_dword_offset(const DeblockSide &s, int ux, int uy, int i, bool &inside)
{
    const int x = 64 * ux - 4 + 4 * (i & 15), y = 64 * uy - 4 + (i >> 4);
    inside = x >= 0 && x < s.width && y >= 0 && y < s.height;
    return ((size_t)(y >> 4) * (size_t)s.tiles_x + (size_t)(x >> 4)) * 512 + (size_t)((y & 15) * 16 + (x & 15));
}

__device__ __forceinline__ void luma_load(const DeblockSide &s, const uint8_t *in, LumaSlab &m, int ux, int uy, int t)
{
    uint32_t d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bool inside;
        const size_t off = luma_dword_offset(s, ux, uy, t + 256 * k, inside);
        d[k] = inside ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(in + off)) : 0u;
    }
    if (t < 144) {
        const int dir = t >= 72, e = dir ? t - 72 : t, j = e / 9, b = e - 9 * j;
        // vertical: edge at x = 64 ux + 8 j between block columns, block row 8 uy - 1 + b; horizontal: the transpose
        const int coord = 64 * (dir ? uy : ux) + 8 * j, along = 8 * (dir ? ux : uy) - 1 + b;
        const int limit = dir ? s.height : s.width, blocks_along = (dir ? s.width : s.height) >> 3;
        uint32_t packed = 0;
        if (coord > 0 && coord < limit && along >= 0 && along < blocks_along) {
            const int c = coord >> 3;
            packed = dir ? deblock_luma_edge(s, along, c - 1, along, c, coord) : deblock_luma_edge(s, c - 1, along, c, along, coord);
        }
        m.edge[dir][j][b] = packed;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = t + 256 * k;
        m.rows[(i >> 4) * (kRowBytes / 4) + (i & 15)] = d[k];
    }
}

__device__ __forceinline__ void luma_store(const DeblockSide &s, uint8_t *out, const LumaSlab &m, int ux, int uy, int t)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = t + 256 * k;
        bool inside;
        const size_t off = luma_dword_offset(s, ux, uy, i, inside);
        if (inside) __builtin_nontemporal_store(m.rows[(i >> 4) * (kRowBytes / 4) + (i & 15)], reinterpret_cast<uint32_t *>(out + off));
    }
}

// vertical edges: lane = row t & 63 of edge (t >> 6) and of edge (t >> 6) + 4.  Rows and edges outside the frame have parameters 0.
__device__ __forceinline__ void luma_vertical(LumaSlab &m, int t)
{
    const int r = t & 63;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = (t >> 6) + 4 * k;
        const uint32_t packed = m.edge[0][j][(r + 4) >> 3];
        const int tc = (int)((packed >> 2) & 63u), beta = (int)(packed >> 8);
        uint32_t *word = &m.rows[r * (kRowBytes / 4) + 2 * j];
        const uint32_t lo = word[0], hi = word[1];
        int v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = (int)((lo >> (8 * e)) & 255u);
            v[4 + e] = (int)((hi >> (8 * e)) & 255u);
        }
        const int terms = (int)deblock_line_terms(v, beta, tc);
        const uint32_t t0 = (uint32_t)quad_lane(terms, 0), t3 = (uint32_t)quad_lane(terms, 3);
        if ((packed & 3u) && deblock_luma_line(v, t0, t3, beta, tc)) {
            word[0] = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
            word[1] = (uint32_t)v[4] | (uint32_t)v[5] << 8 | (uint32_t)v[6] << 16 | (uint32_t)v[7] << 24;
        }
    }
}

// horizontal edges: lane = column t & 63 of edge (t >> 6) and of edge (t >> 6) + 4, the line read down rows 8 j .. 8 j + 7
__device__ __forceinline__ void luma_horizontal(LumaSlab &m, int t)
{
    const int c = t & 63;
    uint8_t *bytes = reinterpret_cast<uint8_t *>(m.rows);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = (t >> 6) + 4 * k;
        const uint32_t packed = m.edge[1][j][(c + 4) >> 3];
        const int tc = (int)((packed >> 2) & 63u), beta = (int)(packed >> 8);
        uint8_t *col = bytes + 8 * j * kRowBytes + c;
        int v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = col[e * kRowBytes];
        const int terms = (int)deblock_line_terms(v, beta, tc);
        const uint32_t t0 = (uint32_t)quad_lane(terms, 0), t3 = (uint32_t)quad_lane(terms, 3);
        if ((packed & 3u) && deblock_luma_line(v, t0, t3, beta, tc)) {
#pragma unroll
            for (int e = 1; e < 7; ++e) col[e * kRowBytes] = (uint8_t)v[e];
        }
    }
}

// ---- chroma: one wave, l = 0..63 -------------------------------------------------------------------------------------------------
// dword i of the unit: row i >> 4, (U, V) pairs 2 (i & 15) and the next
__device__ __forceinline__ size_t chroma_dword_offset(const DeblockSide &s, int ux, int uy, int i, bool &inside)
{
    const int x = 32 * ux - 4 + 2 * (i & 15), y = 32 * uy - 4 + (i >> 4);
    inside = x >= 0 && x < (s.width >> 1) && y >= 0 && y < (s.height >> 1);
    return ((size_t)(y >> 3) * (size_t)s.tiles_x + (size_t)(x >> 3)) * 512 + (size_t)(256 + (y & 7) * 16 + (x & 7) * 2);
}

__device__ __forceinline__ void chroma_load(const DeblockSide &s, const uint8_t *in, ChromaSlab &m, int ux, int uy, int l)
{
    uint32_t d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        bool inside;
        const size_t off = chroma_dword_offset(s, ux, uy, l + 64 * k, inside);
        d[k] = inside ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(in + off)) : 0u;
    }
    if (l < 40) {
        const int dir = l >= 20, e = dir ? l - 20 : l, j = e / 5, b = e - 5 * j;
        const int coord = 32 * (dir ? uy : ux) + 8 * j, along = 4 * (dir ? ux : uy) - 1 + b;
        const int limit = (dir ? s.height : s.width) >> 1, tiles_along = (dir ? s.width : s.height) >> 4;
        uint32_t packed = 0;
        if (coord > 0 && coord < limit && along >= 0 && along < tiles_along) {
            const int c = coord >> 3;
            packed = dir ? deblock_chroma_edge(s, along, c - 1, along, c, coord) : deblock_chroma_edge(s, c - 1, along, c, along, coord);
        }
        m.edge[dir][j][b] = packed;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = l + 64 * k;
        m.rows[(i >> 4) * (kRowBytes / 4) + (i & 15)] = d[k];
    }
}

__device__ __forceinline__ void chroma_store(const DeblockSide &s, uint8_t *out, const ChromaSlab &m, int ux, int uy, int l)
{
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = l + 64 * k;
        bool inside;
        const size_t off = chroma_dword_offset(s, ux, uy, i, inside);
        if (inside) __builtin_nontemporal_store(m.rows[(i >> 4) * (kRowBytes / 4) + (i & 15)], reinterpret_cast<uint32_t *>(out + off));
    }
}

// vertical edges: lane = row l & 31 of edges (l >> 5) and (l >> 5) + 2; p1 p0 | q0 q1 of both planes are bytes 16 j + 4 .. 16 j + 11
__device__ __forceinline__ void chroma_vertical(ChromaSlab &m, int l)
{
    const int r = l & 31;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = (l >> 5) + 2 * k;
        const uint32_t packed = m.edge[0][j][(r + 4) >> 3];
        if (!packed) continue;
        uint32_t *word = &m.rows[r * (kRowBytes / 4) + 4 * j + 1];
        const uint32_t lo = word[0], hi = word[1];                        // U p1, V p1, U p0, V p0 | U q0, V q0, U q1, V q1
        uint32_t out_lo = lo & 0x0000FFFFu, out_hi = hi & 0xFFFF0000u;
#pragma unroll
        for (int plane = 0; plane < 2; ++plane) {
            const int sh = 8 * plane;
            int p0 = (int)((lo >> (16 + sh)) & 255u), q0 = (int)((hi >> sh) & 255u);
            deblock_chroma_line((int)((lo >> sh) & 255u), p0, q0, (int)((hi >> (16 + sh)) & 255u), (int)((packed >> sh) & 255u));
            out_lo |= (uint32_t)p0 << (16 + sh);
            out_hi |= (uint32_t)q0 << sh;
        }
        word[0] = out_lo;
        word[1] = out_hi;
    }
}

// horizontal edges: lane = byte column l (plane l & 1, pair l >> 1) of all four edges, p1 p0 | q0 q1 down rows 8 j + 2 .. 8 j + 5
__device__ __forceinline__ void chroma_horizontal(ChromaSlab &m, int l)
{
    uint8_t *bytes = reinterpret_cast<uint8_t *>(m.rows);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tc = (int)((m.edge[1][j][((l >> 1) + 4) >> 3] >> (8 * (l & 1))) & 255u);
        if (!tc) continue;
        uint8_t *col = bytes + (8 * j + 2) * kRowBytes + l;
        int p0 = col[kRowBytes], q0 = col[2 * kRowBytes];
        deblock_chroma_line(col[0], p0, q0, col[3 * kRowBytes], tc);
        col[kRowBytes] = (uint8_t)p0;
        col[2 * kRowBytes] = (uint8_t)q0;
    }
}

// ---- kernels: blockIdx.x walks the units in raster order -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void deblock_luma_kernel(const uint8_t *in, uint8_t *out, DeblockSide s, int units_x)
{
    __shared__ LumaSlab m;
    const int t = (int)threadIdx.x, uy = (int)(blockIdx.x / (unsigned)units_x), ux = (int)(blockIdx.x - (unsigned)uy * (unsigned)units_x);
    luma_load(s, in, m, ux, uy, t);
    __syncthreads();
    luma_vertical(m, t);
    __syncthreads();
    luma_horizontal(m, t);
    __syncthreads();
    luma_store(s, out, m, ux, uy, t);
}

// four units per workgroup, one per wave; a wave past the last unit only keeps the barriers company
__global__ __launch_bounds__(256) void deblock_chroma_kernel(const uint8_t *in, uint8_t *out, DeblockSide s, int units_x, unsigned n_units)
{
    __shared__ ChromaSlab slabs[4];
    const int l = (int)(threadIdx.x & 63);
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), u = blockIdx.x * 4 + wave;
    const bool active = u < n_units;
    const int uy = (int)(u / (unsigned)units_x), ux = (int)(u - (unsigned)uy * (unsigned)units_x);
    ChromaSlab &m = slabs[wave];
    if (active) chroma_load(s, in, m, ux, uy, l);
    __syncthreads();
    if (active) chroma_vertical(m, l);
    __syncthreads();
    if (active) chroma_horizontal(m, l);
    __syncthreads();
    if (active) chroma_store(s, out, m, ux, uy, l);
}

// m_Y and m_C of a unit in one workgroup: waves 0..3 its luma, wave 4 its chroma, through the same functions as the two kernels above
__global__ __launch_bounds__(320) void deblock_kernel(const uint8_t *in, uint8_t *out, DeblockSide s, int units_x)
{
    __shared__ LumaSlab luma;
    __shared__ ChromaSlab chroma;
    const int t = (int)threadIdx.x, uy = (int)(blockIdx.x / (unsigned)units_x), ux = (int)(blockIdx.x - (unsigned)uy * (unsigned)units_x);
    const bool is_luma = t < 256;                                         // uniform per wave
    if (is_luma) luma_load(s, in, luma, ux, uy, t);
    else         chroma_load(s, in, chroma, ux, uy, t - 256);
    __syncthreads();
    if (is_luma) luma_vertical(luma, t);
    else         chroma_vertical(chroma, t - 256);
    __syncthreads();
    if (is_luma) luma_horizontal(luma, t);
    else         chroma_horizontal(chroma, t - 256);
    __syncthreads();
    if (is_luma) luma_store(s, out, luma, ux, uy, t);
    else         chroma_store(s, out, chroma, ux, uy, t - 256);
}

}  // namespace

hipError_t launch_deblock(int planes, const x266_ref_block_t *d_in, x266_ref_block_t *d_out, int width, int height, const x266_deblock_t &p,
                          hipStream_t stream)
{
    DeblockSide s;
    s.cls = p.d_class;
    s.intra = p.d_intra;
    s.qps = p.d_qp;
    s.nnz = p.d_nnz;
    s.mv = p.d_mv;
    s.qp = p.qp;
    s.beta_off = 2 * p.beta_offset_div2;
    s.tc_off = 2 * p.tc_offset_div2;
    s.width = width;
    s.height = height;
    s.tiles_x = width / 16;
    s.ctus_x = (width + 63) / 64;
    const int units_x = (width + 4 + 63) / 64, units_y = (height + 4 + 63) / 64;
    const size_t n_units = (size_t)units_x * (size_t)units_y;
    if (n_units > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(d_in);
    uint8_t *out = reinterpret_cast<uint8_t *>(d_out);
    if (planes == 1)      hipLaunchKernelGGL(deblock_luma_kernel, dim3((unsigned)n_units), dim3(256), 0, stream, in, out, s, units_x);
    else if (planes == 2) hipLaunchKernelGGL(deblock_chroma_kernel, dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, stream, in, out, s, units_x, (unsigned)n_units);
    else                  hipLaunchKernelGGL(deblock_kernel, dim3((unsigned)n_units), dim3(320), 0, stream, in, out, s, units_x);
    return hipGetLastError();
}

}  // namespace x266
