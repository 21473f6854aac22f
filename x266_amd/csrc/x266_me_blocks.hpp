// x266_me_blocks.hpp -- the per-wave building blocks of the SATD searches, shared by me_search.hip (the exhaustive search) and
// seeded_search_kernels.hip (the seeded one): the lane = position Hadamard transform on the matrix core (make_lane_ops,
// hadamard_lane), the 8x8 window of a position out of an LDS window of signed pixels (load_window8), the addressing of tiled frames
// (tile_block_row, tiled_ref_row, tiled_ref_dword) and the v_sad_u16 step of the score.  See me_search.hip for the derivation.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_mfma_blocks.hpp"

namespace x266 {

// ---- lane = position Hadamard transform on the matrix core ------------------------------------------
// Output row m of the MFMA lands in lane half (m >> 2) & 1, register r = (m & 3) | (m >> 3) << 2.
// A[m][k], k = 16 h + t: (-1)^popcount(r & t) for h == that half, else 0; t = 8 (y & 1) + x indexes the
// 16 pixels of one K-step (window rows 2s, 2s+1).  `neg` = -A.  `kc`: 32 slots x 32 x 32 = 0x8000.
struct LaneOps { v4i pos, neg, kc; };

__device__ __forceinline__ LaneOps make_lane_ops(int lane)
{
    const uint32_t NEG = 0xFEFEFEFEu;
    const uint32_t m = (uint32_t)lane & 31u, h = (uint32_t)lane >> 5;
    const uint32_t r = (m & 3u) | ((m >> 3) << 2);
    const bool active = ((m >> 2) & 1u) == h;
    const uint32_t inner = (r & 1) ? ((r & 2) ? 0x01FFFF01u : 0xFF01FF01u) : ((r & 2) ? 0xFFFF0101u : 0x01010101u);
    const uint32_t f0 = (r & 4) ? NEG : 0u, f1 = (r & 8) ? NEG : 0u;
    const uint32_t on = active ? 0xFFFFFFFFu : 0u;
    LaneOps o;
    o.pos = v4i{(int)(inner & on), (int)((inner ^ f0) & on), (int)((inner ^ f1) & on), (int)((inner ^ f0 ^ f1) & on)};
    o.neg = v4i{(int)((inner ^ NEG) & on), (int)((inner ^ f0 ^ NEG) & on), (int)((inner ^ f1 ^ NEG) & on), (int)((inner ^ f0 ^ f1 ^ NEG) & on)};
    o.kc = v4i{0x20202020, 0x20202020, 0x20202020, 0x20202020};
    return o;
}

// px[s] = window rows 2s, 2s+1 of this lane's 8x8 window (signed pixels, 16 bytes).  out[k], out[16+k]:
// biased uint16 pairs {coefficient 16 + k | coefficient k}, {48 + k | 32 + k} (natural H64 order
// c = 16 q + r over pixel index 8 y + x; the order is irrelevant under sum |.| as long as the block
// table uses the same one, and it does: every block's coefficients come from this function too).
__device__ __forceinline__ void hadamard_lane(const LaneOps &O, const v4i (&px)[4], uint32_t (&out)[32])
{
    const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // high fields: q = 1 (signs + - + -) and q = 3 (+ - - +) share the bias and their first two K-steps
    v16i t = mfma(O.kc, O.kc, zero);
    t = mfma(O.pos, px[0], t); t = mfma(O.neg, px[1], t);
    v16i a = mfma(O.pos, px[2], t); a = mfma(O.neg, px[3], a);
    v16i b = mfma(O.neg, px[2], t); b = mfma(O.pos, px[3], b);
    // << 16 (a full-rate v_lshlrev_b32; the low field's bias is one more constant MFMA), then q = 0 (+ + + +) and q = 2 (+ + - -)
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = (int)((uint32_t)a[k] << 16);
    a = mfma(O.kc, O.kc, a);
    a = mfma(O.pos, px[0], a); a = mfma(O.pos, px[1], a); a = mfma(O.pos, px[2], a); a = mfma(O.pos, px[3], a);
#pragma unroll
    for (int k = 0; k < 16; ++k) b[k] = (int)((uint32_t)b[k] << 16);
    b = mfma(O.kc, O.kc, b);
    b = mfma(O.pos, px[0], b); b = mfma(O.pos, px[1], b); b = mfma(O.neg, px[2], b); b = mfma(O.neg, px[3], b);
#pragma unroll
    for (int k = 0; k < 16; ++k) { out[k] = (uint32_t)a[k]; out[16 + k] = (uint32_t)b[k]; }
}

// 8x8 bytes at (row, col) of an LDS window whose rows are PITCH bytes apart -> the four K-step operands: three aligned dwords per row
// and a funnel shift.  (gfx950 does serve unaligned ds_read_b64 -- tools/probes/lds_unaligned_test.hip -- which would save the 16
// v_alignbit_b32, but at a fraction of the aligned rate: 2.34 -> 2.49 ms per 4K frame, profiles/r03_me_variants.txt.)  The row offsets
// are immediates (PITCH is a compile-time constant).
template <int PITCH>
__device__ __forceinline__ void load_window8(const unsigned char *lds0, int win_offset, int row, int col, v4i (&px)[4])
{
    const int sh = (col & 3) * 8;
    int off = win_offset + row * PITCH + (col & ~3);
    asm volatile("" : "+v"(off));         // keep the window's LDS offset in the register: y * PITCH then fits the DS offset fields
    const unsigned char *base = lds0 + off;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(base + y * PITCH);
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
        px[y >> 1][2 * (y & 1)]     = (int)__builtin_amdgcn_alignbit(d1, d0, sh);
        px[y >> 1][2 * (y & 1) + 1] = (int)__builtin_amdgcn_alignbit(d2, d1, sh);
    }
}

// ---- tiled frames: sample (y, x) of m_Y at byte ((y >> 4) * (width >> 4) + (x >> 4)) * 512 + (y & 15) * 16 + (x & 15) ----------------
__device__ __forceinline__ const uint8_t *tile_block_row(const uint8_t *tiles, int tiles_x, int bx, int by)
{   // row 0 of 8x8 block (bx, by) of a tiled frame: an aligned quadrant of tile (by >> 1, bx >> 1), rows 16 bytes apart
    return tiles + ((size_t)(by >> 1) * (size_t)tiles_x + (size_t)(bx >> 1)) * 512 + (by & 1) * 128 + (bx & 1) * 8;
}

// Row gy of a tiled frame, gy clamped into the frame: tile (gy >> 4, 0) + (gy & 15) * 16
__device__ __forceinline__ const uint8_t *tiled_ref_row(const uint8_t *ref, int width, int height, int gy)
{
    gy = gy < 0 ? 0 : (gy > height - 1 ? height - 1 : gy);
    return ref + (size_t)(gy >> 4) * (size_t)(width >> 4) * 512 + (gy & 15) * 16;
}

// Reference samples (gy, gx0 .. gx0 + 3) of a tiled frame as one dword, gy inside the frame, every x clamped to [0, width - 1].
// `row` = tile (gy >> 4, 0) + (gy & 15) * 16.  Inside the frame: two aligned dwords (each within one 16-byte tile row; the
// second one is clamped into the frame where the shift makes it unused) and a funnel shift; at the left / right edge: bytes.
__device__ __forceinline__ uint32_t tiled_ref_dword(const uint8_t *row, int width, int gx0)
{
    if (gx0 >= 0 && gx0 + 3 <= width - 1) {
        const int xa = gx0 & ~3, xb = xa + 4 < width ? xa + 4 : xa;
        const uint32_t d0 = *reinterpret_cast<const uint32_t *>(row + (size_t)(xa >> 4) * 512 + (xa & 15));
        const uint32_t d1 = *reinterpret_cast<const uint32_t *>(row + (size_t)(xb >> 4) * 512 + (xb & 15));
        return __builtin_amdgcn_alignbit(d1, d0, (gx0 & 3) * 8);
    }
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        int gx = gx0 + b;
        gx = gx < 0 ? 0 : (gx > width - 1 ? width - 1 : gx);
        v |= (uint32_t)row[(size_t)(gx >> 4) * 512 + (gx & 15)] << (8 * b);
    }
    return v;
}

// two |a - b| of uint16 fields per instruction, added to c
__device__ __forceinline__ uint32_t sad16(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_sad_u16(a, b, c); }

}  // namespace x266
