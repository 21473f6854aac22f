// x266_intra.hpp -- the 35-mode 32x32 intra predictor as per-wave building blocks (derivation: intra_kernels.hip), shared by the batch
// kernels of intra_kernels.hip and the frame kernels of intra_frame_kernels.hip: the angle tables in scalar code, sixteen samples of one
// line per lane (predict_line16, in store lanes or in matrix-core fragment lanes), the column-to-row turns through LDS, and the Hadamard
// score of two modes per matrix-core pass (intra_score_modes) on tiles with a 40-byte row pitch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_hadamard.hpp"
#include "x266_mfma_blocks.hpp"

namespace x266 {

// intraPredAngle (H.265 Table 8-4) and |invAngle| (Table 8-5) from the mode, in scalar code: the
// mode is wave-uniform, so these are a handful of SALU selects instead of dependent memory reads.
__device__ __forceinline__ int angle_magnitude(int j)      // j = distance from the pure horizontal / vertical mode, 0..8
{
    const uint32_t lo = 0x09050200u, hi = 0x1A15110Du;      // 0,2,5,9 | 13,17,21,26
    return j >= 8 ? 32 : (int)(((j & 4) ? hi : lo) >> (8 * (j & 3))) & 0xFF;
}
__device__ __forceinline__ int intra_angle(int mode)
{
    const int pure = mode < 18 ? 10 : 26;
    const int j = mode - pure, m = angle_magnitude(j < 0 ? -j : j);
    return (mode < 18) == (j < 0) ? m : -m;                 // horizontal family: positive below 10; vertical: positive above 26
}
__device__ __forceinline__ int intra_inv_angle_magnitude(int j)   // j = 1..8
{
    const int t[8] = {4096, 1638, 910, 630, 482, 390, 315, 256};
    int v = t[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) v = (j == i + 1) ? t[i] : v;
    return v;
}

constexpr int kRawBytes = 144;      // x266_intra_ref_t
constexpr int kExtBytes = 128;      // ref[-32 .. 95]: negative-angle modes only

// a * b + c on two 16-bit lanes, as ONE instruction (written as an expression, the compiler turns "two products plus a constant" into
// multiply, multiply-add, add)
__device__ __forceinline__ uint32_t pk_mad_u16(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t d;
    asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

// 16 samples of one line: taps are the 17 bytes from `p` on (any alignment), weights (32 - f, f).
// Packed 16-bit arithmetic, two samples per instruction: even samples (32-f)*B[2i] + f*B[2i+1],
// odd samples (32-f)*B[2i+1] + f*B[2i+2].
__device__ __forceinline__ void interpolate16(const unsigned char *p, uint32_t f, uint32_t (&px)[4])
{
    const int o = (int)((uintptr_t)p & 3);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - o);
    uint32_t d[6], a[5];
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = q[i];
#pragma unroll
    for (int i = 0; i < 5; ++i) a[i] = __builtin_amdgcn_alignbit(d[i + 1], d[i], (uint32_t)(8 * o));   // bytes p[4i .. 4i+3]
    // weights and rounding term times 8: the ">> 5" becomes ">> 8", i.e. the sample is the HIGH byte of its 16-bit lane and the byte
    // permute that interleaves even and odd samples picks it up for free (255 * 256 + 128 < 2^16: no overflow)
    const uint32_t w0 = (256u - 8u * f) * 0x00010001u, w1 = (8u * f) * 0x00010001u;
    const uint32_t R = 0x00800080u;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const uint32_t t0 = __builtin_amdgcn_perm(0u, a[g], 0x0c020c00u);            // B0, B2
        const uint32_t t1 = __builtin_amdgcn_perm(0u, a[g], 0x0c030c01u);            // B1, B3
        const uint32_t t2 = __builtin_amdgcn_perm(a[g + 1], a[g], 0x0c040c02u);      // B2, B4
        const uint32_t e = pk_mad_u16(t0, w0, pk_mad_u16(t1, w1, R));     // samples 0, 2 (times 256)
        const uint32_t od = pk_mad_u16(t1, w0, pk_mad_u16(t2, w1, R));    // samples 1, 3
        px[g] = __builtin_amdgcn_perm(od, e, 0x07030501u);                // e0 o0 e1 o1, the high bytes
    }
}

// This lane's 16 samples (16h .. 16h+15) of line k of the prediction.  Lines are ROWS for
// planar, DC and the vertical family, COLUMNS for the horizontal family (return value true).
// left / top: the reference set in LDS (top[0] = corner); ext: 128 bytes of wave-private LDS scratch.
// FRAGMENT_LANES false: (k, h) = (lane >> 1, lane & 1), consecutive lanes = consecutive bytes of the 1 KiB prediction (the stores);
// true: (lane & 31, lane >> 5), the lane IS the A-operand fragment of the 32x32 matrix core (row k, K-slots 16h ..).
template <bool FRAGMENT_LANES = false>
__device__ __forceinline__ bool predict_line16(int mode, const unsigned char *left, const unsigned char *top,
                                               unsigned char *ext, int lane, uint32_t (&px)[4])
{
    const int k = FRAGMENT_LANES ? lane & 31 : lane >> 1, h = FRAGMENT_LANES ? lane >> 5 : lane & 1;
    if (mode >= 2) {
        const int angle = intra_angle(mode);
        const bool vertical = mode >= 18;
        const int t = (k + 1) * angle;
        const int idx = t >> 5;
        const uint32_t f = (uint32_t)(t & 31);
        const unsigned char *line;                          // line[x] = ref[x]
        if (angle >= 0) {
            // ref[x] = p[-1+x][-1] is the top array as it lies; ref[1+i] = p[-1][i] is the left array
            // (ref[0] is never a tap when the angle is not negative)
            line = vertical ? top : left - 1;
        } else {
            // negative angles: the other side's samples, projected with invAngle, sit in front of
            // ref[0].  Build ref[-32 .. 64] in ext (two positions per lane).
            const int inv = intra_inv_angle_magnitude(vertical ? 26 - mode : mode - 10);
            const int last = angle;                         // (32 * angle) >> 5
#pragma unroll
            for (int rep = 0; rep < 2; ++rep) {
                const int e = lane + 64 * rep, x = e - 32;
                unsigned v = 0;
                if (x >= 0) {
                    if (x <= 64) v = vertical ? top[x] : (x == 0 ? top[0] : left[x - 1]);
                } else if (last < -1 && x >= last) {
                    const int s = -1 + ((-x * inv + 128) >> 8);              // x * invAngle, invAngle = -inv
                    v = vertical ? left[s] : top[1 + s];
                }
                ext[e] = (unsigned char)v;
            }
            __builtin_amdgcn_wave_barrier();
            line = ext + 32;
        }
        interpolate16(line + 16 * h + idx + 1, f, px);
        return !vertical;
    }
    if (mode == 1) {                                        // DC: 32 top + 32 left samples
        uint32_t s = lane < 32 ? (uint32_t)top[1 + lane] + (uint32_t)left[lane] : 0u;
        s = sum_over_row16(s);
        s = (uint32_t)(__builtin_amdgcn_readlane((int)s, 0) + __builtin_amdgcn_readlane((int)s, 16));   // lanes 32.. hold zeros
        const uint32_t dc = (s + 32u) >> 6;
        px[0] = px[1] = px[2] = px[3] = dc * 0x01010101u;
        return false;
    }
    // planar, row y = k, columns 16h..: ((31-x) L + (x+1) TR + (31-y) T[x] + (y+1) BL + 32) >> 6
    //   = (C + x (TR - L) + (31-y) T[x]) >> 6,  C = 31 L + TR + (y+1) BL + 32: a per-lane ramp plus one
    // multiply per sample, in packed 16-bit lanes (the ramps wrap modulo 2^16 on the way; every finished sum is below 2^16).
    typedef unsigned short v2u __attribute__((ext_vector_type(2)));
    const int tr = top[33], bl = left[32], y = k, lv = left[y];
    const int D = tr - lv, x0 = 16 * h;
    // everything times 4: the ">> 6" becomes ">> 8" and the interleaving byte permute takes the high bytes (4 * (255 * 64 + 32) < 2^16)
    const int c0 = 4 * (31 * lv + tr + (y + 1) * bl + 32 + x0 * D), D4 = 4 * D;
    v2u re = {(unsigned short)c0, (unsigned short)(c0 + 2 * D4)}, ro = {(unsigned short)(c0 + D4), (unsigned short)(c0 + 3 * D4)};
    const v2u inc = {(unsigned short)(4 * D4), (unsigned short)(4 * D4)};
    const unsigned short wy = (unsigned short)(4 * (31 - y));
    const v2u W = {wy, wy};
    const uint32_t *q = reinterpret_cast<const uint32_t *>(top + x0);               // top[1 + x0 ..]: one byte past a dword boundary
    uint32_t d[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) d[i] = q[i];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const uint32_t a = __builtin_amdgcn_alignbit(d[g + 1], d[g], 8u);
        const v2u t0 = __builtin_bit_cast(v2u, __builtin_amdgcn_perm(0u, a, 0x0c020c00u));
        const v2u t1 = __builtin_bit_cast(v2u, __builtin_amdgcn_perm(0u, a, 0x0c030c01u));
        const v2u e = t0 * W + re, od = t1 * W + ro;
        px[g] = __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, od), __builtin_bit_cast(uint32_t, e), 0x07030501u);
        re += inc;
        ro += inc;
    }
    return false;
}

// lane (k, h) holds samples 16h..16h+15 of COLUMN k in px[]; afterwards it holds 16 consecutive samples of a ROW and the return value
// is their byte offset in the row-major 32x32 prediction.  The columns go to LDS as they are (a column-major tile, one b128 write per
// lane) and come back through gfx950's transposing read, which turns 8x8 byte blocks: ds_read_b64_tr_b8 hands lane 16q + 8p + e, as
// byte j, element e of the 8 bytes lane 16q + 2j + p addressed (tools/probes/lds_tr8_read_test.hip).  Source lane 16q + 2j + p addresses
// column 16H + j (second read: + 8), rows R..R+7 of block (R, H) = (8 ((2q + p) & 3), (2q + p) >> 2); the receiving lane holds row
// R + e, columns 16H..16H+15.  (Round 3 scattered the column with sixteen ds_write_b8 per lane.)
__device__ __forceinline__ unsigned turn_columns(unsigned char *cm, int lane, uint32_t (&px)[4])
{
    typedef uint32_t u2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<v4i *>(cm + lane * 16) = v4i{(int)px[0], (int)px[1], (int)px[2], (int)px[3]};      // cm[32 k + 16 h ..]
    const int q = lane >> 4, s = lane & 15;
    const int src_blk = 2 * q + (s & 1);
    const unsigned src = (unsigned)(uintptr_t)cm + (unsigned)((16 * (src_blk >> 2) + (s >> 1)) * 32 + 8 * (src_blk & 3));   // low 32 bits of the generic pointer = LDS offset
    u2 a, b;
    asm volatile("ds_read_b64_tr_b8 %0, %2\n\tds_read_b64_tr_b8 %1, %2 offset:256\n\ts_waitcnt lgkmcnt(0)" : "=&v"(a), "=&v"(b) : "v"(src) : "memory");
    px[0] = a.x; px[1] = a.y; px[2] = b.x; px[3] = b.y;
    const int blk = 2 * q + ((lane >> 3) & 1);
    return (unsigned)((8 * (blk & 3) + (lane & 7)) * 32 + 16 * (blk >> 2));
}

// lane (k, h) = (lane & 31, lane >> 5) holds samples 16h.. of COLUMN k; afterwards rows: the same lane holds row k, columns 16h..
// (ds_read_b64_tr_b8, see turn_columns: receiving lane 16q + 8p + e gets row R + e of the 8x8 byte block the source lanes 16q + 2j + p
// address; here R = 16 (q & 1) + 8 p and the blocks' columns are 16 (q >> 1) + j [+ 8 for the second read])
__device__ __forceinline__ void turn_columns_to_fragment(unsigned char *cm, int lane, uint32_t (&px)[4])
{
    typedef uint32_t u2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<v4i *>(cm + (lane & 31) * 32 + (lane >> 5) * 16) = v4i{(int)px[0], (int)px[1], (int)px[2], (int)px[3]};   // column-major tile
    const int q = lane >> 4, s = lane & 15;
    const unsigned src = (unsigned)(uintptr_t)cm + (unsigned)((16 * (q >> 1) + (s >> 1)) * 32 + 16 * (q & 1) + 8 * (s & 1));
    u2 a, b;
    asm volatile("ds_read_b64_tr_b8 %0, %2\n\tds_read_b64_tr_b8 %1, %2 offset:256\n\ts_waitcnt lgkmcnt(0)" : "=&v"(a), "=&v"(b) : "v"(src) : "memory");
    px[0] = a.x; px[1] = a.y; px[2] = b.x; px[3] = b.y;
}


// ---- the Hadamard score of a prediction against the source (intra_kernels.hip, "mode decision") -----------------------------------------
// Tiles of the decision have a 40-byte row pitch and the second prediction tile starts 32 bytes past a
// 256-byte boundary: the 8-byte window reads of the 16 + 16 sub-blocks then fall into 32 distinct bank pairs
// (with a 32-byte pitch all four sub-block rows and both tiles share banks: 8-way conflicts).
constexpr int kPitch = 40, kTile = 32 * kPitch, kTileB = kTile + 32;

// lane (n, half): rows 4*half .. +3 of sub-block n & 15 (sy = bits 3:2, sx = bits 1:0); columns 16..31 repeat 0..15
__device__ __forceinline__ unsigned cost_window_offset(int lane)
{
    const int half = lane >> 5, sb = lane & 15;
    return (unsigned)((8 * (sb >> 2) + 4 * half) * kPitch + 8 * (sb & 3));
}
__device__ __forceinline__ void cost_window(const unsigned char *tile, unsigned frag, v4i &w0, v4i &w1)
{
    const uint2 r0 = *reinterpret_cast<const uint2 *>(tile + frag), r1 = *reinterpret_cast<const uint2 *>(tile + frag + kPitch);
    const uint2 r2 = *reinterpret_cast<const uint2 *>(tile + frag + 2 * kPitch), r3 = *reinterpret_cast<const uint2 *>(tile + frag + 3 * kPitch);
    w0 = v4i{(int)r0.x, (int)r0.y, (int)r1.x, (int)r1.y};
    w1 = v4i{(int)r2.x, (int)r2.y, (int)r3.x, (int)r3.y};
}

// the lane's 16 source samples (row lane >> 1, columns 16 (lane & 1) ..) into the pitched source tile, offset to signed
__device__ __forceinline__ void cost_stage_source(unsigned char *stile, int lane, const v4i &samples)
{
    const v4i S = {(int)0x80808080u, (int)0x80808080u, (int)0x80808080u, (int)0x80808080u};   // pixels -> signed; the offset cancels
    const v4i sv = samples ^ S;
    unsigned char *d = stile + (lane >> 1) * kPitch + (lane & 1) * 16;                          // 8-byte aligned rows
    *reinterpret_cast<uint2 *>(d) = make_uint2((uint32_t)sv[0], (uint32_t)sv[1]);
    *reinterpret_cast<uint2 *>(d + 8) = make_uint2((uint32_t)sv[2], (uint32_t)sv[3]);
}

// c_a / c_b = sum over the sixteen 8x8 sub-blocks of satd8x8(src - tile) for the two signed pitched tiles at ptile and ptile + kTileB, which the
// wave has written and fenced with a wave barrier; cs = hadamard_pack of the source windows of the lane (lanes 16 .. 31 and 48 .. 63 score the
// second tile: their cs may come from a second source tile).  Any prediction is scored here: the intra modes below, an inter prediction staged
// with cost_stage_source.
__device__ __forceinline__ void score_tiles(const unsigned char *ptile, const HadamardOps &H, const uint32_t (&cs)[16], int lane, unsigned frag,
                                            uint32_t &c_a, uint32_t &c_b)
{
    v4i w0, w1;
    cost_window(ptile + ((lane & 31) >> 4) * kTileB, frag, w0, w1);
    uint32_t p[16];
    hadamard_pack(H, w0, w1, p);
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s = __builtin_amdgcn_sad_u16(p[k], cs[k], s);
    s = sum_with_other_half(s);                          // the other half of the coefficient rows
    const uint32_t c = sum_over_row16((s + 2u) >> 2);    // satd8x8 of this sub-block, summed over the sixteen sub-blocks (one row of lanes per tile)
    __builtin_amdgcn_wave_barrier();
    c_a = (uint32_t)__builtin_amdgcn_readlane((int)c, 0);
    c_b = (uint32_t)__builtin_amdgcn_readlane((int)c, 16);
}

// c_a / c_b = sum over the sixteen 8x8 sub-blocks of satd8x8(src - prediction mode_a / mode_b), cs = hadamard_pack of the source tile's
// windows.  The two predictions go to the tiles ptile and ptile + kTileB; without have_b the second tile keeps what it held and c_b means nothing.
__device__ __forceinline__ void intra_score_modes(int mode_a, int mode_b, bool have_b, const unsigned char *left, const unsigned char *top,
                                                  unsigned char *ext, unsigned char *ptile, const HadamardOps &H, const uint32_t (&cs)[16],
                                                  int lane, unsigned frag, uint32_t &c_a, uint32_t &c_b)
{
#pragma unroll 1
    for (int t = 0; t < 2; ++t) {
        if (t && !have_b) break;
        const int mode = t ? mode_b : mode_a;
        uint32_t px[4];
        const bool columns = predict_line16(mode, left, top, ext, lane, px);
#pragma unroll
        for (int g = 0; g < 4; ++g) px[g] ^= 0x80808080u;
        unsigned char *tile = ptile + t * kTileB;
        unsigned at = (unsigned)((lane >> 1) * kPitch + (lane & 1) * 16);
        if (columns) {                                   // turned inside the tile's own first KiB (one wave: its LDS operations execute in order)
            const unsigned o = turn_columns(tile, lane, px);
            at = (o >> 5) * kPitch + (o & 31);
        }
        *reinterpret_cast<uint2 *>(tile + at) = make_uint2(px[0], px[1]);
        *reinterpret_cast<uint2 *>(tile + at + 8) = make_uint2(px[2], px[3]);
    }
    __builtin_amdgcn_wave_barrier();
    score_tiles(ptile, H, cs, lane, frag, c_a, c_b);
}

}  // namespace x266
