// x266_code_region.hpp -- one 32x32 region through the closed coding loop, held in registers by one wave: forward DCT32 of cur - pred,
// quantise, dequantise, inverse (derivation: dct32_kernels.hip, "the coding loop of a whole CTU").  Shared by dct32_code_ctu_tiles_kernel and
// the intra frame kernels of intra_frame_kernels.hip, so that both code a region with the same instructions.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_mfma_blocks.hpp"
#include "x266_quant.hpp"

namespace x266 {

// a / b: the lane's 16 cur / pred pixels (row lane & 31, columns 16 (lane >> 5) ..).  The levels go to dst_level (the lane's first linear piece of the
// region's 2 KiB, through the 2 KiB converter `slot`), their non-zero count to *nnz (may be NULL); o0 / o1 = the residual IDCT32(Q^-1(level)) of the
// lane's 16 pixels, for recon_luma16 / recon_chroma16.
__device__ __forceinline__ void code_region(const v4i &a, const v4i &b, const LaneConsts &kf, const LaneConsts &ki, const v16i &c2r,
                                            const QuantParams &q, unsigned lane, unsigned char *slot, const TileLanes &t, char *dst_level,
                                            uint32_t *nnz, v4i &o0, v4i &o1)
{
    v4i ylo, yhi;
    pass1_planes<4>(pixels_pass1(a, b, kf), ylo, yhi);
    {
        const v16i acc = fwd_pass2(ylo, yhi, kf);
        uint32_t z[8];
        unsigned nonzero = 0;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int lo = quantise((int)(int16_t)(acc[2 * m] >> 11), q), hi = quantise((int)(int16_t)(acc[2 * m + 1] >> 11), q);
            nonzero += (lo != 0) + (hi != 0);
            z[m] = ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
        }
        v4i s0, s1;
        frag_to_linear(slot, t, v4i{(int)z[0], (int)z[1], (int)z[2], (int)z[3]}, v4i{(int)z[4], (int)z[5], (int)z[6], (int)z[7]}, s0, s1);
        store16_sc1nt(dst_level, s0);
        store16_sc1nt(dst_level + 1024, s1);
        if (nnz) {
            const uint32_t total = wave_sum(nonzero);
            if (lane == 0) *nnz = total;
        }
    }
    v16i acc = fwd_pass2_swapped(ylo, yhi, kf, lane >> 5);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = dequantise(quantise((int)(int16_t)(acc[r] >> 11), q), q);   // bytes 0 / 1 = the int16 coefficient
    v4i zlo, zhi;
    pack_planes(acc, zlo, zhi);
    inv_passes(zlo, zhi, ki, c2r, o0, o1);
}

// region `region` of the frame (6 per CTU): its qp byte clamped to 51, or the scalar qp
__device__ __forceinline__ QuantParams region_quant(const uint8_t *__restrict__ qps, size_t region, unsigned qp, unsigned rounding)
{
    if (qps) {
        qp = uniform_byte(qps, region);
        qp = qp < 51u ? qp : 51u;
    }
    return quant_params(5u, qp, rounding);
}

}  // namespace x266
