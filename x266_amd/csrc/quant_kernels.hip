// quant_kernels.hip -- the quantiser over a sequence of 1024-sample regions (xQuantRegionsGpu): coefficients -> levels with the
// count of non-zero levels per region, or levels -> coefficients.  The arithmetic is x266_quant.hpp's; a region has ONE block size
// and ONE qp, so inside a region the operation is purely element-wise and the block-major layout does not matter.
//
// An HBM-bound leg in the house shape: one region per wave, two 1 KiB-linear loads and two 1 KiB-linear stores
// of whole 128-byte lines, a grid as large as the batch walked in address order, no persistent loop, "nt" loads and "sc1 nt"
// stores.  The class and qp bytes are scalar loads (uniform_byte) and the parameters derived from them are computed on the scalar ALU.  In place
// (out == in) is safe: a lane writes exactly the 32 bytes it has read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_quant.hpp"

namespace x266 {
namespace {

constexpr unsigned kQuantWavesPerWg = 4;

template <bool INVERSE>
__global__ __launch_bounds__(64 * kQuantWavesPerWg) void quant_regions_kernel(const int16_t *in, int16_t *out, size_t n_regions,
                                                                             const uint8_t *__restrict__ cls, const uint8_t *__restrict__ qps,
                                                                             unsigned qp, unsigned rounding, uint32_t *__restrict__ nnz)
{
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t r = (size_t)blockIdx.x * kQuantWavesPerWg + wave_in_wg;
    if (r >= n_regions) return;
    const char *src = reinterpret_cast<const char *>(in) + r * 2048 + lane * 16;
    const v4i g0 = load16<true>(src), g1 = load16<true>(src + 1024);
    const unsigned cls_byte = cls ? uniform_byte(cls, r) : 3u, qp_byte = qps ? uniform_byte(qps, r) : qp;   // two scalar loads, one wait
    const unsigned n = 2u + (cls_byte & 3u), q = qp_byte < 51u ? qp_byte : 51u;
    const QuantParams p = quant_params(n, q, rounding);
    const uint32_t w[8] = {(uint32_t)g0[0], (uint32_t)g0[1], (uint32_t)g0[2], (uint32_t)g0[3],
                           (uint32_t)g1[0], (uint32_t)g1[1], (uint32_t)g1[2], (uint32_t)g1[3]};
    uint32_t z[8];
    unsigned nonzero = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) z[m] = INVERSE ? dequantise_pair(w[m], p) : quantise_pair(w[m], p, nonzero);
    char *dst = reinterpret_cast<char *>(out) + r * 2048 + lane * 16;
    store16_sc1nt(dst, v4i{(int)z[0], (int)z[1], (int)z[2], (int)z[3]});
    store16_sc1nt(dst + 1024, v4i{(int)z[4], (int)z[5], (int)z[6], (int)z[7]});
    if (!INVERSE && nnz) {
        const uint32_t total = wave_sum(nonzero);
        if (lane == 0) nnz[r] = total;
    }
}

}  // namespace

hipError_t launch_quant_regions(bool inverse, const int16_t *d_in, int16_t *d_out, size_t n_regions, const uint8_t *d_class,
                                const uint8_t *d_qp, int qp, int rounding, uint32_t *d_nnz, hipStream_t stream)
{
    if (n_regions == 0) return hipSuccess;
    unsigned wgs;
    if (hipError_t e = wave_grid(n_regions, kQuantWavesPerWg, &wgs)) return e;
    const dim3 block(64 * kQuantWavesPerWg);
    if (inverse) hipLaunchKernelGGL(quant_regions_kernel<true>, dim3(wgs), block, 0, stream, d_in, d_out, n_regions, d_class, d_qp, (unsigned)qp, (unsigned)rounding, d_nnz);
    else         hipLaunchKernelGGL(quant_regions_kernel<false>, dim3(wgs), block, 0, stream, d_in, d_out, n_regions, d_class, d_qp, (unsigned)qp, (unsigned)rounding, d_nnz);
    return hipGetLastError();
}

}  // namespace x266
