// x266_quality.hpp -- frame quality: the one copy of the arithmetic behind xQualityStatsGpu (quality_kernels.hip) and the host call
// xQualityFromTotals -- the sums of four packed samples, the sums of a 4x4 block, the 8x8 window's Q30 value and the constants.  The
// statement is include/x266hip.h's ("frame quality"); tests/_quality_ref.py restates it in numpy.  Plain C++17 on the host (no HIP:
// tests/cpp/quality_window_check.cpp), packed-byte instructions on the device.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define X266_HD __host__ __device__
#else
#define X266_HD
#endif

namespace x266 {

constexpr unsigned kQualityTotalsThreads = 256;    // lanes of the totals' one workgroup
constexpr unsigned kQualityTotalsChunk = 256;      // records it takes per step (xQualityTotalsChunk): one 48-byte record per lane
constexpr uint32_t kSsimC1 = 416;                  // x264's ssim_c1 for 8-bit samples and 64-sample windows: (.01 * 255)^2 * 64, rounded
constexpr uint32_t kSsimC2 = 235963;               // ... and ssim_c2: (.03 * 255)^2 * 64 * 63, rounded
constexpr int kSsimShift = 30;                     // q is in Q30

// the sum of the four bytes of w, and the dot product of the bytes of a and b
X266_HD inline uint32_t quality_sum4(uint32_t w, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(w, 0u, acc);
#else
    return acc + (w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24);
#endif
}
X266_HD inline uint32_t quality_dot4(uint32_t a, uint32_t b, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, acc, false);
#else
    for (int i = 0; i < 4; ++i) acc += ((a >> (8 * i)) & 255u) * ((b >> (8 * i)) & 255u);
    return acc;
#endif
}

// The sums of a set of co-located samples a (source) and b (decoded): s = sum a | (sum b) << 16, ss = sum (a^2 + b^2), ab = sum a b.
// The packed pair holds up to the window's 64 samples: 64 * 255 < 2^16.  Their squared error is ss - 2 ab.
struct QualitySums {
    uint32_t s, ss, ab;
};
X266_HD inline QualitySums operator+(const QualitySums &x, const QualitySums &y) { return {x.s + y.s, x.ss + y.ss, x.ab + y.ab}; }
// ... of four packed samples of each frame added to acc (a byte that is 0 in both words adds nothing: the chroma planes go through their masks)
X266_HD inline QualitySums quality_add4(QualitySums acc, uint32_t a, uint32_t b)
{
    acc.s = quality_sum4(a, acc.s) + (quality_sum4(b, 0u) << 16);
    acc.ss = quality_dot4(b, b, quality_dot4(a, a, acc.ss));
    acc.ab = quality_dot4(a, b, acc.ab);
    return acc;
}
X266_HD inline uint32_t quality_sse(const QualitySums &x) { return x.ss - 2u * x.ab; }

// q of a window from its four sums.  Every term up to the shifts fits 32 bits (S1^2 <= 16320^2, 64 SS <= 2^29.99): the 64-bit
// quotients are of a numerator below 2^60 by a denominator below 2^30, and |lq|, |cq| <= 2^30.
X266_HD inline int64_t quality_window_q(uint32_t s1, uint32_t s2, uint32_t ss, uint32_t s12, int64_t *cn_out = nullptr)
{
    const uint64_t p11 = (uint64_t)s1 * s1, p22 = (uint64_t)s2 * s2, p12 = (uint64_t)s1 * s2;
    const uint64_t vars = 64u * (uint64_t)ss - p11 - p22;
    const int64_t covar = (int64_t)(64u * (uint64_t)s12) - (int64_t)p12;
    const uint64_t ln = 2u * p12 + kSsimC1, ld = p11 + p22 + kSsimC1;
    const int64_t cn = 2 * covar + (int64_t)kSsimC2;
    const uint64_t cd = vars + kSsimC2;
    const uint64_t lq = (ln << kSsimShift) / ld;
    const uint64_t cm = ((uint64_t)(cn < 0 ? -cn : cn) << kSsimShift) / cd;
    const int64_t cq = cn < 0 ? -(int64_t)cm : (int64_t)cm;
    if (cn_out) *cn_out = cn;
    return ((int64_t)lq * cq) >> kSsimShift;                                // arithmetic: floors
}
X266_HD inline int64_t quality_window_q(const QualitySums &w) { return quality_window_q(w.s & 0xFFFFu, w.s >> 16, w.ss, w.ab); }

// ---- PSNR and SSIM from a frame's totals (host only) -------------------------------------------------------------------------------------
inline double quality_psnr(double sse, double samples) { return sse == 0.0 ? 100.0 : 10.0 * std::log10(65025.0 * samples / sse); }
inline void quality_from_totals(const int64_t total[8], int width, int height, double psnr[4], double ssim[3])
{
    const double n_y = (double)width * (double)height, n_c = n_y / 4.0;
    for (int p = 0; p < 3; ++p) {
        const int64_t win = total[p ? 7 : 6];
        psnr[p] = quality_psnr((double)total[p], p ? n_c : n_y);
        ssim[p] = win == 0 ? 1.0 : (double)total[3 + p] / ((double)win * 1073741824.0);
    }
    psnr[3] = quality_psnr((double)total[0] + (double)total[1] + (double)total[2], n_y + 2.0 * n_c);
}

}  // namespace x266
