// x266_alf.hpp -- adaptive loop filter: the one copy of the tables (VAR, TT, the tap positions), of the turn G_tr, of the class
// decision of a 4x4 block and of the per-sample filter that the kernels of alf_kernels.hip share (classification, statistics,
// apply).  The statement is include/x266hip.h's (xAlfClassifyGpu ...).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace x266 {

constexpr int kAlfClasses = 25;
constexpr int kAlfLumaTaps = 12, kAlfChromaTaps = 6;
constexpr int kAlfLumaWords = 2 + kAlfLumaTaps + kAlfLumaTaps * (kAlfLumaTaps + 1) / 2;          // 92: count, sum y^2, b, A
constexpr int kAlfChromaWords = 2 + kAlfChromaTaps + kAlfChromaTaps * (kAlfChromaTaps + 1) / 2;  // 29
constexpr int kAlfCtuWords = kAlfClasses * kAlfLumaWords + 2 * kAlfChromaWords;                  // 2358
constexpr int kAlfMaxSets = 8;

constexpr int kAlfVar[16] = {0, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4};
constexpr int kAlfTT[8] = {0, 1, 0, 2, 2, 3, 1, 3};
// P[i] = (dx, dy): the upper half of the 7x7 (luma) and of the 5x5 (chroma) diamond; every tap also covers (-dx, -dy)
constexpr int kAlfLumaDx[kAlfLumaTaps] = {0, -1, 0, 1, -2, -1, 0, 1, 2, -3, -2, -1};
constexpr int kAlfLumaDy[kAlfLumaTaps] = {-3, -2, -2, -2, -1, -1, -1, -1, -1, 0, 0, 0};
constexpr int kAlfChromaDx[kAlfChromaTaps] = {0, -1, 0, 1, -2, -1};
constexpr int kAlfChromaDy[kAlfChromaTaps] = {-2, -1, -1, -1, 0, 0};

// the luma tap that covers position (dx, dy) of the diamond, (0, 0) excluded
__host__ __device__ constexpr int alf_luma_tap_at(int dx, int dy)
{
    if (dy > 0 || (dy == 0 && dx > 0)) { dx = -dx; dy = -dy; }
    return dy == -3 ? 0 : (dy == -2 ? 2 + dx : (dy == -1 ? 6 + dx : 12 + dx));
}

// G_tr
__host__ __device__ constexpr int alf_turn_x(int tr, int dx, int dy) { return (tr & 1) ? dy : dx; }
__host__ __device__ constexpr int alf_turn_y(int tr, int dx, int dy) { return tr == 0 ? dy : (tr == 1 ? dx : (tr == 2 ? -dy : -dx)); }

// The coefficient that a block turned by tr has at the position of tap j: i with G_tr(P[i]) = +-P[j].  G_tr applied twice is the
// identity or the mirror, so i = the tap at G_tr(P[j]); the same map takes a statistic gathered at P[j] to the E_i it belongs to.
__host__ __device__ constexpr int alf_turned_tap(int tr, int j)
{
    return alf_luma_tap_at(alf_turn_x(tr, kAlfLumaDx[j], kAlfLumaDy[j]), alf_turn_y(tr, kAlfLumaDx[j], kAlfLumaDy[j]));
}
// ... for the four tr at once, four bits each
__host__ __device__ constexpr uint32_t alf_turned_taps(int j)
{
    return (uint32_t)alf_turned_tap(0, j) | (uint32_t)alf_turned_tap(1, j) << 4 | (uint32_t)alf_turned_tap(2, j) << 8 | (uint32_t)alf_turned_tap(3, j) << 12;
}

// word of A_ij (i <= j) in a record with n taps: behind count, sum y^2 and the n words of b, the upper triangle row-major
__host__ __device__ constexpr int alf_a_word(int n, int i, int j) { return 2 + n + i * n - i * (i - 1) / 2 + (j - i); }

__device__ __forceinline__ int alf_abs(int v) { return v < 0 ? -v : v; }

// the class byte of a 4x4 block from its four gradient sums: class | tr << 5
__device__ __forceinline__ unsigned alf_class_byte(int v, int h, int d0, int d1)
{
    int hv1, hv0, dir_hv, dd1, dd0, dir_d;
    if (v > h) { hv1 = v; hv0 = h; dir_hv = 1; } else { hv1 = h; hv0 = v; dir_hv = 3; }
    if (d0 > d1) { dd1 = d0; dd0 = d1; dir_d = 0; } else { dd1 = d1; dd0 = d0; dir_d = 2; }
    int m1, m0, dir1, dir2;                                                  // each sum <= 16320: the products fit 32 bits
    if (dd1 * hv0 > hv1 * dd0) { m1 = dd1; m0 = dd0; dir1 = dir_d; dir2 = dir_hv; } else { m1 = hv1; m0 = hv0; dir1 = dir_hv; dir2 = dir_d; }
    const int dir_s = 2 * m1 > 9 * m0 ? 2 : (m1 > 2 * m0 ? 1 : 0);
    const int idx = (h + v) >> 5;
    const int act = kAlfVar[idx < 15 ? idx : 15];
    const int cls = act + (dir_s ? 5 * (((dir1 & 1) << 1) + dir_s) : 0);
    return (unsigned)cls | (unsigned)kAlfTT[2 * dir1 + (dir2 >> 1)] << 5;
}

// a class byte as read back from an array: class = min(b & 31, 24), tr = b >> 5 & 3
__device__ __forceinline__ int alf_class_of(unsigned b) { return (int)((b & 31u) < 24u ? (b & 31u) : 24u); }
__device__ __forceinline__ int alf_turn_of(unsigned b) { return (int)((b >> 5) & 3u); }

// K[clip & 3] - 1, which fits a byte
__device__ __forceinline__ unsigned alf_clip_minus_1(unsigned clip) { return (0x01071FFFu >> (8 * (clip & 3u))) & 255u; }

__device__ __forceinline__ int alf_clamp(int v, int k) { return v < -k ? -k : (v > k ? k : v); }

// one tap of the filter sum: coef (clamp(a - c, -k, k) + clamp(b - c, -k, k))
__device__ __forceinline__ int alf_tap(int coef, int k, int c, int a, int b) { return coef * (alf_clamp(a - c, k) + alf_clamp(b - c, k)); }

// out = clip8(c + ((s + 64) >> 7))
__device__ __forceinline__ int alf_round(int c, int s)
{
    const int v = c + ((s + 64) >> 7);
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// the unclipped tap of the statistics
__device__ __forceinline__ int alf_e(int c, int a, int b) { return a + b - 2 * c; }

__host__ __device__ constexpr int alf_ceil_log2(int n) { return n <= 1 ? 0 : (n <= 2 ? 1 : (n <= 4 ? 2 : 3)); }

}  // namespace x266
