// quality_kernels.hip -- frame quality (xQualityStatsGpu): per CTU the squared error and the summed Q30 SSIM of a decoded tiled frame against
// its source, for luma and both chroma planes, and their frame totals.  The contract is include/x266hip.h's, the arithmetic x266_quality.hpp's.
//
// Statistics: ONE workgroup of 256 lanes takes one CTU, 16 lanes per tile, tile (i & 3, i >> 2) of the CTU for lanes 16 i .. 16 i + 15.  Lane r of
// a tile reads luma row r of both frames (16 bytes each: one dword per 4x4 block column) and 8 bytes of chroma of both: chroma row 4 ((r >> 2) & 1)
// + (r & 3), half r >> 3 -- four (U, V) pairs, one 4x4 block column of each plane, U and V split by their byte masks.  Sums are v_sad_u8 against 0,
// products v_dot4_u32_u8; the squared error is sum a^2 + sum b^2 - 2 sum a b of the same three sums the windows need.  Either way the four rows
// of a block are the four lanes of a quad: quad permutes leave lane k of the quad with the sums of luma block column k (lanes 0 and 1: of the U
// and of the V block), which it stores into the CTU's grid of block sums in LDS: 17x17 luma and 9x9 per chroma plane, three dwords per
// block.  The grids' last column and row are the halo: a second pass of 144 lanes takes the nine tiles right of and below the CTU the same way and
// stores their first block column / row.  A tile off the frame is not read and its blocks are not stored; no window reaches them.  Then one lane per
// window -- 256 luma, then 64 per chroma plane -- adds its four blocks and does the two 64-bit divisions, and a workgroup reduction (wave_sum,
// then four partial sums through LDS) gives the 48-byte record.  The SSE-only instantiation has no halo pass, no grid and no division.
// Totals: ONE workgroup walks the records kQualityTotalsChunk at a time, a record per lane -- integer sums in a fixed order, no atomics
// (workgroup_totals, x266_lanes.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_ctu_tiles.hpp"
#include "x266_device.hpp"
#include "x266_quality.hpp"

namespace x266 {
namespace {

typedef unsigned v2u __attribute__((ext_vector_type(2)));
constexpr unsigned kQualityThreads = 256, kQualityWaves = kQualityThreads / 64;
constexpr unsigned kGridY = 17, kGridC = 9;         // block sums of a CTU and its halo: luma, one chroma plane
static_assert(sizeof(x266_quality_ctu_t) == 48, "the record is 48 bytes");
static_assert(sizeof(x266_ref_block_t) == 512, "a tile is 512 bytes");

// Sums over the four lanes of a quad that leave every lane with the one sum it stores: each step a lane keeps half of what it holds and takes the
// other lane's share of that half, so four values cost three permutes, not eight.
__device__ __forceinline__ uint32_t from_quad_xor1(uint32_t x) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, true); }    // quad_perm [1,0,3,2]
__device__ __forceinline__ uint32_t from_quad_xor2(uint32_t x) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, true); }    // quad_perm [2,3,0,1]
// lane k of the quad gets the quad's sum of x_k
__device__ __forceinline__ uint32_t quad_sum_of_mine(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, unsigned k)
{
    const bool odd = k & 1, high = k & 2;
    const uint32_t a = (odd ? x1 : x0) + from_quad_xor1(odd ? x0 : x1);      // lanes 0, 2: x0 of the pair; lanes 1, 3: x1
    const uint32_t b = (odd ? x3 : x2) + from_quad_xor1(odd ? x2 : x3);      // ... x2; x3
    return (high ? b : a) + from_quad_xor2(high ? a : b);
}
// even lanes get the quad's sum of x0, odd lanes of x1
__device__ __forceinline__ uint32_t quad_sum_of_mine(uint32_t x0, uint32_t x1, unsigned k)
{
    const bool odd = k & 1;
    const uint32_t a = (odd ? x1 : x0) + from_quad_xor1(odd ? x0 : x1);
    return a + from_quad_xor2(a);
}

// the block sums of a grid in LDS: three planes of dwords
template <unsigned N> struct BlockGrid {
    uint32_t s[N][N], ss[N][N], ab[N][N];
    __device__ __forceinline__ void put(unsigned bx, unsigned by, const QualitySums &v)
    {
        s[by][bx] = v.s;
        ss[by][bx] = v.ss;
        ab[by][bx] = v.ab;
    }
    __device__ __forceinline__ QualitySums get(unsigned bx, unsigned by) const { return {s[by][bx], ss[by][bx], ab[by][bx]}; }
    __device__ __forceinline__ QualitySums window(unsigned bx, unsigned by) const { return get(bx, by) + get(bx + 1, by) + get(bx, by + 1) + get(bx + 1, by + 1); }
};

template <bool SSIM, bool SSE>
__global__ __launch_bounds__(kQualityThreads) void quality_kernel(const x266_ref_block_t *__restrict__ src, const x266_ref_block_t *__restrict__ dec, TileFrame f,
                                                                  x266_quality_ctu_t *__restrict__ ctu)
{
    __shared__ BlockGrid<kGridY> grid_y;
    __shared__ BlockGrid<kGridC> grid_c[2];
    __shared__ int64_t part[kQualityWaves][8];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = tid & 15, k = r & 3;
    const unsigned cx = blockIdx.x % f.ctus_w, cy = blockIdx.x / f.ctus_w;
    uint32_t sse_y = 0, sse_u = 0, sse_v = 0;
#pragma unroll
    for (unsigned pass = 0; pass < (SSIM ? 2u : 1u); ++pass) {
        // tiles 0..15 are the CTU's, 16..19 the column right of it, 20..23 the row below, 24 the corner
        const unsigned j = pass * 16 + (tid >> 4);
        const unsigned tx = j < 16 ? (j & 3) : j < 20 ? 4 : j < 24 ? j - 20 : 4, ty = j < 16 ? (j >> 2) : j < 20 ? j - 16 : 4;
        const unsigned gx = cx * 4 + tx, gy = cy * 4 + ty;
        const bool active = j < 25 && gx < f.tiles_w && gy < f.tiles_h;      // uniform over the row of 16 lanes
        const unsigned crow = 4 * ((r >> 2) & 1) + k, half = r >> 3;
        v4i ya = {0, 0, 0, 0}, yb = {0, 0, 0, 0};
        v2u ca = {0u, 0u}, cb = {0u, 0u};
        if (active) {                                                       // plain loads: the neighbouring CTUs read the halo tiles as their own
            const size_t t = (size_t)gy * f.tiles_w + gx;
            const uint8_t *pa = reinterpret_cast<const uint8_t *>(src + t), *pb = reinterpret_cast<const uint8_t *>(dec + t);
            ya = load16<false>(pa + r * 16);
            yb = load16<false>(pb + r * 16);
            ca = *reinterpret_cast<const v2u *>(pa + 256 + crow * 16 + half * 8);
            cb = *reinterpret_cast<const v2u *>(pb + 256 + crow * 16 + half * 8);
        }
        QualitySums col[4], u = {0, 0, 0}, v = {0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) col[i] = quality_add4(QualitySums{0, 0, 0}, (uint32_t)ya[i], (uint32_t)yb[i]);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t a = i ? ca.y : ca.x, b = i ? cb.y : cb.x;
            u = quality_add4(u, a & 0x00FF00FFu, b & 0x00FF00FFu);
            v = quality_add4(v, a & 0xFF00FF00u, b & 0xFF00FF00u);
        }
        if (SSE && pass == 0) {                                             // an inactive row's sums are 0
            sse_y = quality_sse(col[0]) + quality_sse(col[1]) + quality_sse(col[2]) + quality_sse(col[3]);
            sse_u = quality_sse(u);
            sse_v = quality_sse(v);
        }
        if (SSIM) {
            const QualitySums mine = {quad_sum_of_mine(col[0].s, col[1].s, col[2].s, col[3].s, k), quad_sum_of_mine(col[0].ss, col[1].ss, col[2].ss, col[3].ss, k),
                                      quad_sum_of_mine(col[0].ab, col[1].ab, col[2].ab, col[3].ab, k)};
            const QualitySums uv = {quad_sum_of_mine(u.s, v.s, k), quad_sum_of_mine(u.ss, v.ss, k), quad_sum_of_mine(u.ab, v.ab, k)};
            const unsigned bx = 4 * tx + k, by = 4 * ty + (r >> 2);
            if (active && bx < kGridY && by < kGridY) grid_y.put(bx, by, mine);
            const unsigned bxc = 2 * tx + half, byc = 2 * ty + ((r >> 2) & 1);
            if (active && k < 2 && bxc < kGridC && byc < kGridC) grid_c[k].put(bxc, byc, uv);
        }
    }
    int64_t q_y = 0, q_u = 0, q_v = 0;
    uint32_t n_y = 0, n_c = 0;
    if (SSIM) {
        __syncthreads();
        const unsigned w4 = f.tiles_w * 4, h4 = f.tiles_h * 4;
        {   // luma: window (tid & 15, tid >> 4) of the CTU
            const unsigned bx = tid & 15, by = tid >> 4;
            if (cx * 16 + bx + 1 < w4 && cy * 16 + by + 1 < h4) {
                q_y = quality_window_q(grid_y.window(bx, by));
                n_y = 1;
            }
        }
        if (tid < 128) {                                                    // chroma: wave 0 plane U, wave 1 plane V
            const unsigned bx = tid & 7, by = (tid >> 3) & 7;
            if (cx * 8 + bx + 1 < w4 / 2 && cy * 8 + by + 1 < h4 / 2) {
                const int64_t q = quality_window_q(grid_c[wave].window(bx, by));
                q_u = wave == 0 ? q : 0;
                q_v = wave == 0 ? 0 : q;
                n_c = wave == 0;                                            // the two planes have the same windows: counted once
            }
        }
    }
    // slots of part: 0..2 ssim Y, U, V; 3 sse Y; 4 sse U | sse V << 32 (a CTU's is at most 1024 * 65025 per plane); 6 win_y | win_c << 16 (at most 256, 64)
    auto to_part = [&](int slot, int64_t v) {
        v = wave_sum(v);
        if (lane == 0) part[wave][slot] = v;
    };
    if (SSIM) {
        to_part(0, q_y);
        to_part(1, q_u);
        to_part(2, q_v);
        to_part(6, (int64_t)(n_y | (n_c << 16)));
    }
    if (SSE) {
        to_part(3, (int64_t)sse_y);
        to_part(4, (int64_t)(sse_u | ((uint64_t)sse_v << 32)));
    }
    __syncthreads();
    if (tid == 0) {
        auto whole = [&](int slot) { return part[0][slot] + part[1][slot] + part[2][slot] + part[3][slot]; };
        static_assert(kQualityWaves == 4, "four partial sums");
        int64_t all[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (SSIM) {
            all[0] = whole(0);
            all[1] = whole(1);
            all[2] = whole(2);
            const int64_t n = whole(6);
            all[6] = n & 0xFFFF;
            all[7] = n >> 16;
        }
        if (SSE) {
            all[3] = whole(3);
            const int64_t uv = whole(4);
            all[4] = uv & 0xFFFFFFFF;
            all[5] = (int64_t)((uint64_t)uv >> 32);
        }
        v4i *rec = reinterpret_cast<v4i *>(ctu + blockIdx.x);
        const v4i r0 = {(int)(uint32_t)all[0], (int)(uint32_t)((uint64_t)all[0] >> 32), (int)(uint32_t)all[1], (int)(uint32_t)((uint64_t)all[1] >> 32)};
        const v4i r1 = {(int)(uint32_t)all[2], (int)(uint32_t)((uint64_t)all[2] >> 32), (int)(uint32_t)all[3], (int)(uint32_t)all[4]};
        const v4i r2 = {(int)(uint32_t)all[5], (int)(uint32_t)all[6], (int)(uint32_t)all[7], 0};
        rec[0] = r0;
        rec[1] = r1;
        rec[2] = r2;
    }
}

// total[0..2] = sse Y, U, V, total[3..5] = ssim Y, U, V, total[6] = win_y, total[7] = win_c, each over all records.  One workgroup; lane t takes
// record step * kQualityTotalsChunk + t as three 16-byte loads.
__global__ __launch_bounds__(kQualityTotalsThreads) void quality_totals_kernel(const x266_quality_ctu_t *__restrict__ ctu, size_t n_ctu, int64_t *__restrict__ total)
{
    constexpr unsigned kWaves = kQualityTotalsThreads / 64;
    static_assert(kQualityTotalsChunk == kQualityTotalsThreads, "a step is one record per lane");
    const unsigned tid = threadIdx.x;
    int64_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t j = tid; j < n_ctu; j += kQualityTotalsChunk) {
        const v4i *rec = reinterpret_cast<const v4i *>(ctu + j);
        const v4i r0 = rec[0], r1 = rec[1], r2 = rec[2];
        acc[3] += (int64_t)(((uint64_t)(uint32_t)r0[1] << 32) | (uint32_t)r0[0]);
        acc[4] += (int64_t)(((uint64_t)(uint32_t)r0[3] << 32) | (uint32_t)r0[2]);
        acc[5] += (int64_t)(((uint64_t)(uint32_t)r1[1] << 32) | (uint32_t)r1[0]);
        acc[0] += (uint32_t)r1[2];
        acc[1] += (uint32_t)r1[3];
        acc[2] += (uint32_t)r2[0];
        acc[6] += (uint32_t)r2[1];
        acc[7] += (uint32_t)r2[2];
    }
    const int64_t all = workgroup_totals<kWaves>(acc, tid);
    if (tid < 8) total[tid] = all;
}

template <bool SSIM, bool SSE>
hipError_t launch_quality(const x266_quality_t &p, const TileFrame &f, unsigned n_ctu, hipStream_t stream)
{
    hipLaunchKernelGGL((quality_kernel<SSIM, SSE>), dim3(n_ctu), dim3(kQualityThreads), 0, stream, p.d_src, p.d_dec, f, p.d_ctu);
    return hipGetLastError();
}

}  // namespace

int quality_totals_chunk() { return (int)kQualityTotalsChunk; }

hipError_t launch_quality_stats(const x266_quality_t &p, hipStream_t stream)
{
    const TileFrame f = tile_frame(p.width, p.height);
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(f.n_ctu, 1, &wgs)) return e;                  // a workgroup per CTU
    const bool ssim = (p.flags & X266_QUALITY_SSIM) != 0, sse = (p.flags & X266_QUALITY_SSE) != 0;
    if (hipError_t e = ssim && sse ? launch_quality<true, true>(p, f, wgs, stream)
                       : ssim      ? launch_quality<true, false>(p, f, wgs, stream)
                                   : launch_quality<false, true>(p, f, wgs, stream))
        return e;
    if (!p.d_total) return hipSuccess;
    hipLaunchKernelGGL(quality_totals_kernel, dim3(1), dim3(kQualityTotalsThreads), 0, stream, p.d_ctu, f.n_ctu, p.d_total);
    return hipGetLastError();
}

}  // namespace x266
