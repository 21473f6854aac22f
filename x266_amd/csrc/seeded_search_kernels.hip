// seeded_search_kernels.hip -- xSatd8x8SeededSearchGpu: a small SATD search around per-block starting vectors (the doubled winners of a
// search of the half-size frames, a previous field, the other list's field) with a vector cost, for gfx950.  The contract is
// include/x266hip.h's ("hierarchical motion search"); the arithmetic of the centre list, the walk and the vector cost is x266_seed.hpp's.
//
// One wave per seed cell (an 8x8 block at seed_scale 0, a 16x16 tile = four blocks at seed_scale 1), one launch, no scratch:
//   1. every lane forms the cell's ordered centre list (at most six vectors, wave-uniform) into the wave's LDS slot;
//   2. per centre C the wave stages the reference window the cell's candidates read -- rows and columns -r .. side + r - 1 around the
//      cell moved by C, clamped into the frame, as signed pixels, kSeedPitch bytes per row: (16 + 2r)^2 <= 1 KiB of samples;
//      lanes 0..3 form the Hadamard coefficients of the cell's own blocks on the matrix core (hadamard_lane) and park them in the slot;
//   3. the nb * T candidates of the cell (T = centres * (2r + 1)^2 per block) are dealt to the lanes 64 at a time, block-major, then
//      in walk order: a lane transforms its own 8x8 window (lane = position, as in me_search.hip) and scores it against its block's
//      coefficients with 32 v_sad_u16; satd(cur - ref) = (sum |Hc - Hr| + 2) >> 2 exactly.  J = SATD + vector cost; the lane keeps
//      the least key {J : walk index} per block, so that among equal J the first candidate of the walk wins;
//   4. the keys' minimum over the wave (wave_min, x266_lanes.hpp), per block; lane 0 turns the walk index back into the vector and J back into the SATD.
// Nothing depends on a launch option; the result is a function of the arguments alone.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "x266_device.hpp"
#include "x266_interp.hpp"
#include "x266_me_blocks.hpp"
#include "x266_seed.hpp"

namespace x266 {
namespace {

constexpr unsigned kSeedWavesPerWg = 4;
constexpr int kSeedRows = 16 + 2 * kSeedMaxRange;      // window rows (and columns of samples) at most
// Bytes per window row: a position at column c reads the three dwords from c & ~3, and c <= 8 + 2r = 24, so 36 bytes are read at most;
// 11 dwords: odd, so the rows a wave reads at once spread over the banks.
constexpr int kSeedPitch = 44;
constexpr int kSeedRowDwords = kSeedPitch / 4;
static_assert(((8 + 2 * kSeedMaxRange) & ~3) + 12 <= kSeedPitch, "a position's three dwords stay inside its window row");

struct SeedSlot {
    uint32_t coef[4][32];                                       // the cell's blocks: hadamard_lane's 32 dwords each
    unsigned char win[kSeedMaxCentres][kSeedRows * kSeedPitch]; // one window per centre
    SeedVec centre[kSeedMaxCentres];
};

struct SeedParams {
    const uint8_t *cur, *ref;
    const x266_me_result_t *seed;
    x266_me_result_t *best;
    uint32_t *j;
    int width, height, scale, centres, range, lambda;
    int grid_w, grid_h;
};

__global__ __launch_bounds__(64 * kSeedWavesPerWg) void seeded_search_kernel(const SeedParams P, size_t n_cells)
{
    __shared__ __attribute__((aligned(16))) SeedSlot slots[kSeedWavesPerWg];
    const int lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t cell = (size_t)blockIdx.x * kSeedWavesPerWg + wave_in_wg;
    if (cell >= n_cells) return;                                            // the whole wave: no workgroup barrier follows
    SeedSlot &s = slots[wave_in_wg];
    const int sy = (int)(cell / (size_t)P.grid_w), sx = (int)(cell - (size_t)sy * (size_t)P.grid_w);
    const int r = P.range, side = 8 << P.scale, nb = 1 << (2 * P.scale);
    const int tiles_x = P.width >> 4, blocks_x = P.width >> 3;

    const int n = seed_centre_list(P.seed, P.grid_w, P.grid_h, sx, sy, P.scale, P.centres, s.centre);   // 1. every lane writes the same values
    wave_lds_sync();

    const int x0 = sx * side, y0 = sy * side, rows = side + 2 * r;          // 2.
    for (int ci = 0; ci < n; ++ci) {
        const SeedVec c = s.centre[ci];
        uint32_t *win = reinterpret_cast<uint32_t *>(s.win[ci]);
        for (int i = lane; i < rows * kSeedRowDwords; i += 64) {
            const int ry = i / kSeedRowDwords, d = i - ry * kSeedRowDwords;
            const uint8_t *row = tiled_ref_row(P.ref, P.width, P.height, y0 + c.y - r + ry);
            win[i] = tiled_ref_dword(row, P.width, x0 + c.x - r + 4 * d) ^ 0x80808080u;
        }
    }
    const LaneOps O = make_lane_ops(lane);
    {
        const int j = lane < nb ? lane : nb - 1;                            // the idle lanes repeat the last block
        const uint8_t *src = tile_block_row(P.cur, tiles_x, (sx << P.scale) + (j & 1), (sy << P.scale) + (j >> 1));
        v4i px[4];
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const uint2 q = *reinterpret_cast<const uint2 *>(src + y * 16);
            px[y >> 1][2 * (y & 1)]     = (int)(q.x ^ 0x80808080u);
            px[y >> 1][2 * (y & 1) + 1] = (int)(q.y ^ 0x80808080u);
        }
        uint32_t p[32];
        hadamard_lane(O, px, p);
        if (lane < nb) {
            v4i *dst = reinterpret_cast<v4i *>(s.coef[lane]);
#pragma unroll
            for (int k = 0; k < 8; ++k) dst[k] = v4i{(int)p[4 * k], (int)p[4 * k + 1], (int)p[4 * k + 2], (int)p[4 * k + 3]};
        }
    }
    wave_lds_sync();

    const int T = seed_walk_length(n, r), total = nb * T;                   // 3.
    const SeedVec pred = s.centre[0];
    unsigned long long least[4] = {~0ull, ~0ull, ~0ull, ~0ull};             // per block of the cell: {J : walk index}
    for (int g0 = 0; g0 < total; g0 += 64) {
        const bool valid = g0 + lane < total;
        const int g = valid ? g0 + lane : total - 1;                        // the idle lanes repeat the last candidate
        const int j = g / T, t = g - j * T;
        const SeedStep st = seed_walk_step(t, r);
        v4i px[4];
        load_window8<kSeedPitch>(reinterpret_cast<const unsigned char *>(&s), (int)offsetof(SeedSlot, win) + st.centre * (kSeedRows * kSeedPitch),
                                 8 * (j >> 1) + st.dyi, 8 * (j & 1) + st.dxi, px);
        uint32_t pa[32];
        hadamard_lane(O, px, pa);
        const v4i *cf = reinterpret_cast<const v4i *>(s.coef[j]);
        uint32_t sum = 2u;                                                  // the "+2" of (sum + 2) >> 2
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const v4i q = cf[k];
#pragma unroll
            for (int e = 0; e < 4; ++e) sum = sad16(pa[4 * k + e], (uint32_t)q[e], sum);
        }
        const SeedVec c = s.centre[st.centre];
        const uint32_t cost = (sum >> 2) + seed_vector_cost(P.lambda, c.x + st.dxi - r, c.y + st.dyi - r, pred);
        const unsigned long long key = valid ? ((unsigned long long)cost << 32 | (uint32_t)t) : ~0ull;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (j == b && key < least[b]) least[b] = key;
    }

#pragma unroll
    for (int b = 0; b < 4; ++b) {                                           // 4.
        if (b >= nb) break;
        const unsigned long long v = wave_min(least[b]);
        if (lane == 0) {
            const SeedStep st = seed_walk_step((int)(uint32_t)v, r);
            const SeedVec c = s.centre[st.centre];
            const int vx = c.x + st.dxi - r, vy = c.y + st.dyi - r;
            const uint32_t cost = (uint32_t)(v >> 32);
            const size_t blk = (size_t)((sy << P.scale) + (b >> 1)) * (size_t)blocks_x + (size_t)((sx << P.scale) + (b & 1));
            x266_me_result_t res;
            res.mvx = (int16_t)vx;
            res.mvy = (int16_t)vy;
            res.cost = cost - seed_vector_cost(P.lambda, vx, vy, pred);
            P.best[blk] = res;
            if (P.j) P.j[blk] = cost;
        }
    }
}

}  // namespace

hipError_t launch_seeded_search(const x266_seed_t &p, hipStream_t stream)
{
    SeedParams P;
    P.cur = reinterpret_cast<const uint8_t *>(p.d_cur);
    P.ref = reinterpret_cast<const uint8_t *>(p.d_ref);
    P.seed = p.d_seed;
    P.best = p.d_best;
    P.j = p.d_j;
    P.width = p.width; P.height = p.height; P.scale = p.seed_scale; P.centres = p.centres; P.range = p.range; P.lambda = p.lambda_q4;
    P.grid_w = seed_grid_w(p.width, p.seed_scale);
    P.grid_h = seed_grid_h(p.height, p.seed_scale);
    const size_t n_cells = seed_cells(p.width, p.height, p.seed_scale);
    if (n_cells == 0) return hipSuccess;
    unsigned wgs;
    if (hipError_t e = wave_grid(n_cells, kSeedWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(seeded_search_kernel, dim3(wgs), dim3(64 * kSeedWavesPerWg), 0, stream, P, n_cells);
    return hipGetLastError();
}

}  // namespace x266
