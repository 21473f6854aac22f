// subpel_kernels.hip -- quarter-sample inter prediction on tiled frames (the convention of include/x266hip.h): fractional motion
// compensation of luma and 4:2:0 chroma (xMotionCompQpelLumaGpu / ChromaGpu / Gpu) and the quarter-sample SATD refinement of
// integer vectors (xSatd8x8RefineQpelFromTilesGpu), and their bi-directional counterparts from two references (xMotionCompBiQpelTiles,
// xSatd8x8BiCostsFromTiles, xSatd8x8RefineBiQpelFromTiles).  The filters and their rounding are x266_interp.hpp's, one copy for all.
//
// Both stages are separable and run the same way: the lanes of a group each form the unshifted horizontal sums of ONE row of the
// block's window (one load deep, not a chain of dependent row gathers per lane), park them as int16 in a wave-private LDS slot, and
// the vertical stage reads across the rows.  No kernel here synchronises beyond its own wave.  The window-row load, where a block's
// window row lies, the vertical stage over a slot and the 16-lane Hadamard are x266_subpel_blocks.hpp's, shared with the inter
// partition decision (partition_kernels.hip).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_interp.hpp"
#include "x266_subpel_blocks.hpp"

namespace x266 {
namespace {

// One block of one plane by one group of lanes: luma 16 lanes for the 8x8 block `blk` (0..3, raster) of tile `tile`, chroma 8
// lanes for its 4x4 (U, V) block.  Lane l forms the sums of window row l (luma 15 rows, chroma 7; the group's last lane fills a
// slot row nobody reads) into slot[l], then writes four bytes of the prediction: row l >> 1, half l & 1 of
// the block -- four luma samples or two (U, V) pairs, the same eight-byte read of the slot rows in both planes.  A wave's groups
// cover whole tiles, so its stores cover m_Y (256 bytes) or m_C (128 bytes) of each tile completely.
template <bool CHROMA>
__device__ __forceinline__ void mc_qpel_block(const x266_ref_block_t *__restrict__ ref, const x266_me_result_t *__restrict__ mv,
                                              x266_ref_block_t *__restrict__ pred, int width, int height, int tiles_x, size_t tile,
                                              int blk, int l, v4i *slot)
{
    typedef Interp<CHROMA> I;
    constexpr int edge = CHROMA ? 4 : 8, lg = I::kLog2Phases;
    const size_t ty = tile / (size_t)tiles_x, tx = tile - ty * (size_t)tiles_x;
    const x266_me_result_t r = mv[(ty * 2 + (size_t)(blk >> 1)) * (size_t)(2 * tiles_x) + tx * 2 + (size_t)(blk & 1)];
    const int fx = r.mvx & ((1 << lg) - 1), fy = r.mvy & ((1 << lg) - 1);
    const int xs = ((int)tx * 2 + (blk & 1)) * edge + (r.mvx >> lg) - I::kBefore;
    const int ph = CHROMA ? height >> 1 : height;
    int sy = ((int)ty * 2 + (blk >> 1)) * edge + (r.mvy >> lg) - I::kBefore + l;
    sy = sy < 0 ? 0 : (sy > ph - 1 ? ph - 1 : sy);
    const uint8_t *row = reinterpret_cast<const uint8_t *>(ref) + (CHROMA ? 256 : 0) +
                         (size_t)(sy >> (CHROMA ? 3 : 4)) * (size_t)tiles_x * 512 + (sy & (CHROMA ? 7 : 15)) * 16;
    uint32_t w[4];
    load_window_row<CHROMA>(row, xs, width, w);
    int t[8], h[8];
    interp_taps<CHROMA>(fx, t);
    interp_hsums<CHROMA>(w, t, h);
    slot[l] = pack_hsums(h);
    wave_lds_sync();
    interp_taps<CHROMA>(fy, t);
    const int y = l >> 1, half = l & 1;
    uint2 rows[I::kTaps];                                                   // whole 16-byte rows (as the refinement reads them), then the lane's half
#pragma unroll
    for (int k = 0; k < I::kTaps; ++k) {
        const v4i r = slot[y + k];
        rows[k] = half ? make_uint2((uint32_t)r[2], (uint32_t)r[3]) : make_uint2((uint32_t)r[0], (uint32_t)r[1]);
    }
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int col[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < I::kTaps; ++k) col[k] = hsum_of(c < 2 ? rows[k].x : rows[k].y, c & 1);
        out |= (uint32_t)interp_vertical<CHROMA>(col, t) << (8 * c);
    }
    uint8_t *dst = reinterpret_cast<uint8_t *>(pred + tile) + (CHROMA ? 256 : 0) + ((blk >> 1) * edge + y) * 16 + (blk & 1) * 8 + half * 4;
    __builtin_nontemporal_store(out, reinterpret_cast<uint32_t *>(dst));
}

// luma: 64 lanes per tile, four tiles per workgroup; the slots are 16 rows of 16 bytes per group of 16 lanes
__global__ __launch_bounds__(256) void mc_qpel_luma_kernel(const x266_ref_block_t *__restrict__ ref, const x266_me_result_t *__restrict__ mv,
                                                           x266_ref_block_t *__restrict__ pred, int width, int height, int tiles_x, size_t n_tiles)
{
    __shared__ v4i slots[16][16];
    const size_t tile = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    mc_qpel_block<false>(ref, mv, pred, width, height, tiles_x, tile, (threadIdx.x >> 4) & 3, threadIdx.x & 15, slots[threadIdx.x >> 4]);
}

// chroma: 32 lanes per tile, eight tiles per workgroup; 8 rows of 16 bytes per group of 8 lanes
__global__ __launch_bounds__(256) void mc_qpel_chroma_kernel(const x266_ref_block_t *__restrict__ ref, const x266_me_result_t *__restrict__ mv,
                                                             x266_ref_block_t *__restrict__ pred, int width, int height, int tiles_x, size_t n_tiles)
{
    __shared__ v4i slots[32][8];
    const size_t tile = (size_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (tile >= n_tiles) return;
    mc_qpel_block<true>(ref, mv, pred, width, height, tiles_x, tile, (threadIdx.x >> 3) & 3, threadIdx.x & 7, slots[threadIdx.x >> 3]);
}

// m_Y and m_C in one launch, the role fixed per wave as in motion_comp_kernel: a workgroup of three waves takes two tiles, waves 0
// and 1 the luma of one tile each, wave 2 the chroma of both.  The same block function as the two kernels above: bit-identical.
__global__ __launch_bounds__(192) void mc_qpel_kernel(const x266_ref_block_t *__restrict__ ref, const x266_me_result_t *__restrict__ mv,
                                                      x266_ref_block_t *__restrict__ pred, int width, int height, int tiles_x, size_t n_tiles)
{
    __shared__ v4i luma_slots[8][16];
    __shared__ v4i chroma_slots[8][8];
    if (threadIdx.x < 128) {
        const size_t tile = (size_t)blockIdx.x * 2 + (threadIdx.x >> 6);
        if (tile >= n_tiles) return;
        mc_qpel_block<false>(ref, mv, pred, width, height, tiles_x, tile, (threadIdx.x >> 4) & 3, threadIdx.x & 15, luma_slots[threadIdx.x >> 4]);
    } else {
        const unsigned t = threadIdx.x - 128;
        const size_t tile = (size_t)blockIdx.x * 2 + (t >> 5);
        if (tile >= n_tiles) return;
        mc_qpel_block<true>(ref, mv, pred, width, height, tiles_x, tile, (t >> 3) & 3, t & 7, chroma_slots[t >> 3]);
    }
}

// ---- bi-directional motion compensation ---------------------------------------------------------------------------------------------
// The unrounded V (x266_interp.hpp) of a lane's four outputs from BOTH references: the group's lanes as in mc_qpel_block, one slot
// per list.  Both lists' row loads are issued before the first horizontal stage, so the two fetches overlap.
template <bool CHROMA>
__device__ __forceinline__ void bi_block_v(const x266_ref_block_t *__restrict__ ref0, const x266_ref_block_t *__restrict__ ref1, x266_me_result_t r0,
                                           x266_me_result_t r1, int width, int height, int tiles_x, int tx, int ty, int blk, int l, v4i *slot0, v4i *slot1,
                                           int (&v0)[4], int (&v1)[4])
{
    const WindowRow<CHROMA> s0 = window_row<CHROMA>(ref0, r0, height, tiles_x, tx, ty, blk, l), s1 = window_row<CHROMA>(ref1, r1, height, tiles_x, tx, ty, blk, l);
    uint32_t w0[4], w1[4];
    load_window_row<CHROMA>(s0.row, s0.xs, width, w0);
    load_window_row<CHROMA>(s1.row, s1.xs, width, w1);
    int t[8], h[8];
    interp_taps<CHROMA>(s0.fx, t);
    interp_hsums<CHROMA>(w0, t, h);
    slot0[l] = pack_hsums(h);
    interp_taps<CHROMA>(s1.fx, t);
    interp_hsums<CHROMA>(w1, t, h);
    slot1[l] = pack_hsums(h);
    wave_lds_sync();
    vertical_v4<CHROMA>(slot0, s0.fy, l, v0);
    vertical_v4<CHROMA>(slot1, s1.fy, l, v1);
}

// One block of one plane from two references: the lanes, slots and stores of mc_qpel_block, two slots per group.  A block of
// direction 0 stores nothing (its lanes still take part in the stages: an unused list's record is any int16 vector, and every
// read is clamped into the frame).
template <bool CHROMA>
__device__ __forceinline__ void mc_bi_block(const x266_ref_block_t *__restrict__ ref0, const x266_ref_block_t *__restrict__ ref1,
                                            const x266_me_result_t *__restrict__ mv0, const x266_me_result_t *__restrict__ mv1, const uint8_t *__restrict__ dir,
                                            const x266_wp_t &wp, x266_ref_block_t *__restrict__ pred, int width, int height, int tiles_x, size_t tile, int blk,
                                            int l, v4i *slot0, v4i *slot1)
{
    constexpr int edge = CHROMA ? 4 : 8;
    int tx, ty;
    const size_t b = block_of_tile(tile, tiles_x, blk, &tx, &ty);
    int v0[4], v1[4];
    bi_block_v<CHROMA>(ref0, ref1, mv0[b], mv1[b], width, height, tiles_x, tx, ty, blk, l, slot0, slot1, v0, v1);
    const int d = dir ? dir[b] & 3 : 3;
    if (d == 0) return;
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) out |= (uint32_t)bi_combine(bi_terms(wp, d, CHROMA ? 1 + (c & 1) : 0), v0[c], v1[c]) << (8 * c);
    const int y = l >> 1, half = l & 1;
    uint8_t *dst = reinterpret_cast<uint8_t *>(pred + tile) + (CHROMA ? 256 : 0) + ((blk >> 1) * edge + y) * 16 + (blk & 1) * 8 + half * 4;
    __builtin_nontemporal_store(out, reinterpret_cast<uint32_t *>(dst));
}

// the three launch shapes of the uni kernels above, with two slots per group
__global__ __launch_bounds__(256) void mc_bi_luma_kernel(const x266_ref_block_t *__restrict__ ref0, const x266_ref_block_t *__restrict__ ref1,
                                                         const x266_me_result_t *__restrict__ mv0, const x266_me_result_t *__restrict__ mv1,
                                                         const uint8_t *__restrict__ dir, x266_wp_t wp, x266_ref_block_t *__restrict__ pred, int width, int height,
                                                         int tiles_x, size_t n_tiles)
{
    __shared__ v4i slots[16][2][16];
    const size_t tile = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const unsigned g = threadIdx.x >> 4;
    mc_bi_block<false>(ref0, ref1, mv0, mv1, dir, wp, pred, width, height, tiles_x, tile, g & 3, threadIdx.x & 15, slots[g][0], slots[g][1]);
}

__global__ __launch_bounds__(256) void mc_bi_chroma_kernel(const x266_ref_block_t *__restrict__ ref0, const x266_ref_block_t *__restrict__ ref1,
                                                           const x266_me_result_t *__restrict__ mv0, const x266_me_result_t *__restrict__ mv1,
                                                           const uint8_t *__restrict__ dir, x266_wp_t wp, x266_ref_block_t *__restrict__ pred, int width, int height,
                                                           int tiles_x, size_t n_tiles)
{
    __shared__ v4i slots[32][2][8];
    const size_t tile = (size_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (tile >= n_tiles) return;
    const unsigned g = threadIdx.x >> 3;
    mc_bi_block<true>(ref0, ref1, mv0, mv1, dir, wp, pred, width, height, tiles_x, tile, g & 3, threadIdx.x & 7, slots[g][0], slots[g][1]);
}

__global__ __launch_bounds__(192) void mc_bi_kernel(const x266_ref_block_t *__restrict__ ref0, const x266_ref_block_t *__restrict__ ref1,
                                                    const x266_me_result_t *__restrict__ mv0, const x266_me_result_t *__restrict__ mv1,
                                                    const uint8_t *__restrict__ dir, x266_wp_t wp, x266_ref_block_t *__restrict__ pred, int width, int height,
                                                    int tiles_x, size_t n_tiles)
{
    __shared__ v4i luma_slots[8][2][16];
    __shared__ v4i chroma_slots[8][2][8];
    if (threadIdx.x < 128) {
        const size_t tile = (size_t)blockIdx.x * 2 + (threadIdx.x >> 6);
        if (tile >= n_tiles) return;
        const unsigned g = threadIdx.x >> 4;
        mc_bi_block<false>(ref0, ref1, mv0, mv1, dir, wp, pred, width, height, tiles_x, tile, g & 3, threadIdx.x & 15, luma_slots[g][0], luma_slots[g][1]);
    } else {
        const unsigned t = threadIdx.x - 128, g = t >> 3;
        const size_t tile = (size_t)blockIdx.x * 2 + (t >> 5);
        if (tile >= n_tiles) return;
        mc_bi_block<true>(ref0, ref1, mv0, mv1, dir, wp, pred, width, height, tiles_x, tile, g & 3, t & 7, chroma_slots[g][0], chroma_slots[g][1]);
    }
}

// ---- the three costs of a block: list 0, list 1, both --------------------------------------------------------------------------------
// The luma lanes of mc_bi_luma_kernel.  Each lane holds four differences cur - P_k of one row half; the 8x8 Hadamard runs over the
// group's 16 lanes: two stages inside the lane, one with lane ^ 1 (the other half of the row), three with lane ^ 2, 4, 8 (the
// rows).  The sum of |coefficients| depends on neither the order nor the signs of the butterflies; cost = (sum + 2) >> 2 as
// satd8x8.  The group's lane 0 writes the three costs and the direction of the least of (c0, c1, c2 + penalty), the earlier on a tie.
__global__ __launch_bounds__(256) void satd_bi_costs_kernel(const x266_ref_block_t *__restrict__ cur, const x266_ref_block_t *__restrict__ ref0,
                                                            const x266_ref_block_t *__restrict__ ref1, const x266_me_result_t *__restrict__ mv0,
                                                            const x266_me_result_t *__restrict__ mv1, x266_wp_t wp, uint32_t penalty, uint32_t *__restrict__ costs,
                                                            uint8_t *__restrict__ dir, int width, int height, int tiles_x, size_t n_tiles)
{
    __shared__ v4i slots[16][2][16];
    const size_t tile = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const unsigned g = threadIdx.x >> 4;
    const int blk = (int)(g & 3), l = (int)(threadIdx.x & 15);
    int tx, ty;
    const size_t b = block_of_tile(tile, tiles_x, blk, &tx, &ty);
    int v0[4], v1[4];
    bi_block_v<false>(ref0, ref1, mv0[b], mv1[b], width, height, tiles_x, tx, ty, blk, l, slots[g][0], slots[g][1], v0, v1);
    const uint32_t cw = cur_block_word(cur + tile, blk, l);
    uint32_t cost[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const BiTerms t = bi_terms(wp, k + 1, 0);
        int d[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) d[c] = (int)((cw >> (8 * c)) & 255u) - bi_combine(t, v0[c], v1[c]);
        cost[k] = satd8x8_group16(d, l);
    }
    if (l == 0) {
        if (costs) {
#pragma unroll
            for (int k = 0; k < 3; ++k) store_result4(costs + b * 3 + k, cost[k]);
        }
        if (dir) {
            uint32_t least = cost[0];
            uint8_t best = 1;
            if (cost[1] < least) { least = cost[1]; best = 2; }
            if (cost[2] + penalty < least) best = 3;
            dir[b] = best;
        }
    }
}

// ---- quarter-sample refinement ------------------------------------------------------------------------------------------------------
// One wave per 8x8 block.  All 49 candidates q = 4 m + (dx, dy), dx, dy in -3..3, read one 16x16 window of the reference, rows
// and columns -4..11 around the block moved by m: dx < 0 has integer part m - 1 and phase dx + 4, dx >= 0 integer part m and
// phase dx, so the first tap of output column c sits at window column c + (dx < 0 ? 0 : 1); rows likewise.
//   1. lane L loads dword L & 3 of window row L >> 2 (clamped bytes), lanes 0..15 the block of cur; both go to LDS;
//   2. the 7 x 16 (dx, row) pairs, two per lane, each form the 8 horizontal sums of their row: hs[dx + 3][row][8] as int16;
//   3. lane c < 49 takes candidate (dx, dy) = (c % 7 - 3, c / 7 - 3): the vertical stage over 15 rows of hs[dx + 3], the
//      difference to cur, the 8x8 Hadamard in its own registers (the sum of |coefficients| does not depend on the order of the
//      butterflies, and nothing wraps: |coefficient| <= 64 * 255), cost = (sum + 2) >> 2 as satd8x8;
//   4. the least (cost, rank) over the wave, rank 0 for the centre and 1 + c otherwise: the header's tie rule.
constexpr unsigned kRefineWavesPerWg = 4;

struct RefineSlot {
    v4i window[16];             // 16 rows of 16 bytes
    uint2 cur[8];               // 8 rows of 8 bytes
    v4i hs[7][16];              // [dx + 3][window row]: 8 int16 sums
};

// The body of both refinements.  BI: the cost is that of the bi prediction between the candidate and the fixed list's block
// (ref_fix under mv_fix[b], any int16 quarter-sample vector).  Step 0 forms the fixed list's 8x8 V block: lanes 0..14 each form the
// sums of one window row into hs[0] (which step 2 overwrites later), then lane L takes sample (L >> 3, L & 7) and parks
// V_fix * w_fix + add in 32 bits (V does not fit int16) in fixed[L], so that step 3 adds V_cand * w_cand and rounds.
template <bool BI>
__device__ __forceinline__ void refine_qpel_body(const x266_ref_block_t *cur, const x266_ref_block_t *ref, int width, int height, int tiles_x,
                                                 const x266_me_result_t *mv_int, x266_me_result_t *best, uint32_t *__restrict__ costs, size_t b, int lane,
                                                 RefineSlot &s, const x266_ref_block_t *ref_fix, const x266_me_result_t *mv_fix, const x266_wp_t &wp, int list,
                                                 int *fixed)
{
    const size_t bxn = (size_t)tiles_x * 2, by = b / bxn, bx = b - by * bxn;
    const x266_me_result_t r = mv_int[b];
    const int mx = r.mvx < -8191 ? -8191 : (r.mvx > 8191 ? 8191 : r.mvx), my = r.mvy < -8191 ? -8191 : (r.mvy > 8191 ? 8191 : r.mvy);
    int a_cand = 0, shift = 0;
    if (BI) {                                                               // 0.
        const BiTerms bt = bi_terms(wp, 3, 0);
        a_cand = list ? bt.a1 : bt.a0;
        shift = bt.shift;
        const x266_me_result_t f = mv_fix[b];
        if (lane < 15) {
            const WindowRow<false> src = window_row<false>(ref_fix, f, height, tiles_x, (int)(bx >> 1), (int)(by >> 1), (int)((by & 1) * 2 + (bx & 1)), lane);
            uint32_t w[4];
            load_window_row<false>(src.row, src.xs, width, w);
            int t[8], h[8];
            interp_taps<false>(src.fx, t);
            interp_hsums<false>(w, t, h);
            s.hs[0][lane] = pack_hsums(h);
        }
        wave_lds_sync();
        int t[8], col[8];
        interp_taps<false>(f.mvy & 3, t);
        const int16_t *hs16 = reinterpret_cast<const int16_t *>(s.hs[0]);
#pragma unroll
        for (int k = 0; k < 8; ++k) col[k] = hs16[((lane >> 3) + k) * 8 + (lane & 7)];
        fixed[lane] = interp_vertical_v<false>(col, t) * (list ? bt.a0 : bt.a1) + bt.add;
        wave_lds_sync();                                                    // step 2 overwrites hs[0]
    }
    {   // 1.
        int sy = (int)by * 8 + my - 4 + (lane >> 2);
        sy = sy < 0 ? 0 : (sy > height - 1 ? height - 1 : sy);
        const uint8_t *row = reinterpret_cast<const uint8_t *>(ref) + (size_t)(sy >> 4) * (size_t)tiles_x * 512 + (sy & 15) * 16;
        uint32_t d = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int x = (int)bx * 8 + mx - 4 + 4 * (lane & 3) + e;
            x = x < 0 ? 0 : (x > width - 1 ? width - 1 : x);
            d |= (uint32_t)row[(size_t)(x >> 4) * 512 + (x & 15)] << (8 * e);
        }
        reinterpret_cast<uint32_t *>(s.window)[lane] = d;
        if (lane < 16) {
            const uint8_t *c = reinterpret_cast<const uint8_t *>(cur + (by >> 1) * (size_t)tiles_x + (bx >> 1)) +
                               (((int)by & 1) * 8 + (lane >> 1)) * 16 + ((int)bx & 1) * 8 + (lane & 1) * 4;
            reinterpret_cast<uint32_t *>(s.cur)[lane] = *reinterpret_cast<const uint32_t *>(c);
        }
    }
    wave_lds_sync();
    for (int p = lane; p < 7 * 16; p += 64) {                              // 2.
        const int dx = (p >> 4) - 3, row = p & 15;
        const v4i g = s.window[row];
        const unsigned sh = dx < 0 ? 0u : 8u;
        const uint32_t w[4] = {__builtin_amdgcn_alignbit((uint32_t)g[1], (uint32_t)g[0], sh), __builtin_amdgcn_alignbit((uint32_t)g[2], (uint32_t)g[1], sh),
                               __builtin_amdgcn_alignbit((uint32_t)g[3], (uint32_t)g[2], sh), __builtin_amdgcn_alignbit(0u, (uint32_t)g[3], sh)};
        int t[8], h[8];
        interp_taps<false>(dx & 3, t);
        interp_hsums<false>(w, t, h);
        s.hs[p >> 4][row] = pack_hsums(h);
    }
    wave_lds_sync();
    const int c = lane < 49 ? lane : 48;                                    // 3. (the idle lanes repeat the last candidate)
    const int dyi = c / 7, dxi = c - 7 * dyi, dy = dyi - 3;
    const v4i *hs = s.hs[dxi] + (dy < 0 ? 0 : 1);
    int t[8];
    interp_taps<false>(dy & 3, t);
    v4i rows[15];
#pragma unroll
    for (int k = 0; k < 15; ++k) rows[k] = hs[k];
    int d[8][8];
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        const uint2 cw = s.cur[y];
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            int col[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) col[k] = hsum_of((uint32_t)rows[y + k][x >> 1], x & 1);
            const int pred = BI ? bi_round(interp_vertical_v<false>(col, t) * a_cand + fixed[y * 8 + x], shift) : interp_vertical<false>(col, t);
            d[y][x] = (int)(((x < 4 ? cw.x : cw.y) >> (8 * (x & 3))) & 255u) - pred;
        }
    }
#pragma unroll
    for (int dist = 4; dist >= 1; dist >>= 1)
#pragma unroll
        for (int y = 0; y < 8; ++y)
#pragma unroll
            for (int x = 0; x < 8; ++x)
                if (!(x & dist)) {
                    const int p = d[y][x], q = d[y][x + dist];
                    d[y][x] = p + q;
                    d[y][x + dist] = p - q;
                }
#pragma unroll
    for (int dist = 4; dist >= 1; dist >>= 1)
#pragma unroll
        for (int y = 0; y < 8; ++y)
#pragma unroll
            for (int x = 0; x < 8; ++x)
                if (!(y & dist)) {
                    const int p = d[y][x], q = d[y + dist][x];
                    d[y][x] = p + q;
                    d[y + dist][x] = p - q;
                }
    uint32_t sum = 0;
#pragma unroll
    for (int y = 0; y < 8; ++y)
#pragma unroll
        for (int x = 0; x < 8; ++x) sum += (uint32_t)(d[y][x] < 0 ? -d[y][x] : d[y][x]);
    const uint32_t cost = (sum + 2) >> 2;                                   // < 2^18
    if (costs && lane < 49) store_result4(costs + b * 49 + (size_t)lane, cost);
    uint32_t key = lane < 49 ? (cost << 6 | (lane == 24 ? 0u : (uint32_t)lane + 1u)) : 0xFFFFFFFFu;   // 4.
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)key, m);
        key = o < key ? o : key;
    }
    if (lane == 0) {
        const int rank = (int)(key & 63u), win = rank ? rank - 1 : 24;
        const uint32_t q = (uint32_t)(uint16_t)(4 * mx + win % 7 - 3) | (uint32_t)(uint16_t)(4 * my + win / 7 - 3) << 16;
        *reinterpret_cast<uint2 *>(best + b) = make_uint2(q, key >> 6);
    }
}

__global__ __launch_bounds__(64 * kRefineWavesPerWg) void satd_refine_qpel_kernel(const x266_ref_block_t *cur,
                                                                                   const x266_ref_block_t *ref, int width, int height,
                                                                                   int tiles_x, const x266_me_result_t *mv_int,
                                                                                   x266_me_result_t *best, uint32_t *__restrict__ costs, size_t n_blocks)
{
    __shared__ RefineSlot slots[kRefineWavesPerWg];
    const int lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t b = (size_t)blockIdx.x * kRefineWavesPerWg + wave_in_wg;
    if (b >= n_blocks) return;
    refine_qpel_body<false>(cur, ref, width, height, tiles_x, mv_int, best, costs, b, lane, slots[wave_in_wg], nullptr, nullptr, x266_wp_t{}, 0, nullptr);
}

__global__ __launch_bounds__(64 * kRefineWavesPerWg) void satd_refine_bi_qpel_kernel(const x266_ref_block_t *cur, const x266_ref_block_t *ref_fix,
                                                                                      const x266_me_result_t *mv_fix, const x266_ref_block_t *ref, int list,
                                                                                      x266_wp_t wp, int width, int height, int tiles_x,
                                                                                      const x266_me_result_t *mv_int, x266_me_result_t *best,
                                                                                      uint32_t *__restrict__ costs, size_t n_blocks)
{
    __shared__ RefineSlot slots[kRefineWavesPerWg];
    __shared__ int fixed[kRefineWavesPerWg][64];
    const int lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t b = (size_t)blockIdx.x * kRefineWavesPerWg + wave_in_wg;
    if (b >= n_blocks) return;
    refine_qpel_body<true>(cur, ref, width, height, tiles_x, mv_int, best, costs, b, lane, slots[wave_in_wg], ref_fix, mv_fix, wp, list, fixed[wave_in_wg]);
}

typedef void (*mc_qpel_kernel_fn)(const x266_ref_block_t *, const x266_me_result_t *, x266_ref_block_t *, int, int, int, size_t);

hipError_t launch_mc_qpel_shape(mc_qpel_kernel_fn kernel, unsigned tiles_per_wg, unsigned threads, const x266_ref_block_t *d_ref,
                                const x266_me_result_t *d_mv, x266_ref_block_t *d_pred, int width, int height, hipStream_t stream)
{
    const int tiles_x = width / 16;
    const size_t n_tiles = (size_t)tiles_x * (size_t)(height / 16);
    if (n_tiles == 0) return hipSuccess;
    unsigned wgs;
    if (hipError_t e = wave_grid(n_tiles, tiles_per_wg, &wgs)) return e;
    hipLaunchKernelGGL(kernel, dim3(wgs), dim3(threads), 0, stream, d_ref, d_mv, d_pred, width, height, tiles_x, n_tiles);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_mc_qpel_luma(const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, x266_ref_block_t *d_pred, int width, int height,
                               hipStream_t stream)
{
    return launch_mc_qpel_shape(mc_qpel_luma_kernel, 4, 256, d_ref, d_mv, d_pred, width, height, stream);
}

hipError_t launch_mc_qpel_chroma(const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, x266_ref_block_t *d_pred, int width, int height,
                                 hipStream_t stream)
{
    return launch_mc_qpel_shape(mc_qpel_chroma_kernel, 8, 256, d_ref, d_mv, d_pred, width, height, stream);
}

hipError_t launch_mc_qpel(const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, x266_ref_block_t *d_pred, int width, int height,
                          hipStream_t stream)
{
    return launch_mc_qpel_shape(mc_qpel_kernel, 2, 192, d_ref, d_mv, d_pred, width, height, stream);
}

hipError_t launch_satd_refine_qpel(const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref, int width, int height,
                                   const x266_me_result_t *d_int, x266_me_result_t *d_best, uint32_t *d_costs, hipStream_t stream)
{
    const int tiles_x = width / 16;
    const size_t n_blocks = (size_t)(width / 8) * (size_t)(height / 8);
    if (n_blocks == 0) return hipSuccess;
    unsigned wgs;
    if (hipError_t e = wave_grid(n_blocks, kRefineWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(satd_refine_qpel_kernel, dim3(wgs), dim3(64 * kRefineWavesPerWg), 0, stream, d_cur, d_ref, width, height, tiles_x,
                       d_int, d_best, d_costs, n_blocks);
    return hipGetLastError();
}

hipError_t launch_mc_bi_qpel(int planes, const x266_ref_block_t *d_ref0, const x266_ref_block_t *d_ref1, const x266_me_result_t *d_mv0,
                             const x266_me_result_t *d_mv1, const uint8_t *d_dir, const x266_wp_t &wp, x266_ref_block_t *d_pred, int width, int height,
                             hipStream_t stream)
{
    const int tiles_x = width / 16;
    const size_t n_tiles = (size_t)tiles_x * (size_t)(height / 16);
    if (n_tiles == 0) return hipSuccess;
    const unsigned tiles_per_wg = planes == 1 ? 4 : planes == 2 ? 8 : 2, threads = planes == 3 ? 192 : 256;
    unsigned wgs;
    if (hipError_t e = wave_grid(n_tiles, tiles_per_wg, &wgs)) return e;
    hipLaunchKernelGGL(planes == 1 ? mc_bi_luma_kernel : planes == 2 ? mc_bi_chroma_kernel : mc_bi_kernel, dim3(wgs), dim3(threads), 0, stream, d_ref0, d_ref1,
                       d_mv0, d_mv1, d_dir, wp, d_pred, width, height, tiles_x, n_tiles);
    return hipGetLastError();
}

hipError_t launch_satd_bi_costs(const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref0, const x266_ref_block_t *d_ref1, int width, int height,
                                const x266_me_result_t *d_mv0, const x266_me_result_t *d_mv1, const x266_wp_t &wp, int bi_penalty, uint32_t *d_costs,
                                uint8_t *d_dir, hipStream_t stream)
{
    const int tiles_x = width / 16;
    const size_t n_tiles = (size_t)tiles_x * (size_t)(height / 16);
    if (n_tiles == 0) return hipSuccess;
    unsigned wgs;
    if (hipError_t e = wave_grid(n_tiles, 4, &wgs)) return e;
    hipLaunchKernelGGL(satd_bi_costs_kernel, dim3(wgs), dim3(256), 0, stream, d_cur, d_ref0, d_ref1, d_mv0, d_mv1, wp, (uint32_t)bi_penalty, d_costs, d_dir, width,
                       height, tiles_x, n_tiles);
    return hipGetLastError();
}

hipError_t launch_satd_refine_bi_qpel(const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref_fix, const x266_me_result_t *d_mv_fix,
                                      const x266_ref_block_t *d_ref, const x266_me_result_t *d_int, int list, const x266_wp_t &wp, int width, int height,
                                      x266_me_result_t *d_best, uint32_t *d_costs, hipStream_t stream)
{
    const int tiles_x = width / 16;
    const size_t n_blocks = (size_t)(width / 8) * (size_t)(height / 8);
    if (n_blocks == 0) return hipSuccess;
    unsigned wgs;
    if (hipError_t e = wave_grid(n_blocks, kRefineWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(satd_refine_bi_qpel_kernel, dim3(wgs), dim3(64 * kRefineWavesPerWg), 0, stream, d_cur, d_ref_fix, d_mv_fix, d_ref, list, wp, width, height,
                       tiles_x, d_int, d_best, d_costs, n_blocks);
    return hipGetLastError();
}

}  // namespace x266
