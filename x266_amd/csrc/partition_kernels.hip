// partition_kernels.hip -- xInterPartitionDecideGpu: the bottom-up quadtree merge of a quarter-sample vector field into partitions of
// 8x8, 16x16, 32x32 and 64x64 samples by SATD plus vector bits, for gfx950.  The contract is include/x266hip.h's ("inter partition
// decision"); the clamp, the node geometry, the predictor, the walk and the rate are x266_part.hpp's, the sample work -- the window-row
// load, the two interpolation stages and the 16-lane Hadamard -- x266_subpel_blocks.hpp's and x266_interp.hpp's, shared with
// subpel_kernels.hip.
//
// One workgroup of 1024 lanes per CTU, one launch, no scratch, no atomics and nothing shared between workgroups: the bytes are the same
// on every run.  A group of 16 lanes owns one 8x8 block of the CTU for the whole kernel and scores it under one vector per pass exactly
// as satd_bi_costs_kernel scores a list: row-per-lane horizontal sums into the group's LDS slot, the vertical stage across the rows,
// the Hadamard over the group's lanes.  The levels run in sequence, separated by workgroup barriers; everything a level hands to the next
// lives in LDS:
//   0. lanes 0..84 form the predictor of every node of the CTU from the input field (global memory: the neighbours may lie in other
//      CTUs) and the clamped input vectors; the groups score their own vector: D(b, in(b)) and Best of the level-0 nodes;
//   k = 1..3, per level:
//   1. for every index c of the walk (4 children x (2r + 1)^2), the group scores its block under candidate c of ITS node of level k
//      and parks D in cand[c][block] -- no barrier between candidates, a slot is its group's own.  The candidates of one child and one
//      dx differ in dy alone: their whole-sample rows are one apart at most, so ONE horizontal pass over 16 window rows (a row per lane)
//      serves all of them and only the vertical stage and the Hadamard run per candidate: 12 horizontal passes per level at r = 1, not 36;
//   2. one lane per (node, c) sums the node's blocks and adds the rate: Jw(node, c);
//   3. one lane per node takes the least Jw, the first of equal ones: W(node), and writes the node's d_nodes record;
//   4. the groups keep D(b, W(node)) of their block: what d_out holds if the node becomes a partition.
//   Then the decision, bottom up, one lane per node and a barrier per level; lane 0 writes the CTU's record, lanes 0..63 the blocks'.
// A block outside the frame (a cut CTU) and a block of a node that is not whole still run every pass, on a block clamped into the frame
// and on its own vector, so that every barrier and every cross-lane step sees whole waves; what they compute is never read.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "x266_device.hpp"
#include "x266_interp.hpp"
#include "x266_part.hpp"
#include "x266_subpel_blocks.hpp"

namespace x266 {
namespace {

constexpr unsigned kPartThreads = 1024;                                     // 64 groups of 16 lanes: one per 8x8 block of a CTU
constexpr int kPartBlocks = 64;
constexpr int kPartMaxCand = 4 * (2 * kPartMaxRange + 1) * (2 * kPartMaxRange + 1);
constexpr int kPartNodes = 64 + 16 + 4 + 1;                                 // the nodes of a CTU, level 0 first

__device__ __forceinline__ int part_side(int k) { return 8 >> k; }          // nodes of level k along a CTU's side
__device__ __forceinline__ int part_first(int k) { return k == 0 ? 0 : k == 1 ? 64 : k == 2 ? 80 : 84; }
__device__ __forceinline__ uint32_t part_pack(PartVec v) { return (uint32_t)(uint16_t)v.x | (uint32_t)(uint16_t)v.y << 16; }
__device__ __forceinline__ PartVec part_unpack(uint32_t w) { return PartVec{(int)(int16_t)(w & 0xFFFFu), (int)(int16_t)(w >> 16)}; }

struct PartBest {
    uint32_t j, dist, bits, parts;
};

struct PartShared {
    v4i slot[kPartBlocks][16];                  // per group: 16 window rows of 8 int16 sums
    uint32_t cand[kPartMaxCand][kPartBlocks];   // D(block, candidate c of its node) at the running level
    uint32_t jcand[16][kPartMaxCand];           // Jw(node, c) at the running level
    uint32_t dlev[kPartLevels][kPartBlocks];    // D(block, W(its node of level k))
    uint32_t w[kPartNodes];                     // W(node), packed
    PartVec pred[kPartNodes];
    uint32_t jw[kPartNodes], rate[kPartNodes], cwin[kPartNodes], merged[kPartNodes];
    PartBest best[kPartNodes];
};

struct PartParams {
    const x266_ref_block_t *cur, *ref;
    const x266_me_result_t *mv;
    x266_me_result_t *out, *nodes;
    uint8_t *level;
    x266_part_ctu_t *ctu;
    int width, height, range, lambda;
    int bw, bh, ctus_x;
};

// candidate c of the node (nlx, nly) of level k: W of the child the walk names, moved by (dx, dy)
__device__ __forceinline__ PartVec part_candidate(const PartShared &s, int k, int nlx, int nly, int c, int r)
{
    const PartStep st = part_walk_step(c, r);
    const PartVec v = part_unpack(s.w[part_first(k - 1) + (2 * nly + (st.child >> 1)) * part_side(k - 1) + 2 * nlx + (st.child & 1)]);
    return PartVec{part_clamp_cand(v.x + st.dx), part_clamp_cand(v.y + st.dy)};
}

__global__ __launch_bounds__(kPartThreads) void partition_decide_kernel(const PartParams P)
{
    __shared__ __attribute__((aligned(16))) PartShared s;
    const int tid = (int)threadIdx.x, g = tid >> 4, l = tid & 15;
    const int cy = (int)blockIdx.x / P.ctus_x, cx = (int)blockIdx.x - cy * P.ctus_x;
    const int bw = P.bw, bh = P.bh, tiles_x = P.width >> 4, r = P.range, span = 2 * r + 1, ncand = part_walk_length(r);

    if (tid < kPartNodes) {                                                 // 0. predictors, input vectors
        const int k = tid < 64 ? 0 : tid < 80 ? 1 : tid < 84 ? 2 : 3, i = tid - part_first(k);
        const int X = (cx * 8) + ((i % part_side(k)) << k), Y = (cy * 8) + ((i / part_side(k)) << k);
        const bool exists = X < bw && Y < bh;
        s.pred[tid] = exists ? part_predictor(P.mv, bw, X, Y, 1 << k) : PartVec{0, 0};
        s.merged[tid] = 0;
        s.best[tid] = PartBest{0, 0, 0, 0};
        if (k == 0) s.w[tid] = part_pack(part_in(P.mv, bw, X < bw ? X : bw - 1, Y < bh ? Y : bh - 1));
    }

    const int gx = g & 7, gy = g >> 3;
    const bool live = cx * 8 + gx < bw && cy * 8 + gy < bh;
    const int bx = cx * 8 + gx < bw ? cx * 8 + gx : bw - 1, by = cy * 8 + gy < bh ? cy * 8 + gy : bh - 1;   // clamped into the frame
    const int tx = bx >> 1, ty = by >> 1, blk = (by & 1) * 2 + (bx & 1);
    const uint32_t cw = cur_block_word(P.cur + (size_t)ty * (size_t)tiles_x + (size_t)tx, blk, l);
    v4i *slot = s.slot[g];

    // The two stages of D(block, q), apart: candidates that differ in dy alone share the horizontal sums.  hstage forms the sums of the 16
    // window rows from whole-sample row iy - 3 on under the horizontal component qx, a row per lane; vstage scores the vertical phase fy
    // from slot row `down` (0, or 1 where the candidate's whole-sample row is iy + 1) on: D(block, q) in every lane of the group.
    auto hstage = [&](int qx, int iy) {
        x266_me_result_t rec;
        rec.mvx = (int16_t)qx;
        rec.mvy = (int16_t)(iy * 4);
        rec.cost = 0;
        const WindowRow<false> src = window_row<false>(P.ref, rec, P.height, tiles_x, tx, ty, blk, l);
        uint32_t win[4];
        load_window_row<false>(src.row, src.xs, P.width, win);
        int t[8], h[8];
        interp_taps<false>(src.fx, t);
        interp_hsums<false>(win, t, h);
        slot[l] = pack_hsums(h);
        wave_lds_sync();
    };
    auto vstage = [&](int down, int fy) -> uint32_t {
        int v[4], d[4];
        vertical_v4<false>(slot + down, fy, l, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) d[c] = (int)((cw >> (8 * c)) & 255u) - interp_round(v[c]);
        return satd8x8_group16(d, l);
    };

    __syncthreads();
    {
        const PartVec q = part_unpack(s.w[g]);
        hstage(q.x, q.y >> 2);
        const uint32_t dist = vstage(0, q.y & 3);
        wave_lds_sync();                                                    // the next pass overwrites the slot
        if (l == 0 && live) {
            const uint32_t bits = part_rate(0, q.x, q.y, s.pred[g]);
            s.dlev[0][g] = dist;
            s.best[g] = PartBest{dist + part_rate_cost(P.lambda, bits), dist, bits, 1};
        }
    }

    for (int k = 1; k < kPartLevels; ++k) {
        const int side = part_side(k), first = part_first(k);
        const int nlx = gx >> k, nly = gy >> k;
        const bool whole = part_whole(bw, bh, k, cx * side + nlx, cy * side + nly);
        __syncthreads();                                                    // W of level k - 1 is complete, cand[] is free
        for (int child = 0; child < 4; ++child) {                           // 1. walk index c = (child * span + dy + r) * span + dx + r
            const PartVec v = part_unpack(s.w[whole ? part_first(k - 1) + (2 * nly + (child >> 1)) * part_side(k - 1) + 2 * nlx + (child & 1) : g]);
            const int iy = part_clamp_cand(v.y - r) >> 2;                   // the clamp keeps the order: the rows of dy = -r..r are iy or iy + 1
            for (int dxi = 0; dxi < span; ++dxi) {
                hstage(part_clamp_cand(v.x + dxi - r), iy);
                for (int dyi = 0; dyi < span; ++dyi) {
                    const int qy = part_clamp_cand(v.y + dyi - r);
                    const uint32_t dist = vstage((qy >> 2) - iy, qy & 3);
                    if (l == 0) s.cand[(child * span + dyi) * span + dxi][g] = dist;
                }
                wave_lds_sync();                                            // the next pass overwrites the slot
            }
        }
        __syncthreads();
        if (tid < side * side * ncand) {                                    // 2.
            const int node = tid / ncand, c = tid - node * ncand, mx = node % side, my = node / side;
            if (part_whole(bw, bh, k, cx * side + mx, cy * side + my)) {
                uint32_t sum = 0;
                for (int y = 0; y < (1 << k); ++y)
                    for (int x = 0; x < (1 << k); ++x) sum += s.cand[c][((my << k) + y) * 8 + (mx << k) + x];
                const PartVec q = part_candidate(s, k, mx, my, c, r);
                s.jcand[node][c] = sum + part_rate_cost(P.lambda, part_rate(k, q.x, q.y, s.pred[first + node]));
            }
        }
        __syncthreads();
        if (tid < side * side) {                                            // 3.
            const int mx = tid % side, my = tid / side, nx = cx * side + mx, ny = cy * side + my;
            if (part_whole(bw, bh, k, nx, ny)) {
                uint32_t least = s.jcand[tid][0];
                int win = 0;
                for (int c = 1; c < ncand; ++c) {
                    const uint32_t j = s.jcand[tid][c];
                    if (j < least) { least = j; win = c; }
                }
                const PartVec q = part_candidate(s, k, mx, my, win, r);
                s.w[first + tid] = part_pack(q);                            // level k: no lane of this step reads it
                s.jw[first + tid] = least;
                s.rate[first + tid] = part_rate(k, q.x, q.y, s.pred[first + tid]);
                s.cwin[first + tid] = (uint32_t)win;
                if (P.nodes) {
                    const size_t at = part_nodes_offset(bw, bh, k) + (size_t)ny * (size_t)part_whole_w(bw, k) + (size_t)nx;
                    *reinterpret_cast<uint2 *>(P.nodes + at) = make_uint2(part_pack(q), least);
                }
            }
        }
        __syncthreads();
        if (l == 0 && whole) s.dlev[k][g] = s.cand[s.cwin[first + nly * side + nlx]][g];                    // 4.
    }

    for (int k = 1; k < kPartLevels; ++k) {                                 // the decision, bottom up
        const int side = part_side(k), first = part_first(k), below = part_first(k - 1);
        __syncthreads();
        if (tid < side * side) {
            const int mx = tid % side, my = tid / side;
            PartBest sum = {0, 0, 0, 0};                                    // a child outside the frame holds zeros
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const PartBest b = s.best[below + (2 * my + (ch >> 1)) * (2 * side) + 2 * mx + (ch & 1)];
                sum.j += b.j;
                sum.dist += b.dist;
                sum.bits += b.bits;
                sum.parts += b.parts;
            }
            if (part_whole(bw, bh, k, cx * side + mx, cy * side + my)) {
                const uint32_t split = sum.j + part_rate_cost(P.lambda, 1), jw = s.jw[first + tid], bits = s.rate[first + tid];
                if (jw <= split) {                                          // a tie merges
                    sum = PartBest{jw, jw - part_rate_cost(P.lambda, bits), bits, 1};
                    s.merged[first + tid] = 1;
                } else {
                    sum.j = split;
                    sum.bits += 1;
                }
            }                                                               // a cut node: the sum of its existing children, no flag
            s.best[first + tid] = sum;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const PartBest b = s.best[part_first(3)];
        x266_part_ctu_t rec;
        rec.j = b.j;
        rec.dist = b.dist;
        rec.bits = b.bits;
        rec.parts = b.parts;
        P.ctu[blockIdx.x] = rec;
    }
    if (tid < kPartBlocks) {
        const int ox = tid & 7, oy = tid >> 3, fx = cx * 8 + ox, fy = cy * 8 + oy;
        if (fx < bw && fy < bh) {
            int level = 0;
#pragma unroll
            for (int k = 1; k < kPartLevels; ++k)
                if (s.merged[part_first(k) + (oy >> k) * part_side(k) + (ox >> k)]) level = k;
            const size_t b = (size_t)fy * (size_t)bw + (size_t)fx;
            *reinterpret_cast<uint2 *>(P.out + b) = make_uint2(s.w[part_first(level) + (oy >> level) * part_side(level) + (ox >> level)], s.dlev[level][tid]);
            P.level[b] = (uint8_t)level;
        }
    }
}

}  // namespace

hipError_t launch_partition_decide(const x266_part_t &p, hipStream_t stream)
{
    PartParams P;
    P.cur = p.d_cur;
    P.ref = p.d_ref;
    P.mv = p.d_mv;
    P.out = p.d_out;
    P.nodes = p.d_nodes;
    P.level = p.d_level;
    P.ctu = p.d_ctu;
    P.width = p.width; P.height = p.height; P.range = p.range; P.lambda = p.lambda_q4;
    P.bw = p.width / 8;
    P.bh = p.height / 8;
    P.ctus_x = (p.width + 63) / 64;
    const size_t n_ctu = (size_t)P.ctus_x * (size_t)((p.height + 63) / 64);
    if (n_ctu == 0) return hipSuccess;
    unsigned wgs;
    if (hipError_t e = wave_grid(n_ctu, 1, &wgs)) return e;
    hipLaunchKernelGGL(partition_decide_kernel, dim3(wgs), dim3(kPartThreads), 0, stream, P);
    return hipGetLastError();
}

}  // namespace x266
