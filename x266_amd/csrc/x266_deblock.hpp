// x266_deblock.hpp -- the in-loop deblocking filter of include/x266hip.h (xDeblockLumaGpu / ChromaGpu / Gpu): the tables, the
// boundary strength and parameter derivation of an edge, and the per-line filters, in ONE copy that the three kernels of
// deblock_kernels.hip and both edge directions share -- "the fused call is bit-identical to the pair" holds by construction.
//
// The arithmetic is HEVC's deblocking filter at 8-bit depth as recalled, unverified offline; the header's text is the contract.
// What the code below relies on:
//   * neither table is in memory: BETA is 0 below index 16, index - 10 up to 28, 2 index - 38 from 29 on, and TC is seven runs
//     and three linear stretches (deblock_tc) -- tests/_deblock_ref.py holds both tables as lists;
//   * every intermediate fits comfortably in 32 bits (samples 0..255, tc <= 24, beta <= 64);
//   * the strong filter's results are averages of samples, so after the +-2 tc clamp around a sample they need no clip8;
//   * a chroma edge that is not filtered has tc 0 in its packed parameters, and tc = 0 clamps D to 0: one code path.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"

namespace x266 {

// the side information of a call as the kernels take it (x266_deblock_t plus the frame's geometry)
struct DeblockSide {
    const uint8_t *cls, *intra, *qps;
    const uint32_t *nnz;
    const x266_me_result_t *mv;
    int qp, beta_off, tc_off;       // the offsets already doubled
    int width, height, tiles_x, ctus_x;
};

__device__ __forceinline__ int deblock_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int deblock_abs(int v) { return v < 0 ? -v : v; }
__device__ __forceinline__ int deblock_beta(int index) { return index < 16 ? 0 : (index < 29 ? index - 10 : 2 * index - 38); }
// TC[index] for index 0..53 in closed form (the runs of the table, then its three linear stretches): no dependent table load
__device__ __forceinline__ int deblock_tc(int index)
{
    return index < 18 ? 0 : index < 27 ? 1 : index < 31 ? 2 : index < 35 ? 3 : index < 38 ? 4 : index < 40 ? 5 : index < 42 ? 6 :
           index < 47 ? index - 35 : index < 49 ? index - 34 : 2 * index - 82;
}

// luma region 6 ctu + q of the 8x8 block (bx, by)
__device__ __forceinline__ size_t deblock_luma_region(const DeblockSide &s, int bx, int by)
{
    return ((size_t)(by >> 3) * (size_t)s.ctus_x + (size_t)(bx >> 3)) * 6 + (size_t)(((by >> 2) & 1) * 2 + ((bx >> 2) & 1));
}

// The packed parameters of the luma edge between the 8x8 blocks P = (pbx, pby) and Q = (qbx, qby), at sample coordinate `coord`
// (x of a vertical edge, y of a horizontal one): bs | tc << 2 | beta << 8; 0 when the edge is left alone.  Every entry the rules
// may look at is loaded up front -- no address depends on a loaded value, so the derivation costs one memory latency, not a chain.
__device__ __forceinline__ uint32_t deblock_luma_edge(const DeblockSide &s, int pbx, int pby, int qbx, int qby, int coord)
{
    const size_t rp = deblock_luma_region(s, pbx, pby), rq = deblock_luma_region(s, qbx, qby), blocks_x = (size_t)(s.width >> 3);
    const unsigned cls_q = s.cls ? s.cls[rq] : 3u;
    const unsigned intra_p = s.intra ? s.intra[rp] : 0u, intra_q = s.intra ? s.intra[rq] : 0u;
    const unsigned coded_p = s.nnz ? s.nnz[rp] : 1u, coded_q = s.nnz ? s.nnz[rq] : 1u;
    const int qp_p = s.qps ? (int)s.qps[rp] : s.qp, qp_q = s.qps ? (int)s.qps[rq] : s.qp;
    int mvx_p = 0, mvy_p = 0, mvx_q = 0, mvy_q = 0;
    if (s.mv) {
        const x266_me_result_t a = s.mv[(size_t)pby * blocks_x + (size_t)pbx], b = s.mv[(size_t)qby * blocks_x + (size_t)qbx];
        mvx_p = a.mvx, mvy_p = a.mvy, mvx_q = b.mvx, mvy_q = b.mvy;
    }
    const bool transform_edge = rp != rq || (coord & ((4 << (cls_q & 3u)) - 1)) == 0;
    const bool intra = (intra_p | intra_q) != 0;
    const int bs = transform_edge && intra ? 2 : transform_edge && (coded_p | coded_q) != 0 ? 1 :
                   !intra && (deblock_abs(mvx_p - mvx_q) >= 4 || deblock_abs(mvy_p - mvy_q) >= 4) ? 1 : 0;
    if (!bs) return 0;
    const int qp = ((qp_p < 51 ? qp_p : 51) + (qp_q < 51 ? qp_q : 51) + 1) >> 1;
    const int beta = deblock_beta(deblock_clamp(qp + s.beta_off, 0, 51));
    const int tc = deblock_tc(deblock_clamp(qp + 2 * (bs - 1) + s.tc_off, 0, 53));
    return (uint32_t)bs | (uint32_t)tc << 2 | (uint32_t)beta << 8;
}

// The packed parameters of the chroma edge between the tiles P = (ptx, pty) and Q = (qtx, qty), at chroma coordinate `coord`:
// tc of U | tc of V << 8, 0 for a plane whose edge is not filtered.  Loads up front, as above.
__device__ __forceinline__ uint32_t deblock_chroma_edge(const DeblockSide &s, int ptx, int pty, int qtx, int qty, int coord)
{
    const size_t cp = (size_t)(pty >> 2) * (size_t)s.ctus_x + (size_t)(ptx >> 2), cq = (size_t)(qty >> 2) * (size_t)s.ctus_x + (size_t)(qtx >> 2);
    if (!s.intra) return 0;
    const unsigned intra_p = s.intra[cp * 6 + (size_t)(((pty >> 1) & 1) * 2 + ((ptx >> 1) & 1))];
    const unsigned intra_q = s.intra[cq * 6 + (size_t)(((qty >> 1) & 1) * 2 + ((qtx >> 1) & 1))];
    unsigned cls_q[2];
    int qp_p[2], qp_q[2];
#pragma unroll
    for (int plane = 0; plane < 2; ++plane) {
        cls_q[plane] = s.cls ? s.cls[cq * 6 + 4 + (size_t)plane] : 3u;
        qp_p[plane] = s.qps ? (int)s.qps[cp * 6 + 4 + (size_t)plane] : s.qp;
        qp_q[plane] = s.qps ? (int)s.qps[cq * 6 + 4 + (size_t)plane] : s.qp;
    }
    if (!(intra_p | intra_q)) return 0;
    uint32_t packed = 0;
#pragma unroll
    for (int plane = 0; plane < 2; ++plane) {
        if (cp == cq && (coord & ((4 << (cls_q[plane] & 3u)) - 1)) != 0) continue;
        const int qp = ((qp_p[plane] < 51 ? qp_p[plane] : 51) + (qp_q[plane] < 51 ? qp_q[plane] : 51) + 1) >> 1;
        packed |= (uint32_t)deblock_tc(deblock_clamp(qp + 2 + s.tc_off, 0, 53)) << (8 * plane);
    }
    return packed;
}

// ---- luma lines -----------------------------------------------------------------------------------------------------------------
// A line's own decision terms, packed for the exchange inside its segment: dp | dq << 10 | (the line passes the three strong tests) << 20
__device__ __forceinline__ uint32_t deblock_line_terms(const int (&v)[8], int beta, int tc)
{
    const int dp = deblock_abs(v[1] - 2 * v[2] + v[3]), dq = deblock_abs(v[6] - 2 * v[5] + v[4]);
    const bool strong = 2 * (dp + dq) < (beta >> 2) && deblock_abs(v[0] - v[3]) + deblock_abs(v[4] - v[7]) < (beta >> 3) &&
                        deblock_abs(v[3] - v[4]) < ((5 * tc + 1) >> 1);
    return (uint32_t)dp | (uint32_t)dq << 10 | (uint32_t)strong << 20;
}

// One line p3 p2 p1 p0 | q0 q1 q2 q3 = v[0..7] of a segment, with the terms of the segment's lines 0 and 3.  Returns whether v changed
// (it is rewritten either way when the segment is on).
__device__ __forceinline__ bool deblock_luma_line(int (&v)[8], uint32_t t0, uint32_t t3, int beta, int tc)
{
    const int dp = (int)(t0 & 1023u) + (int)(t3 & 1023u), dq = (int)((t0 >> 10) & 1023u) + (int)((t3 >> 10) & 1023u);
    if (dp + dq >= beta) return false;
    const int p3 = v[0], p2 = v[1], p1 = v[2], p0 = v[3], q0 = v[4], q1 = v[5], q2 = v[6], q3 = v[7];
    if ((t0 & t3) >> 20 & 1u) {
        const int t2 = 2 * tc;
        v[3] = deblock_clamp((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, p0 - t2, p0 + t2);
        v[2] = deblock_clamp((p2 + p1 + p0 + q0 + 2) >> 2, p1 - t2, p1 + t2);
        v[1] = deblock_clamp((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3, p2 - t2, p2 + t2);
        v[4] = deblock_clamp((q2 + 2 * q1 + 2 * q0 + 2 * p0 + p1 + 4) >> 3, q0 - t2, q0 + t2);
        v[5] = deblock_clamp((q2 + q1 + q0 + p0 + 2) >> 2, q1 - t2, q1 + t2);
        v[6] = deblock_clamp((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3, q2 - t2, q2 + t2);
        return true;
    }
    int delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4;
    if (deblock_abs(delta) >= 10 * tc) return false;
    delta = deblock_clamp(delta, -tc, tc);
    const int side = (beta + (beta >> 1)) >> 3, h = tc >> 1;
    v[3] = deblock_clamp(p0 + delta, 0, 255);
    v[4] = deblock_clamp(q0 - delta, 0, 255);
    if (dp < side) v[2] = deblock_clamp(p1 + deblock_clamp((((p2 + p0 + 1) >> 1) - p1 + delta) >> 1, -h, h), 0, 255);
    if (dq < side) v[5] = deblock_clamp(q1 + deblock_clamp((((q2 + q0 + 1) >> 1) - q1 - delta) >> 1, -h, h), 0, 255);
    return true;
}

// ---- chroma lines ---------------------------------------------------------------------------------------------------------------
// p1 p0 | q0 q1 of one plane: the new p0 and q0
__device__ __forceinline__ void deblock_chroma_line(int p1, int &p0, int &q0, int q1, int tc)
{
    const int delta = deblock_clamp((((q0 - p0) << 2) + p1 - q1 + 4) >> 3, -tc, tc);
    p0 = deblock_clamp(p0 + delta, 0, 255);
    q0 = deblock_clamp(q0 - delta, 0, 255);
}

}  // namespace x266
