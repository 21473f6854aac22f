// x266_args.hpp -- the argument rules of the device entry points of include/x266hip.h, host-only: plain C++17, no HIP, no context.
//
// Every device entry point has one rule function here (calls with the same rules share one).  It takes the call's arguments
// and returns the reason the call is refused, or nullptr when it is accepted; it reads nothing through the pointers and touches
// no state, so tests/cpp/arg_rules_check.cpp -- one table with a row per entry point, one walk over it -- holds the rules of
// every one of them without a device.  x266hip_abi.hip turns a reason into X266HIP_EINVAL and the text
// "<entry point>: <reason>" and launches nothing.  A new entry point declares its rules here and adds a row there.  The calls whose
// device pointers are fields of a host-read struct -- the compact level stream (levels_pack, levels_unpack), the source analysis
// (aq_stats, aq_decide), the lookahead (la_*), the seeded search (seeded_search), the mixed inter / intra frame (mixed_code_frame), RDOQ
// and the level rate estimate (rdoq_regions, levels_bits) -- are held the same way by tests/cpp/struct_rules_check.cpp: one description
// per struct, one walk over every call of every one; a new struct call adds a row to its struct's description there, a new struct a
// description.  The transform decision (transform_decide, x266_tdecide_t) has a stand-alone driver of the same form,
// tests/cpp/tdecide_rules_check.cpp, and so have frame quality (quality_stats, x266_quality_t): tests/cpp/quality_rules_check.cpp, and the
// inter partition decision (partition_decide, x266_part_t): tests/cpp/partition_rules_check.cpp, the compact motion stream (motion_pack,
// motion_unpack, x266_motion_t): tests/cpp/motion_rules_check.cpp, and the entropy coder (entropy_encode, entropy_decode, x266_entropy_t):
// tests/cpp/entropy_rules_check.cpp, and the entropy coder of the motion stream (entropy_motion_encode, entropy_motion_decode,
// x266_entropy_motion_t; motion_reconstruct): tests/cpp/entropy_motion_rules_check.cpp, and the entropy coder of the side information
// (entropy_side_encode, entropy_side_decode, x266_entropy_side_t): tests/cpp/entropy_side_rules_check.cpp, and the bin statistics
// (entropy_stats_levels, entropy_stats_side, x266_entropy_stats_t, x266_entropy_side_stats_t): tests/cpp/entropy_stats_rules_check.cpp.
//
// A call's buffers are declared once (Buf) and walked by one checker: NULL, alignment, "does the span fit in the address
// space", "does an output overlap anything".  An extent of 0 means that the extent is not part of the call's rules today: the
// older calls check NULL and alignment only.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/x266hip.h"
#include "x266_part.hpp"
#include "x266_seed.hpp"

namespace x266 {
namespace args {

constexpr const char *kNull = "a required pointer is NULL";
constexpr const char *kMisaligned = "a pointer is misaligned";
constexpr const char *kNoFit = "a buffer does not fit in the address space";
constexpr const char *kOverlap = "an output overlaps another buffer";
constexpr const char *kQuantScalars = "qp must be 0..51 (without d_qp) and rounding 0..511";
constexpr const char *kChroma = "pitch < 1 or overlapping U / V outputs";

struct Buf {
    const char *name;
    const void *p;
    unsigned align;
    size_t bytes;                   // 0: no extent in this call's rules
    bool output, optional, fitted;  // fitted: the span's end is checked against the address space
    const char *same_as;            // an output may BE this input (the very same address), and must not overlap it otherwise
};
constexpr Buf in(const char *name, const void *p, unsigned align, size_t bytes = 0) { return {name, p, align, bytes, false, false, true, nullptr}; }
constexpr Buf out(const char *name, const void *p, unsigned align, size_t bytes = 0, const char *same_as = nullptr) { return {name, p, align, bytes, true, false, true, same_as}; }
constexpr Buf opt(Buf b) { b.optional = true; return b; }
constexpr Buf unfitted(Buf b) { b.fitted = false; return b; }    // overlap is tested, the span's end is not: the calls from before the quantiser

inline const char *check(const Buf *b, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!b[i].p && !b[i].optional) return kNull;
    for (size_t i = 0; i < n; ++i)
        if ((uintptr_t)b[i].p & (b[i].align - 1u)) return kMisaligned;
    for (size_t i = 0; i < n; ++i) {
        uintptr_t end = 0;
        if (b[i].p && b[i].fitted && __builtin_add_overflow((uintptr_t)b[i].p, b[i].bytes, &end)) return kNoFit;
    }
    for (size_t o = 0; o < n; ++o) {
        if (!b[o].output || !b[o].p || !b[o].bytes) continue;
        for (size_t i = 0; i < n; ++i) {
            if (i == o || !b[i].p || !b[i].bytes) continue;
            if (b[o].p == b[i].p && b[o].same_as && !std::strcmp(b[o].same_as, b[i].name)) continue;
            const uintptr_t x = (uintptr_t)b[o].p, y = (uintptr_t)b[i].p;
            if (x < y + b[i].bytes && y < x + b[o].bytes) return kOverlap;
        }
    }
    return nullptr;
}
template <size_t N> const char *check(const Buf (&b)[N]) { return check(b, N); }

// ---- extents: the checked arithmetic.  A product that wraps size_t saturates, and a saturated span fits behind no pointer.
inline size_t mul(size_t a, size_t b)
{
    size_t r = 0;
    return __builtin_mul_overflow(a, b, &r) ? SIZE_MAX : r;
}
// first byte of block 0 to the last byte of block n - 1 of a stream with a pitch of `pitch` blocks
inline size_t stream_bytes(size_t n_blocks, size_t pitch, size_t block_bytes)
{
    if (n_blocks == 0) return 0;
    const size_t t = mul(n_blocks - 1, pitch);
    return mul(t == SIZE_MAX ? t : t + 1, block_bytes);
}
inline size_t tile_bytes(int w, int h) { return (size_t)w * (size_t)h * 2; }                  // 512 bytes per 256 pixels
inline size_t blocks8(int w, int h) { return (size_t)(w / 8) * (size_t)(h / 8); }
inline size_t ctus(int w, int h) { return (((size_t)w + 63) / 64) * (((size_t)h + 63) / 64); }

// ---- frame sizes and scalar ranges
inline const char *frame(int w, int h, int granule)
{
    if (w > 0 && h > 0 && w % granule == 0 && h % granule == 0) return nullptr;
    return granule == 8 ? "width/height must be positive multiples of 8" : granule == 16 ? "width/height must be positive multiples of 16"
         : granule == 32 ? "width/height must be positive multiples of 32" : "width/height must be positive multiples of 64";
}
inline bool qp_ok(const void *d_qp, int qp) { return d_qp || (qp >= 0 && qp <= 51); }
inline bool rounding_ok(int rounding) { return rounding >= 0 && rounding <= 511; }
inline bool range_ok(int range) { return range >= 1 && range <= 64; }
inline bool offset_ok(int offset_div2) { return offset_div2 >= -6 && offset_div2 <= 6; }
inline bool lambda_ok(int lambda_q4) { return lambda_q4 >= 0 && lambda_q4 <= 65535; }
inline bool edge_8_or_32(int block_edge) { return block_edge == 8 || block_edge == 32; }

// the two output streams of a chroma call must not overlap: plane V starts at or after U's first block ends (interleaved
// form) or anywhere else outside [U, U + span)
inline bool chroma_outputs_ok(const void *u, const void *v, size_t block_bytes, size_t n_blocks, size_t pitch)
{
    if (!u || !v || pitch < 1 || n_blocks == 0) return u && v && pitch >= 1;
    const uintptr_t a = (uintptr_t)u, b = (uintptr_t)v;
    const uintptr_t lo = a < b ? a : b, hi = a < b ? b : a;
    const size_t gap = (size_t)(hi - lo);
    if (gap >= ((n_blocks - 1) * pitch + 1) * block_bytes) return true;     // disjoint spans
    // interleaved: the other plane's blocks sit in the holes of this one's pitch
    return pitch >= 2 && gap % block_bytes == 0 && gap / block_bytes >= 1 && gap / block_bytes <= pitch - 1;
}

// ---- the batch calls: NULL and alignment only, and n == 0 is accepted whatever the pointers are ------------------------------------
// xDct32FwdBatchDev, xDct32InvBatchDev, either half of xDct32SatdFrameDev, xSatd8x8BatchDev (out_align 4)
inline const char *batch(const void *d_in, const void *d_out, unsigned out_align, size_t n)
{
    const Buf b[] = {in("d_in", d_in, 16), out("d_out", d_out, out_align)};
    return n ? check(b) : nullptr;
}
inline const char *dct32_satd_frame(const void *d_dct_in, const void *d_dct_out, size_t n_dct, const void *d_diff, const void *d_satd_out, size_t n_satd)
{
    const char *why = batch(d_dct_in, d_dct_out, 16, n_dct);
    return why ? why : batch(d_diff, d_satd_out, 16, n_satd);
}
inline const char *dct32_pass(const void *d_in, const void *d_out, size_t n, int shift)
{
    return shift < 1 || shift > 15 ? "shift must be 1..15" : batch(d_in, d_out, 16, n);
}
inline const char *dct32_fwd_inv_batch(const void *d_in, const void *d_coef, const void *d_recon, size_t n)
{
    const Buf b[] = {in("d_in", d_in, 16), opt(out("d_coef", d_coef, 16)), out("d_recon", d_recon, 16)};
    return n ? check(b) : nullptr;
}
inline const char *mem_ceiling(int kind, const void *d_src, const void *d_dst, size_t bytes)
{
    if (kind < X266_MEM_COPY || kind > X266_MEM_READ_PROBE) return "kind must be X266_MEM_COPY, _READ, _WRITE or _READ_PROBE";
    if (bytes & 15u) return "bytes must be a multiple of 16";
    const Buf b[] = {out("d_dst", d_dst, 16), in("d_src", d_src, 16)};       // X266_MEM_WRITE reads nothing: d_src is not looked at
    return bytes ? check(b, kind == X266_MEM_WRITE ? 1 : 2) : nullptr;
}
inline const char *intra32_predict(const void *d_refs, const void *d_modes, const void *d_ref_index, const void *d_pred, size_t n)
{
    const Buf b[] = {in("d_refs", d_refs, 16), in("d_modes", d_modes, 1), opt(in("d_ref_index", d_ref_index, 4)), out("d_pred", d_pred, 16)};
    return n ? check(b) : nullptr;
}
inline const char *intra32_residual_dct32(const void *d_refs, const void *d_modes, const void *d_ref_index, const void *d_src, const void *d_coef, size_t n)
{
    const Buf b[] = {in("d_refs", d_refs, 16), in("d_modes", d_modes, 1), opt(in("d_ref_index", d_ref_index, 4)), in("d_src", d_src, 16), out("d_coef", d_coef, 16)};
    return n ? check(b) : nullptr;
}
inline const char *intra32_costs(const void *d_refs, const void *d_src, const void *d_costs, const void *d_best_mode, size_t n)
{
    const Buf b[] = {in("d_refs", d_refs, 16), in("d_src", d_src, 16), out("d_costs", d_costs, 4), opt(out("d_best_mode", d_best_mode, 1))};
    return n ? check(b) : nullptr;
}
inline const char *fill_residual(const void *d_dst, size_t n_samples)
{
    const Buf b[] = {out("d_dst", d_dst, 16)};
    return n_samples ? check(b) : nullptr;
}
constexpr int kTransformTypes = 4;                  // DCT-II, DST-VII, and the two mixed horizontal / vertical pairs
// xTransformFwdBatchDev, xTransformInvBatchDev
inline const char *transform_batch(int type, int size, const void *d_in, const void *d_out, size_t n, const void *d_offsets)
{
    if (type < 0 || type >= kTransformTypes) return "unknown transform type";
    if (size != 4 && size != 8 && size != 16 && !(size == 32 && type == X266_TR_DCT2)) return "size must be 4, 8, 16 (or 32 for DCT-II)";
    const Buf b[] = {in("d_in", d_in, 16), out("d_out", d_out, 16), opt(in("d_offsets", d_offsets, 4))};
    return n ? check(b) : nullptr;
}
inline const char *transform_tiles(const void *d_in, const void *d_out, size_t n_tiles, const void *d_tile_offsets, const void *d_tile_class)
{
    const Buf b[] = {in("d_in", d_in, 16), out("d_out", d_out, 16), opt(in("d_tile_offsets", d_tile_offsets, 4)), in("d_tile_class", d_tile_class, 1)};
    return n_tiles ? check(b) : nullptr;
}
inline const char *sad_batch(int edge, const void *d_a, const void *d_b, const void *d_out, size_t n)
{
    if (edge != 4 && edge != 8 && edge != 16 && edge != 32 && edge != 64) return "edge must be 4, 8, 16, 32 or 64";
    const Buf b[] = {in("d_a", d_a, 16), in("d_b", d_b, 16), out("d_out", d_out, 4)};
    return n ? check(b) : nullptr;
}

// ---- planar frames <-> tiles, and the calls from tiles: NULL and alignment only ----------------------------------------------------
// xConvInputFmtDev (to_tiles: the planes are the inputs, strdC is not an argument) and xConvOutput420Dev
inline const char *tile_convert(bool to_tiles, const void *d_tiles, const void *d_y, const void *d_u, const void *d_v, intptr_t strdY, intptr_t strdC, int w, int h)
{
    if (const char *why = frame(w, h, 16)) return why;
    if (strdY < w || (strdY & 15) || (!to_tiles && (strdC < w / 2 || (strdC & 7)))) return "a stride is too small or misaligned";
    Buf b[] = {in("d_tiles", d_tiles, 16), in("d_y", d_y, 16), in("d_u", d_u, 8), in("d_v", d_v, 8)};
    for (Buf &x : b) x.output = to_tiles == (&x == b);
    return check(b);
}
inline const char *residual_luma(const void *d_cur, const void *d_pred, int w, int h, int block_edge, const void *d_residual)
{
    if (!edge_8_or_32(block_edge)) return "block_edge must be 8 or 32";
    if (const char *why = frame(w, h, block_edge == 32 ? 32 : 16)) return why;
    const Buf b[] = {in("d_cur", d_cur, 16), in("d_pred", d_pred, 16), out("d_residual", d_residual, 16)};
    return check(b);
}
// xDct32FwdFromTilesDev (granule 32), xSatd8x8FromTilesDev (16, out_align 4), xDct32FwdCtuFromTilesDev (64)
inline const char *from_tiles(const void *d_cur, const void *d_pred, int w, int h, int granule, const void *d_out, unsigned out_align)
{
    if (const char *why = frame(w, h, granule)) return why;
    const Buf b[] = {in("d_cur", d_cur, 16), in("d_pred", d_pred, 16), out("d_out", d_out, out_align)};
    return check(b);
}
// xResidualChromaDev (block_edge 8 or 32), xDct32FwdChromaFromTilesDev (32, 16-byte outputs), xSatd8x8ChromaFromTilesDev (block_edge 8: one
// 4-byte sum per 8x8 chroma block); the luma frame of a 32x32 chroma block is a 64x64 CTU's
inline const char *chroma_from_tiles(const void *d_cur, const void *d_pred, int w, int h, int block_edge, const void *d_u, const void *d_v, unsigned out_align,
                                     size_t block_bytes, size_t pitch)
{
    if (!edge_8_or_32(block_edge)) return "block_edge must be 8 or 32";
    if (const char *why = frame(w, h, block_edge == 32 ? 64 : 16)) return why;
    const Buf b[] = {in("d_cur", d_cur, 16), in("d_pred", d_pred, 16), out("d_u", d_u, out_align), out("d_v", d_v, out_align)};
    if (const char *why = check(b)) return why;
    return chroma_outputs_ok(d_u, d_v, block_bytes, (size_t)(w / 2 / block_edge) * (size_t)(h / 2 / block_edge), pitch) ? nullptr : kChroma;
}

// ---- reconstruction into tiles: the output may BE the prediction, and must not overlap an input otherwise --------------------------
inline const char *recon_luma(const void *d_pred, const void *d_residual, int w, int h, int block_edge, const void *d_recon)
{
    if (!edge_8_or_32(block_edge)) return "block_edge must be 8 or 32";
    if (const char *why = frame(w, h, block_edge == 32 ? 32 : 16)) return why;
    const Buf b[] = {unfitted(in("d_pred", d_pred, 16, tile_bytes(w, h))), unfitted(in("d_residual", d_residual, 16, tile_bytes(w, h))),
                     unfitted(out("d_recon", d_recon, 16, tile_bytes(w, h), "d_pred"))};
    return check(b);
}
inline const char *recon_chroma(const void *d_pred, const void *d_res_u, const void *d_res_v, size_t pitch, int w, int h, int block_edge, const void *d_recon)
{
    if (!edge_8_or_32(block_edge)) return "block_edge must be 8 or 32";
    if (const char *why = frame(w, h, block_edge == 32 ? 64 : 16)) return why;
    if (pitch < 1) return "block_pitch < 1";
    const size_t span = stream_bytes((size_t)(w / 2 / block_edge) * (size_t)(h / 2 / block_edge), pitch, (size_t)block_edge * block_edge * 2);
    const Buf b[] = {unfitted(in("d_pred", d_pred, 16, tile_bytes(w, h))), in("d_res_u", d_res_u, 16, span), in("d_res_v", d_res_v, 16, span),
                     unfitted(out("d_recon", d_recon, 16, tile_bytes(w, h), "d_pred"))};
    return check(b);
}
// xDct32InvToTilesDev (granule 32: as many bytes of coefficients as of tiles), xDct32InvCtuToTilesDev (64: 12 KiB per CTU)
inline const char *inv_to_tiles(const void *d_coef, const void *d_pred, int w, int h, int granule, const void *d_recon)
{
    if (const char *why = frame(w, h, granule)) return why;
    const Buf b[] = {unfitted(in("d_coef", d_coef, 16, granule == 64 ? ctus(w, h) * 12288 : tile_bytes(w, h))), unfitted(in("d_pred", d_pred, 16, tile_bytes(w, h))),
                     unfitted(out("d_recon", d_recon, 16, tile_bytes(w, h), "d_pred"))};
    return check(b);
}

// ---- the mixed transform set per CTU, the quantiser, the fused CTU coding call -----------------------------------------------------
inline const char *transform_ctu_from_tiles(const void *d_cur, const void *d_pred, int w, int h, const void *d_class, const void *d_coef)
{
    if (const char *why = frame(w, h, 16)) return why;
    const Buf b[] = {in("d_cur", d_cur, 16, tile_bytes(w, h)), in("d_pred", d_pred, 16, tile_bytes(w, h)), in("d_class", d_class, 1, ctus(w, h) * 6),
                     out("d_coef", d_coef, 16, ctus(w, h) * 12288)};
    return check(b);
}
inline const char *transform_ctu_to_tiles(const void *d_coef, const void *d_class, const void *d_pred, int w, int h, const void *d_recon)
{
    if (const char *why = frame(w, h, 16)) return why;
    const Buf b[] = {in("d_coef", d_coef, 16, ctus(w, h) * 12288), in("d_class", d_class, 1, ctus(w, h) * 6), in("d_pred", d_pred, 16, tile_bytes(w, h)),
                     out("d_recon", d_recon, 16, tile_bytes(w, h), "d_pred")};
    return check(b);
}
// scalar errors first; the entry point then accepts n_regions == 0 whatever the pointers are
inline const char *quant_regions(int inverse, const void *d_in, const void *d_out, size_t n_regions, const void *d_class, const void *d_qp, int qp, int rounding,
                                 const void *d_nnz)
{
    if (!qp_ok(d_qp, qp) || !rounding_ok(rounding)) return kQuantScalars;
    if (inverse && d_nnz) return "d_nnz must be NULL with inverse = 1";
    const Buf b[] = {in("d_in", d_in, 16, mul(n_regions, 2048)), out("d_out", d_out, 16, mul(n_regions, 2048), "d_in"), opt(in("d_class", d_class, 1, n_regions)),
                     opt(in("d_qp", d_qp, 1, n_regions)), opt(out("d_nnz", d_nnz, 4, mul(n_regions, 4)))};
    return n_regions ? check(b) : nullptr;
}
inline const char *dct32_code_ctu_tiles(const void *d_cur, const void *d_pred, int w, int h, const void *d_qp, int qp, int rounding, const void *d_level,
                                        const void *d_nnz, const void *d_recon)
{
    if (const char *why = frame(w, h, 64)) return why;
    if (!qp_ok(d_qp, qp) || !rounding_ok(rounding)) return kQuantScalars;
    const Buf b[] = {in("d_pred", d_pred, 16, tile_bytes(w, h)), opt(in("d_qp", d_qp, 1, ctus(w, h) * 6)), out("d_level", d_level, 16, ctus(w, h) * 12288),
                     opt(out("d_nnz", d_nnz, 4, ctus(w, h) * 24)), out("d_recon", d_recon, 16, tile_bytes(w, h), "d_pred"), in("d_cur", d_cur, 16, tile_bytes(w, h))};
    return check(b, d_cur == d_pred ? 5 : 6);                              // one frame given as both inputs is one buffer
}

// ---- motion search and compensation ------------------------------------------------------------------------------------------------
// xSatd8x8SearchDev and xSad8x8SearchDev (sad: the current frame is read four bytes at a time) on planar frames: NULL and alignment only
inline const char *plane_search(bool sad, const void *d_cur, intptr_t cur_stride, const void *d_ref, intptr_t ref_stride, int w, int h, int range,
                                const void *d_best, const void *d_costs)
{
    if (const char *why = frame(w, h, 8)) return why;
    if (!range_ok(range)) return "range must be 1..64";
    if (cur_stride < w || ref_stride < (intptr_t)w + 2 * range) return "stride too small";
    if (sad && (cur_stride & 3)) return "the current frame's stride must be a multiple of 4";
    const Buf b[] = {in("d_cur", d_cur, sad ? 4 : 1), in("d_ref", d_ref, 1), out("d_best", d_best, 8), opt(out("d_costs", d_costs, 4))};
    return check(b);
}
// xSatd8x8SearchFromTilesDev, xSad8x8SearchFromTilesDev.  The inputs are read-only, so d_cur == d_ref is fine.  Each output is held against
// the two frames, not against the other output, and only the cost map's end against the address space: two lists.
inline const char *tile_search(const void *d_cur, const void *d_ref, int w, int h, int range, const void *d_best, const void *d_costs)
{
    if (const char *why = frame(w, h, 16)) return why;
    if (!range_ok(range)) return "range must be 1..64";
    const size_t span = (size_t)(2 * range + 1);
    const Buf best[] = {unfitted(in("d_cur", d_cur, 16, tile_bytes(w, h))), unfitted(in("d_ref", d_ref, 16, tile_bytes(w, h))),
                        unfitted(out("d_best", d_best, 8, blocks8(w, h) * 8))};
    const Buf costs[] = {best[0], best[1], opt(out("d_costs", d_costs, 4, mul(blocks8(w, h), span * span * 4)))};
    const char *why = check(best);
    return why ? why : check(costs);
}
// xMotionComp{,Luma,Chroma}Dev, and xMotionCompQpel{,Luma,Chroma}Gpu (fitted: a span must not run past the end of the address space)
inline const char *motion_comp(bool fitted, const void *d_ref, const void *d_mv, int w, int h, const void *d_pred)
{
    if (const char *why = frame(w, h, 16)) return why;
    Buf b[] = {in("d_ref", d_ref, 16, tile_bytes(w, h)), in("d_mv", d_mv, 8, blocks8(w, h) * 8), out("d_pred", d_pred, 16, tile_bytes(w, h))};
    for (Buf &x : b) x.fitted = fitted;
    return check(b);
}
inline const char *refine_qpel(const void *d_cur, const void *d_ref, int w, int h, const void *d_int, const void *d_best, const void *d_costs)
{
    if (const char *why = frame(w, h, 16)) return why;
    const Buf b[] = {in("d_cur", d_cur, 16, tile_bytes(w, h)), in("d_ref", d_ref, 16, tile_bytes(w, h)), in("d_int", d_int, 8, blocks8(w, h) * 8),
                     out("d_best", d_best, 8, blocks8(w, h) * 8, "d_int"), opt(out("d_costs", d_costs, 4, blocks8(w, h) * 49 * 4))};   // n_blocks < 2^56: no product wraps
    return check(b);
}

// the three bi-directional calls: wp NULL is the default, otherwise every field is held to its range
constexpr const char *kWp = "a wp field is out of range (w, o -128..127, log2_denom 0..7)";
inline bool wp_ok(const x266_wp_t *wp)
{
    if (!wp) return true;
    for (int l = 0; l < 2; ++l)
        for (int c = 0; c < 3; ++c)
            if (wp->w[l][c] < -128 || wp->w[l][c] > 127 || wp->o[l][c] < -128 || wp->o[l][c] > 127) return false;
    return wp->log2_denom[0] <= 7 && wp->log2_denom[1] <= 7;
}
// xMotionCompBiQpelTiles: the two references are read-only and may be one frame
inline const char *mc_bi_qpel(const void *d_ref0, const void *d_ref1, const void *d_mv0, const void *d_mv1, const void *d_dir, const x266_wp_t *wp, int planes,
                              int w, int h, const void *d_pred)
{
    if (const char *why = frame(w, h, 16)) return why;
    if (planes < 1 || planes > 3) return "planes must be 1, 2 or 3";
    if (!wp_ok(wp)) return kWp;
    const Buf b[] = {in("d_ref0", d_ref0, 16, tile_bytes(w, h)), in("d_ref1", d_ref1, 16, tile_bytes(w, h)), in("d_mv0", d_mv0, 8, blocks8(w, h) * 8),
                     in("d_mv1", d_mv1, 8, blocks8(w, h) * 8), opt(in("d_dir", d_dir, 1, blocks8(w, h))), out("d_pred", d_pred, 16, tile_bytes(w, h))};
    return check(b);
}
// xSatd8x8BiCostsFromTiles: either output may be NULL, not both
inline const char *bi_costs(const void *d_cur, const void *d_ref0, const void *d_ref1, int w, int h, const void *d_mv0, const void *d_mv1, const x266_wp_t *wp,
                            int bi_penalty, const void *d_costs, const void *d_dir)
{
    if (const char *why = frame(w, h, 16)) return why;
    if (bi_penalty < 0 || bi_penalty > 65535) return "bi_penalty must be 0..65535";
    if (!wp_ok(wp)) return kWp;
    if (!d_costs && !d_dir) return "d_costs and d_dir are both NULL";
    const Buf b[] = {in("d_cur", d_cur, 16, tile_bytes(w, h)), in("d_ref0", d_ref0, 16, tile_bytes(w, h)), in("d_ref1", d_ref1, 16, tile_bytes(w, h)),
                     in("d_mv0", d_mv0, 8, blocks8(w, h) * 8), in("d_mv1", d_mv1, 8, blocks8(w, h) * 8),
                     opt(out("d_costs", d_costs, 4, blocks8(w, h) * 12)), opt(out("d_dir", d_dir, 1, blocks8(w, h)))};
    return check(b);
}
// xSatd8x8RefineBiQpelFromTiles
inline const char *refine_bi_qpel(const void *d_cur, const void *d_ref_fix, const void *d_mv_fix, const void *d_ref, const void *d_int, int list,
                                  const x266_wp_t *wp, int w, int h, const void *d_best, const void *d_costs)
{
    if (const char *why = frame(w, h, 16)) return why;
    if (list < 0 || list > 1) return "list must be 0 or 1";
    if (!wp_ok(wp)) return kWp;
    const Buf b[] = {in("d_cur", d_cur, 16, tile_bytes(w, h)), in("d_ref_fix", d_ref_fix, 16, tile_bytes(w, h)), in("d_mv_fix", d_mv_fix, 8, blocks8(w, h) * 8),
                     in("d_ref", d_ref, 16, tile_bytes(w, h)), in("d_int", d_int, 8, blocks8(w, h) * 8),
                     out("d_best", d_best, 8, blocks8(w, h) * 8, "d_int"), opt(out("d_costs", d_costs, 4, blocks8(w, h) * 49 * 4))};
    return check(b);
}

// ---- the in-loop filters -----------------------------------------------------------------------------------------------------------
// xDeblockLumaGpu, xDeblockChromaGpu, xDeblockGpu
inline const char *deblock(const void *d_in, int w, int h, const x266_deblock_t *p, const void *d_out)
{
    if (!p) return "NULL parameter struct";
    if (const char *why = frame(w, h, 16)) return why;
    if (!qp_ok(p->d_qp, p->qp) || !offset_ok(p->beta_offset_div2) || !offset_ok(p->tc_offset_div2)) return "qp must be 0..51 (without d_qp) and the offsets -6..6";
    const size_t tab = ctus(w, h) * 6;
    const Buf b[] = {in("d_in", d_in, 16, tile_bytes(w, h)), out("d_out", d_out, 16, tile_bytes(w, h), "d_in"), opt(in("d_mv", p->d_mv, 8, blocks8(w, h) * 8)),
                     opt(in("d_nnz", p->d_nnz, 4, ctus(w, h) * 24)), opt(in("d_class", p->d_class, 1, tab)), opt(in("d_intra", p->d_intra, 1, tab)),
                     opt(in("d_qp", p->d_qp, 1, tab))};
    return check(b);
}
// xSaoStatsGpu (d_param NULL, lambda_q4 0) and xSaoSearchGpu (decide: d_param is the required output, d_stats the optional one)
inline const char *sao_stats(bool decide, const void *d_org, const void *d_dec, int w, int h, int lambda_q4, const void *d_param, const void *d_stats)
{
    if (const char *why = frame(w, h, 16)) return why;
    if (!lambda_ok(lambda_q4)) return "lambda_q4 must be 0..65535";
    Buf b[] = {out("d_param", d_param, 8, ctus(w, h) * 24), out("d_stats", d_stats, 4, ctus(w, h) * 1152), in("d_org", d_org, 16, tile_bytes(w, h)),
               in("d_dec", d_dec, 16, tile_bytes(w, h))};
    b[decide ? 1 : 0].optional = true;
    return check(b);
}
// the entry point then accepts n_ctu == 0 without a launch
inline const char *sao_decide(const void *d_stats, size_t n_ctu, int lambda_q4, const void *d_param)
{
    if (!lambda_ok(lambda_q4)) return "lambda_q4 must be 0..65535";
    if (n_ctu > 0x7FFFFFFFull) return "n_ctu must be below 2^31";
    const Buf b[] = {out("d_param", d_param, 8, n_ctu * 24), in("d_stats", d_stats, 4, n_ctu * 1152)};
    return check(b);
}
inline const char *sao_apply(const void *d_in, int w, int h, const void *d_param, const void *d_out)
{
    if (const char *why = frame(w, h, 16)) return why;
    const Buf b[] = {out("d_out", d_out, 16, tile_bytes(w, h)), in("d_in", d_in, 16, tile_bytes(w, h)), in("d_param", d_param, 8, ctus(w, h) * 24)};
    return check(b);                                                        // in place is not possible
}

// The adaptive loop filter.  A CTU's statistics are 2358 int32, a class map one byte per 4x4 luma block, d_ctrl 3 bytes per CTU; a
// set array is not looked at when its count is 0.
constexpr size_t kAlfCtuBytes = 2358 * 4;
constexpr const char *kAlfCounts = "n_luma and n_chroma must be 0..8";
inline size_t blocks4(int w, int h) { return (size_t)(w / 4) * (size_t)(h / 4); }
inline bool alf_counts_ok(int n_luma, int n_chroma) { return n_luma >= 0 && n_luma <= 8 && n_chroma >= 0 && n_chroma <= 8; }
inline Buf alf_sets(const char *name, const void *p, int count, size_t each) { return count > 0 ? in(name, p, 4, (size_t)count * each) : opt(in(name, nullptr, 4)); }
inline const char *alf_classify(const void *d_dec, int w, int h, const void *d_class)
{
    if (const char *why = frame(w, h, 16)) return why;
    const Buf b[] = {out("d_class", d_class, 1, blocks4(w, h)), in("d_dec", d_dec, 16, tile_bytes(w, h))};
    return check(b);
}
inline const char *alf_stats(const void *d_org, const void *d_dec, int w, int h, const void *d_class, const void *d_stats)
{
    if (const char *why = frame(w, h, 16)) return why;
    const Buf b[] = {out("d_stats", d_stats, 4, ctus(w, h) * kAlfCtuBytes), in("d_org", d_org, 16, tile_bytes(w, h)), in("d_dec", d_dec, 16, tile_bytes(w, h)),
                     opt(in("d_class", d_class, 1, blocks4(w, h)))};
    return check(b);
}
// the entry point then accepts n_ctu == 0 without a launch, as for the next one
inline const char *alf_sum_stats(const void *d_stats, size_t n_ctu, const void *d_mask, const void *d_total)
{
    if (n_ctu > 0x7FFFFFFFull) return "n_ctu must be below 2^31";
    const Buf b[] = {out("d_total", d_total, 8, 2358 * 8), in("d_stats", d_stats, 4, n_ctu * kAlfCtuBytes), opt(in("d_mask", d_mask, 1, n_ctu))};
    return check(b);
}
inline const char *alf_decide(const void *d_stats, size_t n_ctu, const void *d_luma, int n_luma, const void *d_chroma, int n_chroma, int lambda_q4,
                              const void *d_ctrl)
{
    if (!alf_counts_ok(n_luma, n_chroma)) return kAlfCounts;
    if (!lambda_ok(lambda_q4)) return "lambda_q4 must be 0..65535";
    if (n_ctu > 0x7FFFFFFFull) return "n_ctu must be below 2^31";
    const Buf b[] = {out("d_ctrl", d_ctrl, 1, n_ctu * 3), in("d_stats", d_stats, 4, n_ctu * kAlfCtuBytes), alf_sets("d_luma", d_luma, n_luma, sizeof(x266_alf_luma_t)),
                     alf_sets("d_chroma", d_chroma, n_chroma, sizeof(x266_alf_chroma_t))};
    return check(b);
}
inline const char *alf_apply(const void *d_in, int w, int h, const void *d_class, const void *d_luma, int n_luma, const void *d_chroma, int n_chroma,
                             const void *d_ctrl, const void *d_out)
{
    if (const char *why = frame(w, h, 16)) return why;
    if (!alf_counts_ok(n_luma, n_chroma)) return kAlfCounts;
    const Buf b[] = {out("d_out", d_out, 16, tile_bytes(w, h)), in("d_in", d_in, 16, tile_bytes(w, h)), opt(in("d_class", d_class, 1, blocks4(w, h))),
                     alf_sets("d_luma", d_luma, n_luma, sizeof(x266_alf_luma_t)), alf_sets("d_chroma", d_chroma, n_chroma, sizeof(x266_alf_chroma_t)),
                     in("d_ctrl", d_ctrl, 1, ctus(w, h) * 3)};
    return check(b);                                                        // in place is not possible
}

// ---- the compact level stream ------------------------------------------------------------------------------------------------------
// xLevelsPackGpu, xLevelsUnpackGpu: the device pointers are the fields of the host-read x266_levels_t, held by tests/cpp/struct_rules_check.cpp.
// d_stream may be NULL when cap_words is 0 (pack: the count-only call); with n_regions == 0 pack looks at d_total alone and unpack at nothing.
inline size_t levels_stream_bytes(uint64_t cap_words) { return cap_words > SIZE_MAX / 2 ? SIZE_MAX : (size_t)cap_words * 2; }
inline const char *levels_pack(const x266_levels_t *p)
{
    if (!p) return "NULL parameter struct";
    const size_t n = p->n_regions;
    if (n == 0) {
        const Buf b[] = {out("d_total", p->d_total, 8, 16)};
        return check(b);
    }
    Buf b[] = {out("d_region", p->d_region, 8, mul(n, 32)), out("d_stream", p->d_stream, 16, levels_stream_bytes(p->cap_words)), out("d_total", p->d_total, 8, 16),
               in("d_level", p->d_level, 16, mul(n, 2048)), opt(in("d_class", p->d_class, 1, n)), opt(in("d_nnz", p->d_nnz, 4, mul(n, 4)))};
    b[1].optional = p->cap_words == 0;
    return check(b);
}
inline const char *levels_unpack(const x266_levels_t *p)
{
    if (!p) return "NULL parameter struct";
    const size_t n = p->n_regions;
    if (n == 0) return nullptr;
    Buf b[] = {out("d_level", p->d_level, 16, mul(n, 2048)), opt(out("d_nnz", p->d_nnz, 4, mul(n, 4))), in("d_region", p->d_region, 8, mul(n, 32)),
               in("d_stream", p->d_stream, 16, levels_stream_bytes(p->cap_words)), opt(in("d_class", p->d_class, 1, n))};
    b[3].optional = p->cap_words == 0;
    return check(b);
}

// ---- rate-distortion optimised quantisation and the level rate estimate -------------------------------------------------------------
// xRdoQuantRegionsGpu, xLevelsBitsGpu: the device pointers are the fields of the host-read x266_rdoq_t, held by
// tests/cpp/struct_rules_check.cpp.  rdoq reads d_coef and writes d_level (which may BE d_coef), d_nnz and d_stat; bits reads d_level and
// d_nnz, writes d_stat and looks at neither d_coef, d_qp, qp nor lambda.  With n_regions == 0 neither looks at anything.
constexpr const char *kRdoqScalars = "qp must be 0..51 (without d_qp) and lambda 0..8192";
inline const char *rdoq_regions(const x266_rdoq_t *p)
{
    if (!p) return "NULL parameter struct";
    const size_t n = p->n_regions;
    if (n == 0) return nullptr;
    if (!qp_ok(p->d_qp, p->qp) || p->lambda < 0 || p->lambda > 8192) return kRdoqScalars;
    const Buf b[] = {out("d_level", p->d_level, 16, mul(n, 2048), "d_coef"), opt(out("d_nnz", p->d_nnz, 4, mul(n, 4))), opt(out("d_stat", p->d_stat, 8, mul(n, 16))),
                     in("d_coef", p->d_coef, 16, mul(n, 2048)), opt(in("d_class", p->d_class, 1, n)), opt(in("d_qp", p->d_qp, 1, n))};
    return check(b);
}
inline const char *levels_bits(const x266_rdoq_t *p)
{
    if (!p) return "NULL parameter struct";
    const size_t n = p->n_regions;
    if (n == 0) return nullptr;
    const Buf b[] = {out("d_stat", p->d_stat, 8, mul(n, 16)), in("d_level", p->d_level, 16, mul(n, 2048)), opt(in("d_class", p->d_class, 1, n)),
                     opt(in("d_nnz", p->d_nnz, 4, mul(n, 4)))};
    return check(b);
}

// ---- the transform decision ---------------------------------------------------------------------------------------------------------
// xTransformDecideCtuTilesGpu: the device pointers are the fields of the host-read x266_tdecide_t, held by tests/cpp/tdecide_rules_check.cpp.
// It reads d_cur and d_pred (which may be the same frame), d_qp and d_cand, and writes d_class, d_level, d_nnz, d_stat and d_cost: no
// output may overlap anything.
constexpr const char *kTDecideMasks = "cand_luma and cand_chroma must have a bit set and none outside 0x777F";
inline bool tdecide_mask_ok(unsigned m) { return m != 0 && (m & ~(unsigned)X266_TDECIDE_CLASSES) == 0; }
inline const char *transform_decide(const x266_tdecide_t *p)
{
    if (!p) return "NULL parameter struct";
    if (const char *why = frame(p->width, p->height, 16)) return why;
    if (!qp_ok(p->d_qp, p->qp) || p->lambda < 0 || p->lambda > 8192) return kRdoqScalars;
    if (!tdecide_mask_ok(p->cand_luma) || !tdecide_mask_ok(p->cand_chroma)) return kTDecideMasks;
    const size_t n = mul(ctus(p->width, p->height), 6), frame_bytes = tile_bytes(p->width, p->height);
    const Buf b[] = {out("d_class", p->d_class, 1, n), out("d_level", p->d_level, 16, mul(n, 2048)), opt(out("d_nnz", p->d_nnz, 4, mul(n, 4))),
                     opt(out("d_stat", p->d_stat, 8, mul(n, 16))), opt(out("d_cost", p->d_cost, 8, mul(n, 128))), in("d_cur", p->d_cur, 16, frame_bytes),
                     in("d_pred", p->d_pred, 16, frame_bytes), opt(in("d_qp", p->d_qp, 1, n)), opt(in("d_cand", p->d_cand, 2, mul(n, 2)))};
    return check(b);
}

// ---- frame quality ------------------------------------------------------------------------------------------------------------------
// xQualityStatsGpu: the device pointers are the fields of the host-read x266_quality_t, held by tests/cpp/quality_rules_check.cpp.  It
// reads d_src and d_dec (which may be the same frame) and writes d_ctu and, if given, d_total: no output may overlap anything.
constexpr const char *kQualityFlags = "flags must be X266_QUALITY_SSE, X266_QUALITY_SSIM or both";
inline const char *quality_stats(const x266_quality_t *p)
{
    if (!p) return "NULL parameter struct";
    if (const char *why = frame(p->width, p->height, 16)) return why;
    if (p->flags == 0 || (p->flags & ~(X266_QUALITY_SSE | X266_QUALITY_SSIM))) return kQualityFlags;
    const size_t frame_bytes = tile_bytes(p->width, p->height);
    const Buf b[] = {out("d_ctu", p->d_ctu, 16, mul(ctus(p->width, p->height), sizeof(x266_quality_ctu_t))), opt(out("d_total", p->d_total, 8, 64)),
                     in("d_src", p->d_src, 16, frame_bytes), in("d_dec", p->d_dec, 16, frame_bytes)};
    return check(b);
}
// xQualityFromTotals (host pointers): the totals of one frame, as xQualityStatsGpu writes them -- a window count is the geometry's, or 0
// after a run without X266_QUALITY_SSIM
inline const char *quality_from_totals(const int64_t *total, int w, int h, double *psnr, double *ssim)
{
    if (!total || !psnr || !ssim) return kNull;
    if (const char *why = frame(w, h, 16)) return why;
    for (int i = 0; i < 3; ++i)
        if (total[i] < 0) return "an SSE total is negative";
    const int64_t win_y = ((int64_t)(w / 4) - 1) * ((int64_t)(h / 4) - 1), win_c = ((int64_t)(w / 8) - 1) * ((int64_t)(h / 8) - 1);
    if ((total[6] != 0 && total[6] != win_y) || (total[7] != 0 && total[7] != win_c)) return "a window count is not the frame's";
    return nullptr;
}

// ---- source analysis ----------------------------------------------------------------------------------------------------------------
// xAqStatsGpu, xAqDecideGpu: the device pointers are the fields of the host-read x266_aq_t, held by tests/cpp/struct_rules_check.cpp.  Stats
// looks at d_src, d_tile, d_total and the frame size alone; decide at everything but d_src, and needs one of its two outputs.
constexpr const char *kAqScalars = "mode must be 1 or 2, strength_q8 0..1024, qp 0..51 and chroma_qp_offset -12..12";
inline size_t tiles16(int w, int h) { return (size_t)(w / 16) * (size_t)(h / 16); }
inline const char *aq_stats(const x266_aq_t *p)
{
    if (!p) return "NULL parameter struct";
    if (const char *why = frame(p->width, p->height, 16)) return why;
    const Buf b[] = {out("d_tile", p->d_tile, 16, tiles16(p->width, p->height) * 32), out("d_total", p->d_total, 8, 64),
                     in("d_src", p->d_src, 16, tile_bytes(p->width, p->height))};
    return check(b);
}
inline const char *aq_decide(const x266_aq_t *p)
{
    if (!p) return "NULL parameter struct";
    if (const char *why = frame(p->width, p->height, 16)) return why;
    if (p->mode < 1 || p->mode > 2 || p->strength_q8 < 0 || p->strength_q8 > 1024 || p->qp < 0 || p->qp > 51 || p->chroma_qp_offset < -12 ||
        p->chroma_qp_offset > 12)
        return kAqScalars;
    if (!p->d_offset && !p->d_qp) return "d_offset and d_qp are both NULL";
    const Buf b[] = {opt(out("d_offset", p->d_offset, 2, tiles16(p->width, p->height) * 2)), opt(out("d_qp", p->d_qp, 1, ctus(p->width, p->height) * 6)),
                     in("d_tile", p->d_tile, 16, tiles16(p->width, p->height) * 32), in("d_total", p->d_total, 8, 64)};
    return check(b);
}
// xWeightsFromTotals (host pointers): the totals of two frames of one size, as xAqStatsGpu writes them
inline const char *weights_from_totals(const int64_t *cur, const int64_t *ref, int list, const x266_wp_t *wp)
{
    if (!cur || !ref || !wp) return kNull;
    if (list < 0 || list > 1) return "list must be 0 or 1";
    if (wp->log2_denom[0] > 7 || wp->log2_denom[1] > 7) return "log2_denom must be 0..7";
    if (cur[7] != ref[7]) return "the two frames differ in size";
    if (cur[7] < 1 || cur[7] > ((int64_t)1 << 24)) return "the tile count must be 1..2^24";
    for (int i = 0; i < 7; ++i)
        if (cur[i] < 0 || ref[i] < 0) return "a total is negative";
    return nullptr;
}

// ---- lookahead ------------------------------------------------------------------------------------------------------------------------
// xLaDownscaleGpu, xLaIntraCostsGpu, xLaFrameCostGpu, xLaPropagateGpu, xLaTreeQpGpu: the device pointers are the fields of the host-read
// x266_la_t, held by tests/cpp/struct_rules_check.cpp.  Each call looks at the fields the header names for it; the sides are the
// full-resolution frame's, multiples of 32; n = tiles16 is the number of lowres blocks.  An accumulator added into counts as an output.
constexpr const char *kLaPenalty = "intra_penalty must be 0..65535";
constexpr const char *kLaScalars = "strength_q8 must be 0..1024, qp 0..51 and chroma_qp_offset -12..12";
inline const char *la_frame(const x266_la_t *p)
{
    if (!p) return "NULL parameter struct";
    return frame(p->width, p->height, 32);
}
inline const char *la_downscale(const x266_la_t *p)
{
    if (const char *why = la_frame(p)) return why;
    const Buf b[] = {out("d_low", p->d_low, 16, tile_bytes(p->width, p->height) / 4), in("d_src", p->d_src, 16, tile_bytes(p->width, p->height))};
    return check(b);
}
inline const char *la_intra_costs(const x266_la_t *p)
{
    if (const char *why = la_frame(p)) return why;
    const size_t n = tiles16(p->width, p->height);
    const Buf b[] = {out("d_intra", p->d_intra, 4, n * 4), opt(out("d_mode", p->d_mode, 1, n)), in("d_low", p->d_low, 16, tile_bytes(p->width, p->height) / 4)};
    return check(b);
}
inline const char *la_frame_cost(const x266_la_t *p)
{
    if (const char *why = la_frame(p)) return why;
    if (p->intra_penalty < 0 || p->intra_penalty > 65535) return kLaPenalty;
    const size_t n = tiles16(p->width, p->height);
    const Buf b[] = {out("d_block", p->d_block, 16, n * 16), out("d_total", p->d_total, 8, 64), in("d_intra", p->d_intra, 4, n * 4), opt(in("d_mode", p->d_mode, 1, n)),
                     opt(in("d_inter0", p->d_inter0, 8, n * 8)), opt(in("d_inter1", p->d_inter1, 8, n * 8))};
    return check(b);
}
inline const char *la_propagate(const x266_la_t *p)
{
    if (const char *why = la_frame(p)) return why;
    const size_t n = tiles16(p->width, p->height);
    const Buf b[] = {opt(out("d_prop_ref0", p->d_prop_ref0, 8, n * 8)), opt(out("d_prop_ref1", p->d_prop_ref1, 8, n * 8)), in("d_block", p->d_block, 16, n * 16),
                     opt(in("d_prop", p->d_prop, 8, n * 8))};
    return check(b);
}
inline const char *la_tree_qp(const x266_la_t *p)
{
    if (const char *why = la_frame(p)) return why;
    if (p->strength_q8 < 0 || p->strength_q8 > 1024 || p->qp < 0 || p->qp > 51 || p->chroma_qp_offset < -12 || p->chroma_qp_offset > 12) return kLaScalars;
    if (!p->d_offset && !p->d_qp) return "d_offset and d_qp are both NULL";
    const size_t n = tiles16(p->width, p->height);
    const Buf b[] = {opt(out("d_offset", p->d_offset, 2, n * 2)), opt(out("d_qp", p->d_qp, 1, ctus(p->width, p->height) * 6)), in("d_block", p->d_block, 16, n * 16),
                     opt(in("d_prop", p->d_prop, 8, n * 8)), opt(in("d_aq_offset", p->d_aq_offset, 2, n * 2))};
    return check(b);
}
// xSceneCutFromTotals (a host pointer): p and i above 2^40 are refused so that every product fits int64
inline const char *scene_cut_from_totals(const int64_t *total, int threshold_q8, int frames_since_key, int min_keyint, int max_keyint)
{
    if (!total) return kNull;
    if (threshold_q8 < 0 || threshold_q8 > 256) return "threshold_q8 must be 0..256";
    if (frames_since_key < 0 || min_keyint < 1 || max_keyint < min_keyint) return "frames_since_key must be >= 0 and 1 <= min_keyint <= max_keyint";
    for (int i = 0; i < 8; ++i)
        if (total[i] < 0) return "a total is negative";
    if (total[7] < 1 || total[7] > ((int64_t)1 << 24)) return "the block count must be 1..2^24";
    if (total[0] > ((int64_t)1 << 40) || total[1] > ((int64_t)1 << 40)) return "a cost total is above 2^40";
    return nullptr;
}

// ---- the seeded search ----------------------------------------------------------------------------------------------------------------
// xSatd8x8SeededSearchGpu: the device pointers are the fields of the host-read x266_seed_t, held by tests/cpp/struct_rules_check.cpp.  The
// seed grid and the scalars' ranges are x266_seed.hpp's, the kernel's own.  The two frames are read-only and may be one; an output
// overlaps nothing, the seeds included: blocks read their neighbours' seeds.
constexpr const char *kSeedScalars = "seed_scale must be 0 or 1, centres 0..31, range 0..8 and lambda_q4 0..65535";
inline const char *seeded_search(const x266_seed_t *p)
{
    if (!p) return "NULL parameter struct";
    if (const char *why = frame(p->width, p->height, 16)) return why;
    if (p->seed_scale < 0 || p->seed_scale > 1 || p->centres < 0 || p->centres > kSeedCentreBits || p->range < 0 || p->range > kSeedMaxRange || !lambda_ok(p->lambda_q4))
        return kSeedScalars;
    const size_t n = blocks8(p->width, p->height);
    const Buf b[] = {out("d_best", p->d_best, 8, n * 8), opt(out("d_j", p->d_j, 4, n * 4)), in("d_cur", p->d_cur, 16, tile_bytes(p->width, p->height)),
                     in("d_ref", p->d_ref, 16, tile_bytes(p->width, p->height)), in("d_seed", p->d_seed, 8, seed_cells(p->width, p->height, p->seed_scale) * 8)};
    return check(b);
}

// ---- the inter partition decision -----------------------------------------------------------------------------------------------------
// xInterPartitionDecideGpu: the device pointers are the fields of the host-read x266_part_t, held by tests/cpp/partition_rules_check.cpp.
// The node counts and the range of r are x266_part.hpp's, the kernel's own.  The two frames are read-only and may be one; an output
// overlaps nothing, the input field included: nodes read their neighbours' input vectors.
constexpr const char *kPartScalars = "range must be 0 or 1 and lambda_q4 0..65535";
inline const char *partition_decide(const x266_part_t *p)
{
    if (!p) return "NULL parameter struct";
    if (const char *why = frame(p->width, p->height, 16)) return why;
    if (p->range < 0 || p->range > kPartMaxRange || !lambda_ok(p->lambda_q4)) return kPartScalars;
    const size_t n = blocks8(p->width, p->height), frame_bytes = tile_bytes(p->width, p->height);
    const Buf b[] = {out("d_out", p->d_out, 8, n * 8), out("d_level", p->d_level, 1, n), out("d_ctu", p->d_ctu, 8, ctus(p->width, p->height) * sizeof(x266_part_ctu_t)),
                     opt(out("d_nodes", p->d_nodes, 8, part_nodes_total(p->width / 8, p->height / 8) * 8)), in("d_cur", p->d_cur, 16, frame_bytes),
                     in("d_ref", p->d_ref, 16, frame_bytes), in("d_mv", p->d_mv, 8, n * 8)};
    return check(b);
}

// ---- the compact motion stream --------------------------------------------------------------------------------------------------------
// xMotionPackGpu, xMotionUnpackGpu: the device pointers are the fields of the host-read x266_motion_t, held by
// tests/cpp/motion_rules_check.cpp.  The stream's extent and the count-only call (d_stream NULL with cap_words 0) are the level stream's;
// d_total is the pack call's alone.  An output overlaps nothing.
inline const char *motion_pack(const x266_motion_t *p)
{
    if (!p) return "NULL parameter struct";
    if (const char *why = frame(p->width, p->height, 16)) return why;
    const size_t n = blocks8(p->width, p->height);
    Buf b[] = {out("d_ctu", p->d_ctu, 8, ctus(p->width, p->height) * sizeof(x266_motion_ctu_t)), out("d_stream", p->d_stream, 16, levels_stream_bytes(p->cap_words)),
               out("d_total", p->d_total, 8, 16), in("d_mv", p->d_mv, 8, n * 8), in("d_level", p->d_level, 1, n)};
    b[1].optional = p->cap_words == 0;
    return check(b);
}
inline const char *motion_unpack(const x266_motion_t *p)
{
    if (!p) return "NULL parameter struct";
    if (const char *why = frame(p->width, p->height, 16)) return why;
    const size_t n = blocks8(p->width, p->height);
    Buf b[] = {out("d_mv", p->d_mv, 8, n * 8), out("d_level", p->d_level, 1, n), in("d_ctu", p->d_ctu, 8, ctus(p->width, p->height) * sizeof(x266_motion_ctu_t)),
               in("d_stream", p->d_stream, 16, levels_stream_bytes(p->cap_words))};
    b[3].optional = p->cap_words == 0;
    return check(b);
}

// ---- the entropy coder of the level stream -------------------------------------------------------------------------------------------------
// xEntropyEncodeLevelsGpu, xEntropyDecodeLevelsGpu: the device pointers are the fields of the host-read x266_entropy_t, held by
// tests/cpp/entropy_rules_check.cpp.  Buffers, extents and the count-only call are the compact level stream's; `init` is host memory and
// every entry of it lies in 31 .. 2017, the interval the adaptation never leaves.
constexpr const char *kEntropyInit = "every entry of init must be 31..2017";
inline bool entropy_init_ok(const uint16_t *init)
{
    if (!init) return true;
    for (unsigned i = 0; i < X266_ENTROPY_CONTEXTS; ++i)
        if (init[i] < 31 || init[i] > 2017) return false;
    return true;
}
inline const char *entropy_encode(const x266_entropy_t *p)
{
    if (!p) return "NULL parameter struct";
    if (!entropy_init_ok(p->init)) return kEntropyInit;
    const size_t n = p->n_regions;
    if (n == 0) {
        const Buf b[] = {out("d_total", p->d_total, 8, 16)};
        return check(b);
    }
    Buf b[] = {out("d_region", p->d_region, 8, mul(n, 32)), out("d_stream", p->d_stream, 16, levels_stream_bytes(p->cap_words)), out("d_total", p->d_total, 8, 16),
               in("d_level", p->d_level, 16, mul(n, 2048)), opt(in("d_class", p->d_class, 1, n)), opt(in("d_nnz", p->d_nnz, 4, mul(n, 4)))};
    b[1].optional = p->cap_words == 0;
    return check(b);
}
inline const char *entropy_decode(const x266_entropy_t *p)
{
    if (!p) return "NULL parameter struct";
    if (!entropy_init_ok(p->init)) return kEntropyInit;
    const size_t n = p->n_regions;
    if (n == 0) return nullptr;
    Buf b[] = {out("d_level", p->d_level, 16, mul(n, 2048)), opt(out("d_nnz", p->d_nnz, 4, mul(n, 4))), in("d_region", p->d_region, 8, mul(n, 32)),
               in("d_stream", p->d_stream, 16, levels_stream_bytes(p->cap_words)), opt(in("d_class", p->d_class, 1, n))};
    b[3].optional = p->cap_words == 0;
    return check(b);
}

// ---- the entropy coder of the motion stream ----------------------------------------------------------------------------------------------
// xEntropyEncodeMvGpu, xEntropyDecodeMvGpu: the device pointers are the fields of the host-read x266_entropy_motion_t, held by
// tests/cpp/entropy_motion_rules_check.cpp.  `init` is host memory, 7 entries in 31 .. 2017; the stream's extent and the count-only call
// are the level stream's; d_words is in_words * 2 bytes on encode (NULL allowed when that is 0) and 512 bytes per CTU on decode.
// xMotionReconstructGpu has the rules of xMotionUnpackGpu.
inline bool entropy_motion_init_ok(const uint16_t *init)
{
    if (!init) return true;
    for (unsigned i = 0; i < X266_ENTROPY_MOTION_CONTEXTS; ++i)
        if (init[i] < 31 || init[i] > 2017) return false;
    return true;
}
inline const char *entropy_motion_encode(const x266_entropy_motion_t *p)
{
    if (!p) return "NULL parameter struct";
    if (const char *why = frame(p->width, p->height, 16)) return why;
    if (!entropy_motion_init_ok(p->init)) return kEntropyInit;
    const size_t n = ctus(p->width, p->height);
    Buf b[] = {out("d_coded", p->d_coded, 8, n * sizeof(x266_entropy_motion_ctu_t)), out("d_stream", p->d_stream, 16, levels_stream_bytes(p->cap_words)),
               out("d_total", p->d_total, 8, 16), in("d_ctu", p->d_ctu, 8, n * sizeof(x266_motion_ctu_t)), in("d_words", p->d_words, 16, levels_stream_bytes(p->in_words))};
    b[1].optional = p->cap_words == 0;
    b[4].optional = p->in_words == 0;
    return check(b);
}
inline const char *entropy_motion_decode(const x266_entropy_motion_t *p)
{
    if (!p) return "NULL parameter struct";
    if (const char *why = frame(p->width, p->height, 16)) return why;
    if (!entropy_motion_init_ok(p->init)) return kEntropyInit;
    const size_t n = ctus(p->width, p->height);
    Buf b[] = {out("d_ctu", p->d_ctu, 8, n * sizeof(x266_motion_ctu_t)), out("d_words", p->d_words, 16, n * 512), opt(out("d_status", p->d_status, 1, n)),
               in("d_coded", p->d_coded, 8, n * sizeof(x266_entropy_motion_ctu_t)), in("d_stream", p->d_stream, 16, levels_stream_bytes(p->cap_words))};
    b[4].optional = p->cap_words == 0;
    return check(b);
}
inline const char *motion_reconstruct(const x266_motion_t *p) { return motion_unpack(p); }

// ---- the entropy coder of the side information -------------------------------------------------------------------------------------------
// xEntropyEncodeSideGpu, xEntropyDecodeSideGpu: the device pointers are the fields of the host-read x266_entropy_side_t, held by
// tests/cpp/entropy_side_rules_check.cpp.  `init` is host memory, 16 entries in 31 .. 2017; the stream's extent and the count-only call are
// the level stream's; the five arrays are optional on both sides, but kinds cannot be coded without their modes.
constexpr const char *kEntropySideScalars = "qp must be 0..51 and chroma_qp_offset -12..12";
constexpr const char *kEntropySideModes = "d_kind needs d_mode";
inline bool entropy_side_init_ok(const uint16_t *init)
{
    if (!init) return true;
    for (unsigned i = 0; i < X266_ENTROPY_SIDE_CONTEXTS; ++i)
        if (init[i] < 31 || init[i] > 2017) return false;
    return true;
}
inline bool entropy_side_scalars_ok(int qp, int chroma_qp_offset) { return qp >= 0 && qp <= 51 && chroma_qp_offset >= -12 && chroma_qp_offset <= 12; }
inline const char *entropy_side_encode(const x266_entropy_side_t *p)
{
    if (!p) return "NULL parameter struct";
    if (!entropy_side_scalars_ok(p->qp, p->chroma_qp_offset)) return kEntropySideScalars;
    if (!entropy_side_init_ok(p->init)) return kEntropyInit;
    const size_t n = p->n_ctu;
    if (n == 0) {
        const Buf b[] = {out("d_total", p->d_total, 8, 16)};
        return check(b);
    }
    if (p->d_kind && !p->d_mode) return kEntropySideModes;
    Buf b[] = {out("d_coded", p->d_coded, 8, mul(n, 32)), out("d_stream", p->d_stream, 16, levels_stream_bytes(p->cap_words)), out("d_total", p->d_total, 8, 16),
               opt(in("d_kind", p->d_kind, 1, mul(n, 6))), opt(in("d_mode", p->d_mode, 1, mul(n, 6))), opt(in("d_class", p->d_class, 1, mul(n, 6))),
               opt(in("d_qp", p->d_qp, 1, mul(n, 6))), opt(in("d_nnz", p->d_nnz, 4, mul(n, 24)))};
    b[1].optional = p->cap_words == 0;
    return check(b);
}
inline const char *entropy_side_decode(const x266_entropy_side_t *p)
{
    if (!p) return "NULL parameter struct";
    if (!entropy_side_scalars_ok(p->qp, p->chroma_qp_offset)) return kEntropySideScalars;
    if (!entropy_side_init_ok(p->init)) return kEntropyInit;
    const size_t n = p->n_ctu;
    if (n == 0) return nullptr;
    Buf b[] = {opt(out("d_kind", p->d_kind, 1, mul(n, 6))), opt(out("d_mode", p->d_mode, 1, mul(n, 6))), opt(out("d_class", p->d_class, 1, mul(n, 6))),
               opt(out("d_qp", p->d_qp, 1, mul(n, 6))), opt(out("d_nnz", p->d_nnz, 4, mul(n, 24))), opt(out("d_status", p->d_status, 1, n)),
               in("d_coded", p->d_coded, 8, mul(n, 32)), in("d_stream", p->d_stream, 16, levels_stream_bytes(p->cap_words))};
    b[7].optional = p->cap_words == 0;
    return check(b);
}

// ---- the per-context bin statistics ----------------------------------------------------------------------------------------------------------
// xEntropyStatsLevelsGpu, xEntropyStatsSideGpu: the device pointers are the fields of the host-read x266_entropy_stats_t and
// x266_entropy_side_stats_t, held by tests/cpp/entropy_stats_rules_check.cpp.  The inputs are the encode calls'; d_counts is 16 bytes per
// context and d_part that per row of X266_ENTROPY_STATS_REGIONS regions or X266_ENTROPY_SIDE_STATS_CTUS CTUs.  With n == 0 only d_counts
// (and the side call's scalars) are looked at.
inline size_t entropy_stats_rows(size_t n_units, size_t per_row) { return per_row ? n_units / per_row + (n_units % per_row != 0) : 0; }
inline const char *entropy_stats_levels(const x266_entropy_stats_t *p)
{
    if (!p) return "NULL parameter struct";
    const size_t n = p->n_regions, counts = 16 * X266_ENTROPY_CONTEXTS;
    if (n == 0) {
        const Buf b[] = {out("d_counts", p->d_counts, 8, counts)};
        return check(b);
    }
    const Buf b[] = {out("d_counts", p->d_counts, 8, counts), out("d_part", p->d_part, 16, mul(entropy_stats_rows(n, X266_ENTROPY_STATS_REGIONS), counts / 2)),
                     in("d_level", p->d_level, 16, mul(n, 2048)), opt(in("d_class", p->d_class, 1, n)), opt(in("d_nnz", p->d_nnz, 4, mul(n, 4)))};
    return check(b);
}
inline const char *entropy_stats_side(const x266_entropy_side_stats_t *p)
{
    if (!p) return "NULL parameter struct";
    if (!entropy_side_scalars_ok(p->qp, p->chroma_qp_offset)) return kEntropySideScalars;
    const size_t n = p->n_ctu, counts = 16 * X266_ENTROPY_SIDE_CONTEXTS;
    if (n == 0) {
        const Buf b[] = {out("d_counts", p->d_counts, 8, counts)};
        return check(b);
    }
    if (p->d_kind && !p->d_mode) return kEntropySideModes;
    const Buf b[] = {out("d_counts", p->d_counts, 8, counts), out("d_part", p->d_part, 16, mul(entropy_stats_rows(n, X266_ENTROPY_SIDE_STATS_CTUS), counts / 2)),
                     opt(in("d_kind", p->d_kind, 1, mul(n, 6))), opt(in("d_mode", p->d_mode, 1, mul(n, 6))), opt(in("d_class", p->d_class, 1, mul(n, 6))),
                     opt(in("d_qp", p->d_qp, 1, mul(n, 6))), opt(in("d_nnz", p->d_nnz, 4, mul(n, 24)))};
    return check(b);
}

// ---- intra coding of tiled frames --------------------------------------------------------------------------------------------------
inline const char *intra32_refs_from_tiles(const void *d_frame, int w, int h, int component, const void *d_refs)
{
    if (const char *why = frame(w, h, 64)) return why;
    if (component < 0 || component > 2) return "component must be 0, 1 or 2";
    const Buf b[] = {out("d_refs", d_refs, 16, ctus(w, h) * (component == 0 ? 4u : 1u) * sizeof(x266_intra_ref_t)), in("d_frame", d_frame, 16, tile_bytes(w, h))};
    return check(b);
}
inline const char *intra32_code_frame(const void *d_cur, int w, int h, const void *d_qp, int qp, int rounding, const void *d_mode_in, const void *d_level,
                                      const void *d_nnz, const void *d_mode, const void *d_recon)
{
    if (const char *why = frame(w, h, 64)) return why;
    if (!qp_ok(d_qp, qp) || !rounding_ok(rounding)) return kQuantScalars;
    const Buf b[] = {out("d_recon", d_recon, 16, tile_bytes(w, h)), out("d_level", d_level, 16, ctus(w, h) * 12288), out("d_mode", d_mode, 1, ctus(w, h) * 6, "d_mode_in"),
                     opt(out("d_nnz", d_nnz, 4, ctus(w, h) * 24)), in("d_cur", d_cur, 16, tile_bytes(w, h)), opt(in("d_qp", d_qp, 1, ctus(w, h) * 6)),
                     opt(in("d_mode_in", d_mode_in, 1, ctus(w, h) * 6))};
    return check(b);
}
// xDct32CodeMixedFrameGpu: the device pointers are the fields of the host-read x266_mixed_t, held by tests/cpp/struct_rules_check.cpp.  Three
// outputs may BE one input each (the reconstruction the inter prediction, the kinds and the modes their inputs); d_cur == d_pred are two inputs.
constexpr const char *kMixedPenalty = "intra_penalty must be 0..16777216";
inline const char *mixed_code_frame(const x266_mixed_t *p)
{
    if (!p) return "NULL parameter struct";
    const int w = p->width, h = p->height;
    if (const char *why = frame(w, h, 64)) return why;
    if (!qp_ok(p->d_qp, p->qp) || !rounding_ok(p->rounding)) return kQuantScalars;
    if (p->intra_penalty < 0 || p->intra_penalty > (1 << 24)) return kMixedPenalty;
    const size_t n = ctus(w, h) * 6;
    const Buf b[] = {out("d_recon", p->d_recon, 16, tile_bytes(w, h), "d_pred"), out("d_level", p->d_level, 16, n * 2048), out("d_kind", p->d_kind, 1, n, "d_kind_in"),
                     out("d_mode", p->d_mode, 1, n, "d_mode_in"), opt(out("d_nnz", p->d_nnz, 4, n * 4)), opt(out("d_cost", p->d_cost, 4, n * 8)),
                     in("d_cur", p->d_cur, 16, tile_bytes(w, h)), in("d_pred", p->d_pred, 16, tile_bytes(w, h)), opt(in("d_qp", p->d_qp, 1, n)),
                     opt(in("d_kind_in", p->d_kind_in, 1, n)), opt(in("d_mode_in", p->d_mode_in, 1, n))};
    return check(b);
}

}  // namespace args
}  // namespace x266
