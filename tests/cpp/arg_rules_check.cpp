// CPU check of the device entry points' argument rules (x266_amd/csrc/x266_args.hpp).  The rule functions are pure integer
// arithmetic on addresses and sizes, so the addresses here are made-up integers: nothing is dereferenced and no device is needed.
//
// CALLS below is the contract written down once more, by hand, from include/x266hip.h and from the checks the entry points
// carried before the rules moved into the header: one row per device entry point, with every pointer's alignment, whether it
// may be NULL, whether it is written, its extent as a function of the call's sizes where the call's rules have one (none: the
// older calls check NULL and alignment only, and overlapping buffers are ACCEPTED there -- recorded as today's behaviour, so that
// tightening one is a visible diff of this table), whether the span's end is held against the address space, the exact alias it
// may form, and an output the rules do not hold it against.  One walk (generic) perturbs every row the same way; the checks that
// are a call's own follow in own_rules.  The expected verdict of every perturbation follows from that table and from the
// literals in the per-call checks, never from the functions under test.  A new entry point adds a row.
// Test infrastructure; built and run by tests/test_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "rules_expect.hpp"
#include "x266_args.hpp"

using namespace x266;

struct Args {
    std::vector<U> p;
    int w = 0, h = 0;       // frame calls
    size_t n = 0;           // count calls: blocks, regions, CTUs
    // the scalars, each at a valid value
    int qp = 30, rounding = 171, beta = 0, tc = 0, lambda_q4 = 100, range = 4, shift = 7, component = 0, planes = 3, list = 1, bi_penalty = 7, n_luma = 3,
        n_chroma = 8;
    const x266_wp_t *wp = nullptr;
};
static const void *V(U x) { return (const void *)x; }

typedef size_t (*Extent)(const Args &);
enum { OPT = 1, OUT = 2, UNFIT = 4 };
struct Ptr {
    const char *name;
    unsigned align;
    int flags = 0;
    Extent bytes = nullptr;            // nullptr: no extent in this call's rules
    const char *alias = nullptr;       // the input this output may exactly be
    const char *not_vs = nullptr;      // an output the rules do not hold this one against
};
struct Call {
    const char *name;
    int granule;             // 0: a count call (n units; n == 0 is accepted whatever the pointers are, unless zero_needs_ptrs)
    std::vector<Ptr> ptrs;
    std::function<const char *(const Args &)> rule;
    bool zero_needs_ptrs = false;
    bool uv_rule = false;         // the last two pointers are the U / V output streams, which have a rule of their own
};

// extents, as include/x266hip.h states them
static size_t BLK(const Args &a, size_t edge) { return ((size_t)a.w / edge) * ((size_t)a.h / edge); }
static size_t CT(const Args &a) { return (((size_t)a.w + 63) / 64) * (((size_t)a.h + 63) / 64); }
static size_t TB(const Args &a) { return BLK(a, 1) * 2; }                           // a frame of tiles: 512 bytes per 16x16 pixels
static size_t B8(const Args &a) { return BLK(a, 8) * 8; }                           // one 8-byte record per 8x8 block
static size_t B8x1(const Args &a) { return BLK(a, 8); }                             // a direction byte per 8x8 block
static size_t B8x12(const Args &a) { return BLK(a, 8) * 12; }                       // three costs per 8x8 block
static size_t B4x1(const Args &a) { return BLK(a, 4); }                             // a class byte per 4x4 block
static size_t CT3(const Args &a) { return CT(a) * 3; }
static size_t CT6(const Args &a) { return CT(a) * 6; }
static size_t CT24(const Args &a) { return CT(a) * 24; }
static size_t CT12K(const Args &a) { return CT(a) * 12288; }
static size_t CT1152(const Args &a) { return CT(a) * 1152; }
static size_t CT9432(const Args &a) { return CT(a) * 9432; }                        // a CTU's ALF statistics: 2358 int32
static size_t REFS(const Args &a) { return CT(a) * (a.component ? 1 : 4) * sizeof(x266_intra_ref_t); }
static size_t COSTS(const Args &a) { return BLK(a, 8) * (2 * a.range + 1) * (2 * a.range + 1) * 4; }
static size_t COSTS49(const Args &a) { return BLK(a, 8) * 49 * 4; }
static size_t CHROMA8(const Args &a) { return BLK(a, 16) * 128; }                   // 8x8 int16 blocks at pitch 1
static size_t N2048(const Args &a) { return a.n * 2048; }
static size_t N1(const Args &a) { return a.n; }
static size_t N3(const Args &a) { return a.n * 3; }
static size_t N4(const Args &a) { return a.n * 4; }
static size_t N24(const Args &a) { return a.n * 24; }
static size_t N1152(const Args &a) { return a.n * 1152; }
static size_t N9432(const Args &a) { return a.n * 9432; }
static size_t TOTAL(const Args &) { return 2358 * 8; }
static size_t LUMA(const Args &a) { return (size_t)a.n_luma * 600; }
static size_t CHROMA(const Args &a) { return (size_t)a.n_chroma * 16; }

// every pointer in a region of its own, at exactly its alignment times an odd number
static Args base(const Call &c, int mult_w = 1, int mult_h = 1)
{
    Args a;
    for (size_t i = 0; i < c.ptrs.size(); ++i) a.p.push_back(((U)(i + 1) << 44) + (U)c.ptrs[i].align * (2 * i + 1));
    a.w = c.granule * mult_w;
    a.h = c.granule * mult_h;
    a.n = 3;
    return a;
}
// the second frame size: 80x48 has a cut CTU column and a cut CTU row, 96x96 likewise; a granule of 64 cuts nothing
static Args second(const Call &c) { return c.granule <= 16 ? base(c, 80 / c.granule, 48 / c.granule) : c.granule == 32 ? base(c, 3, 3) : base(c, 3, 2); }
static const char *size_reason(int granule)
{
    return granule == 8 ? "width/height must be positive multiples of 8" : granule == 16 ? "width/height must be positive multiples of 16"
         : granule == 32 ? "width/height must be positive multiples of 32" : "width/height must be positive multiples of 64";
}

static void generic(const Call &c)
{
    const char *n = c.name;
    expect(n, "base", c.rule(base(c)), false);
    if (c.granule) expect(n, "second size", c.rule(second(c)), false);
    bool extents = false;
    for (size_t i = 0; i < c.ptrs.size(); ++i) {
        const Ptr &p = c.ptrs[i];
        Args a = base(c);
        a.p[i] = 0;
        expect(n, std::string(p.name) + " NULL", c.rule(a), !(p.flags & OPT), (p.flags & OPT) ? nullptr : args::kNull);
        if (p.align > 1) {
            a = base(c);
            a.p[i] += p.align / 2;
            expect(n, std::string(p.name) + " at half its alignment", c.rule(a), true, args::kMisaligned);
        }
        extents = extents || p.bytes;
    }
    if (c.granule) {
        for (int dim = 0; dim < 2; ++dim)
            for (int v : {0, -c.granule, c.granule / 2, c.granule + c.granule / 2}) {
                Args a = base(c);
                (dim ? a.h : a.w) = v;
                expect(n, std::string(dim ? "height " : "width ") + std::to_string(v), c.rule(a), true, size_reason(c.granule));
            }
    } else {
        Args a = base(c);
        a.n = 0;
        expect(n, "n == 0", c.rule(a), false);
        for (U &x : a.p) x = 0;
        expect(n, "n == 0, NULL pointers", c.rule(a), c.zero_needs_ptrs);
    }
    if (!extents) {                                         // today's behaviour: these calls do not look at overlap
        Args a = base(c);
        for (size_t i = 0; i + (c.uv_rule ? 1 : 0) < a.p.size(); ++i) a.p[i] = ((U)1 << 44) + 16 * 3;
        expect(n, "every buffer at one address (no extents in the rules)", c.rule(a), false);
        return;
    }
    const U shared = (U)(c.ptrs.size() + 1) << 44;          // a region of its own, aligned for every buffer
    for (int size = 0; size < (c.granule ? 2 : 1); ++size) {
        const Args b = size ? second(c) : base(c);
        for (size_t o = 0; o < c.ptrs.size(); ++o) {
            const Ptr &po = c.ptrs[o];
            if (!po.bytes) continue;
            const size_t no = po.bytes(b);
            const bool fitted = !(po.flags & UNFIT);
            // the top of the address space: the highest aligned address whose span fits, the next one, and the highest aligned address
            Args a = b;
            a.p[o] = down(UINTPTR_MAX - no, po.align);
            expect(n, std::string(po.name) + " ends at the top of the address space", c.rule(a), false);
            a.p[o] += po.align;
            if (a.p[o]) expect(n, std::string(po.name) + " ends one unit past the top of the address space", c.rule(a), fitted, fitted ? args::kNoFit : nullptr);
            a.p[o] = down(UINTPTR_MAX, po.align);
            expect(n, std::string(po.name) + " runs past the top of the address space", c.rule(a), fitted, fitted ? args::kNoFit : nullptr);
            if (!(po.flags & OUT)) continue;
            for (size_t i = 0; i < c.ptrs.size(); ++i) {
                const Ptr &pi = c.ptrs[i];
                if (i == o || !pi.bytes) continue;
                const size_t ni = pi.bytes(b);
                const bool held = !(po.not_vs && !std::strcmp(po.not_vs, pi.name));
                const bool alias = po.alias && !std::strcmp(po.alias, pi.name);
                const std::string pair = std::string(po.name) + " / " + pi.name;
                a = b;
                a.p[o] = up(b.p[i] - no + 1, po.align);             // the last byte(s) of the output on the first of the other
                expect(n, pair + " overlap from below", c.rule(a), held, held ? args::kOverlap : nullptr);
                a.p[o] = down(b.p[i] + ni - 1, po.align);           // the output starts in the last byte(s) of the other
                expect(n, pair + " overlap from above", c.rule(a), held, held ? args::kOverlap : nullptr);
                a.p[o] = down(b.p[i] - no, po.align);
                expect(n, pair + " end touches start", c.rule(a), false);
                a.p[o] = up(b.p[i] + ni, po.align);
                expect(n, pair + " start touches end", c.rule(a), false);
                a = b;
                a.p[o] = a.p[i] = shared;
                expect(n, pair + " at the same address", c.rule(a), !alias && held, alias || !held ? nullptr : args::kOverlap);
                if (alias) {                                        // the two are aligned alike wherever an alias is allowed
                    a = b;
                    a.p[o] = b.p[i] + po.align;
                    expect(n, pair + " alias moved by one alignment unit", c.rule(a), true, args::kOverlap);
                }
            }
        }
    }
}

// ---- the table ---------------------------------------------------------------------------------------------------------------------
#define P(i) V(a.p[i])
static std::vector<Call> CALLS;
static const Call &call(const char *name) {
    for (const Call &c : CALLS) if (!std::strcmp(c.name, name)) return c;
    std::printf("no call %s\n", name);
    std::exit(2);
}
static x266_deblock_t deblock_params(const Args &a)
{
    x266_deblock_t p;
    p.d_class = (const uint8_t *)a.p[2]; p.d_intra = (const uint8_t *)a.p[3]; p.d_nnz = (const uint32_t *)a.p[4]; p.d_qp = (const uint8_t *)a.p[5];
    p.d_mv = (const x266_me_result_t *)a.p[6]; p.qp = a.qp; p.beta_offset_div2 = a.beta; p.tc_offset_div2 = a.tc;
    return p;
}

static void build_table()
{
    const std::vector<Ptr> in_out16 = {{"d_in", 16}, {"d_out", 16, OUT}};
    for (const char *n : {"xDct32FwdBatchDev", "xDct32InvBatchDev"})
        CALLS.push_back({n, 0, in_out16, [](const Args &a) { return args::batch(P(0), P(1), 16, a.n); }});
    CALLS.push_back({"xDct32SatdFrameDev", 0, {{"d_dct_in", 16}, {"d_dct_out", 16, OUT}, {"d_diff", 16}, {"d_satd_out", 16, OUT}},
                     [](const Args &a) { return args::dct32_satd_frame(P(0), P(1), a.n, P(2), P(3), a.n); }});
    CALLS.push_back({"xDct32PassDev", 0, in_out16, [](const Args &a) { return args::dct32_pass(P(0), P(1), a.n, a.shift); }});
    CALLS.push_back({"xDct32FwdInvBatchDev", 0, {{"d_in", 16}, {"d_coef", 16, OUT | OPT}, {"d_recon", 16, OUT}},
                     [](const Args &a) { return args::dct32_fwd_inv_batch(P(0), P(1), P(2), a.n); }});
    CALLS.push_back({"xSatd8x8BatchDev", 0, {{"d_diff", 16}, {"d_out", 4, OUT}}, [](const Args &a) { return args::batch(P(0), P(1), 4, a.n); }});
    CALLS.push_back({"xHipMemCeilingDev", 0, {{"d_src", 16}, {"d_dst", 16, OUT}}, [](const Args &a) { return args::mem_ceiling(X266_MEM_COPY, P(0), P(1), a.n * 16); }});
    CALLS.push_back({"xIntra32PredictDev", 0, {{"d_refs", 16}, {"d_modes", 1}, {"d_ref_index", 4, OPT}, {"d_pred", 16, OUT}},
                     [](const Args &a) { return args::intra32_predict(P(0), P(1), P(2), P(3), a.n); }});
    CALLS.push_back({"xIntra32ResidualDct32Dev", 0, {{"d_refs", 16}, {"d_modes", 1}, {"d_ref_index", 4, OPT}, {"d_src", 16}, {"d_coef", 16, OUT}},
                     [](const Args &a) { return args::intra32_residual_dct32(P(0), P(1), P(2), P(3), P(4), a.n); }});
    CALLS.push_back({"xIntra32CostsDev", 0, {{"d_refs", 16}, {"d_src", 16}, {"d_costs", 4, OUT}, {"d_best_mode", 1, OUT | OPT}},
                     [](const Args &a) { return args::intra32_costs(P(0), P(1), P(2), P(3), a.n); }});
    CALLS.push_back({"xFillResidualDev", 0, {{"d_dst", 16, OUT}}, [](const Args &a) { return args::fill_residual(P(0), a.n); }});
    for (const char *n : {"xTransformFwdBatchDev", "xTransformInvBatchDev"})
        CALLS.push_back({n, 0, {{"d_in", 16}, {"d_out", 16, OUT}, {"d_offsets", 4, OPT}},
                         [](const Args &a) { return args::transform_batch(X266_TR_DST7, 8, P(0), P(1), a.n, P(2)); }});
    CALLS.push_back({"xTransformTilesDev", 0, {{"d_in", 16}, {"d_out", 16, OUT}, {"d_tile_offsets", 4, OPT}, {"d_tile_class", 1}},
                     [](const Args &a) { return args::transform_tiles(P(0), P(1), a.n, P(2), P(3)); }});
    CALLS.push_back({"xSadBatchDev", 0, {{"d_a", 16}, {"d_b", 16}, {"d_out", 4, OUT}}, [](const Args &a) { return args::sad_batch(8, P(0), P(1), P(2), a.n); }});

    const std::vector<Ptr> planes = {{"d_tiles", 16}, {"d_y", 16}, {"d_u", 8}, {"d_v", 8}};
    CALLS.push_back({"xConvInputFmtDev", 16, planes, [](const Args &a) { return args::tile_convert(true, P(0), P(1), P(2), P(3), a.w, 0, a.w, a.h); }});
    CALLS.push_back({"xConvOutput420Dev", 16, planes, [](const Args &a) { return args::tile_convert(false, P(0), P(1), P(2), P(3), a.w, a.w / 2, a.w, a.h); }});
    CALLS.push_back({"xResidualLumaDev", 16, {{"d_cur", 16}, {"d_pred", 16}, {"d_residual", 16, OUT}},
                     [](const Args &a) { return args::residual_luma(P(0), P(1), a.w, a.h, 8, P(2)); }});
    CALLS.push_back({"xDct32FwdFromTilesDev", 32, {{"d_cur", 16}, {"d_pred", 16}, {"d_coef", 16, OUT}},
                     [](const Args &a) { return args::from_tiles(P(0), P(1), a.w, a.h, 32, P(2), 16); }});
    CALLS.push_back({"xSatd8x8FromTilesDev", 16, {{"d_cur", 16}, {"d_pred", 16}, {"d_out", 4, OUT}},
                     [](const Args &a) { return args::from_tiles(P(0), P(1), a.w, a.h, 16, P(2), 4); }});
    CALLS.push_back({"xDct32FwdCtuFromTilesDev", 64, {{"d_cur", 16}, {"d_pred", 16}, {"d_coef", 16, OUT}},
                     [](const Args &a) { return args::from_tiles(P(0), P(1), a.w, a.h, 64, P(2), 16); }});
    CALLS.push_back({"xResidualChromaDev", 16, {{"d_cur", 16}, {"d_pred", 16}, {"d_res_u", 16, OUT}, {"d_res_v", 16, OUT}},
                     [](const Args &a) { return args::chroma_from_tiles(P(0), P(1), a.w, a.h, 8, P(2), P(3), 16, 128, 1); }, false, true});
    CALLS.push_back({"xDct32FwdChromaFromTilesDev", 64, {{"d_cur", 16}, {"d_pred", 16}, {"d_coef_u", 16, OUT}, {"d_coef_v", 16, OUT}},
                     [](const Args &a) { return args::chroma_from_tiles(P(0), P(1), a.w, a.h, 32, P(2), P(3), 16, 2048, 1); }, false, true});
    CALLS.push_back({"xSatd8x8ChromaFromTilesDev", 16, {{"d_cur", 16}, {"d_pred", 16}, {"d_out_u", 4, OUT}, {"d_out_v", 4, OUT}},
                     [](const Args &a) { return args::chroma_from_tiles(P(0), P(1), a.w, a.h, 8, P(2), P(3), 4, 4, 1); }, false, true});

    CALLS.push_back({"xReconLumaDev", 16, {{"d_pred", 16, UNFIT, TB}, {"d_residual", 16, UNFIT, TB}, {"d_recon", 16, OUT | UNFIT, TB, "d_pred"}},
                     [](const Args &a) { return args::recon_luma(P(0), P(1), a.w, a.h, 8, P(2)); }});
    CALLS.push_back({"xReconChromaDev", 16, {{"d_pred", 16, UNFIT, TB}, {"d_res_u", 16, 0, CHROMA8}, {"d_res_v", 16, 0, CHROMA8}, {"d_recon", 16, OUT | UNFIT, TB, "d_pred"}},
                     [](const Args &a) { return args::recon_chroma(P(0), P(1), P(2), 1, a.w, a.h, 8, P(3)); }});
    CALLS.push_back({"xDct32InvToTilesDev", 32, {{"d_coef", 16, UNFIT, TB}, {"d_pred", 16, UNFIT, TB}, {"d_recon", 16, OUT | UNFIT, TB, "d_pred"}},
                     [](const Args &a) { return args::inv_to_tiles(P(0), P(1), a.w, a.h, 32, P(2)); }});
    CALLS.push_back({"xDct32InvCtuToTilesDev", 64, {{"d_coef", 16, UNFIT, CT12K}, {"d_pred", 16, UNFIT, TB}, {"d_recon", 16, OUT | UNFIT, TB, "d_pred"}},
                     [](const Args &a) { return args::inv_to_tiles(P(0), P(1), a.w, a.h, 64, P(2)); }});
    CALLS.push_back({"xTransformCtuFromTilesDev", 16, {{"d_cur", 16, 0, TB}, {"d_pred", 16, 0, TB}, {"d_class", 1, 0, CT6}, {"d_coef", 16, OUT, CT12K}},
                     [](const Args &a) { return args::transform_ctu_from_tiles(P(0), P(1), a.w, a.h, P(2), P(3)); }});
    CALLS.push_back({"xTransformCtuToTilesDev", 16, {{"d_coef", 16, 0, CT12K}, {"d_class", 1, 0, CT6}, {"d_pred", 16, 0, TB}, {"d_recon", 16, OUT, TB, "d_pred"}},
                     [](const Args &a) { return args::transform_ctu_to_tiles(P(0), P(1), P(2), a.w, a.h, P(3)); }});

    CALLS.push_back({"xSatd8x8SearchDev", 8, {{"d_cur", 1}, {"d_ref", 1}, {"d_best", 8, OUT}, {"d_costs", 4, OUT | OPT}},
                     [](const Args &a) { return args::plane_search(false, P(0), a.w, P(1), a.w + 2 * a.range, a.w, a.h, a.range, P(2), P(3)); }});
    CALLS.push_back({"xSad8x8SearchDev", 8, {{"d_cur", 4}, {"d_ref", 1}, {"d_best", 8, OUT}, {"d_costs", 4, OUT | OPT}},
                     [](const Args &a) { return args::plane_search(true, P(0), a.w, P(1), a.w + 2 * a.range, a.w, a.h, a.range, P(2), P(3)); }});
    // today's behaviour: each output is held against the two frames only, and only the cost map's end against the address space
    for (const char *n : {"xSatd8x8SearchFromTilesDev", "xSad8x8SearchFromTilesDev"})
        CALLS.push_back({n, 16, {{"d_cur", 16, UNFIT, TB}, {"d_ref", 16, UNFIT, TB}, {"d_best", 8, OUT | UNFIT, B8, nullptr, "d_costs"}, {"d_costs", 4, OUT | OPT, COSTS, nullptr, "d_best"}},
                         [](const Args &a) { return args::tile_search(P(0), P(1), a.w, a.h, a.range, P(2), P(3)); }});
    for (const char *n : {"xMotionCompLumaDev", "xMotionCompChromaDev", "xMotionCompDev"})
        CALLS.push_back({n, 16, {{"d_ref", 16, UNFIT, TB}, {"d_mv", 8, UNFIT, B8}, {"d_pred", 16, OUT | UNFIT, TB}},
                         [](const Args &a) { return args::motion_comp(false, P(0), P(1), a.w, a.h, P(2)); }});
    for (const char *n : {"xMotionCompQpelLumaGpu", "xMotionCompQpelChromaGpu", "xMotionCompQpelGpu"})
        CALLS.push_back({n, 16, {{"d_ref", 16, 0, TB}, {"d_mv", 8, 0, B8}, {"d_pred", 16, OUT, TB}}, [](const Args &a) { return args::motion_comp(true, P(0), P(1), a.w, a.h, P(2)); }});
    CALLS.push_back({"xSatd8x8RefineQpelFromTilesGpu", 16, {{"d_cur", 16, 0, TB}, {"d_ref", 16, 0, TB}, {"d_int", 8, 0, B8}, {"d_best", 8, OUT, B8, "d_int"}, {"d_costs", 4, OUT | OPT, COSTS49}},
                     [](const Args &a) { return args::refine_qpel(P(0), P(1), a.w, a.h, P(2), P(3), P(4)); }});
    CALLS.push_back({"xMotionCompBiQpelTiles", 16, {{"d_ref0", 16, 0, TB}, {"d_ref1", 16, 0, TB}, {"d_mv0", 8, 0, B8}, {"d_mv1", 8, 0, B8}, {"d_dir", 1, OPT, B8x1}, {"d_pred", 16, OUT, TB}},
                     [](const Args &a) { return args::mc_bi_qpel(P(0), P(1), P(2), P(3), P(4), a.wp, a.planes, a.w, a.h, P(5)); }});
    CALLS.push_back({"xSatd8x8BiCostsFromTiles", 16, {{"d_cur", 16, 0, TB}, {"d_ref0", 16, 0, TB}, {"d_ref1", 16, 0, TB}, {"d_mv0", 8, 0, B8}, {"d_mv1", 8, 0, B8},
                     {"d_costs", 4, OUT | OPT, B8x12}, {"d_dir", 1, OUT | OPT, B8x1}},
                     [](const Args &a) { return args::bi_costs(P(0), P(1), P(2), a.w, a.h, P(3), P(4), a.wp, a.bi_penalty, P(5), P(6)); }});
    CALLS.push_back({"xSatd8x8RefineBiQpelFromTiles", 16, {{"d_cur", 16, 0, TB}, {"d_ref_fix", 16, 0, TB}, {"d_mv_fix", 8, 0, B8}, {"d_ref", 16, 0, TB}, {"d_int", 8, 0, B8},
                     {"d_best", 8, OUT, B8, "d_int"}, {"d_costs", 4, OUT | OPT, COSTS49}},
                     [](const Args &a) { return args::refine_bi_qpel(P(0), P(1), P(2), P(3), P(4), a.list, a.wp, a.w, a.h, P(5), P(6)); }});

    CALLS.push_back({"xQuantRegionsGpu", 0, {{"d_in", 16, 0, N2048}, {"d_out", 16, OUT, N2048, "d_in"}, {"d_class", 1, OPT, N1}, {"d_qp", 1, OPT, N1}, {"d_nnz", 4, OUT | OPT, N4}},
                     [](const Args &a) { return args::quant_regions(0, P(0), P(1), a.n, P(2), P(3), a.qp, a.rounding, P(4)); }});
    CALLS.push_back({"xDct32CodeCtuTilesGpu", 64, {{"d_cur", 16, 0, TB}, {"d_pred", 16, 0, TB}, {"d_qp", 1, OPT, CT6}, {"d_level", 16, OUT, CT12K}, {"d_nnz", 4, OUT | OPT, CT24},
                     {"d_recon", 16, OUT, TB, "d_pred"}},
                     [](const Args &a) { return args::dct32_code_ctu_tiles(P(0), P(1), a.w, a.h, P(2), a.qp, a.rounding, P(3), P(4), P(5)); }});
    for (const char *n : {"xDeblockLumaGpu", "xDeblockChromaGpu", "xDeblockGpu"})
        CALLS.push_back({n, 16, {{"d_in", 16, 0, TB}, {"d_out", 16, OUT, TB, "d_in"}, {"d_class", 1, OPT, CT6}, {"d_intra", 1, OPT, CT6}, {"d_nnz", 4, OPT, CT24}, {"d_qp", 1, OPT, CT6},
                         {"d_mv", 8, OPT, B8}}, [](const Args &a) { const x266_deblock_t p = deblock_params(a); return args::deblock(P(0), a.w, a.h, &p, P(1)); }});
    CALLS.push_back({"xSaoStatsGpu", 16, {{"d_org", 16, 0, TB}, {"d_dec", 16, 0, TB}, {"d_stats", 4, OUT, CT1152}},
                     [](const Args &a) { return args::sao_stats(false, P(0), P(1), a.w, a.h, 0, nullptr, P(2)); }});
    CALLS.push_back({"xSaoSearchGpu", 16, {{"d_org", 16, 0, TB}, {"d_dec", 16, 0, TB}, {"d_param", 8, OUT, CT24}, {"d_stats", 4, OUT | OPT, CT1152}},
                     [](const Args &a) { return args::sao_stats(true, P(0), P(1), a.w, a.h, a.lambda_q4, P(2), P(3)); }});
    CALLS.push_back({"xSaoDecideGpu", 0, {{"d_stats", 4, 0, N1152}, {"d_param", 8, OUT, N24}}, [](const Args &a) { return args::sao_decide(P(0), a.n, a.lambda_q4, P(1)); }, true});
    CALLS.push_back({"xSaoApplyGpu", 16, {{"d_in", 16, 0, TB}, {"d_param", 8, 0, CT24}, {"d_out", 16, OUT, TB}}, [](const Args &a) { return args::sao_apply(P(0), a.w, a.h, P(1), P(2)); }});
    CALLS.push_back({"xAlfClassifyGpu", 16, {{"d_dec", 16, 0, TB}, {"d_class", 1, OUT, B4x1}}, [](const Args &a) { return args::alf_classify(P(0), a.w, a.h, P(1)); }});
    CALLS.push_back({"xAlfStatsGpu", 16, {{"d_org", 16, 0, TB}, {"d_dec", 16, 0, TB}, {"d_class", 1, OPT, B4x1}, {"d_stats", 4, OUT, CT9432}},
                     [](const Args &a) { return args::alf_stats(P(0), P(1), a.w, a.h, P(2), P(3)); }});
    CALLS.push_back({"xAlfSumStatsGpu", 0, {{"d_stats", 4, 0, N9432}, {"d_mask", 1, OPT, N1}, {"d_total", 8, OUT, TOTAL}},
                     [](const Args &a) { return args::alf_sum_stats(P(0), a.n, P(1), P(2)); }, true});
    CALLS.push_back({"xAlfDecideGpu", 0, {{"d_stats", 4, 0, N9432}, {"d_luma", 4, 0, LUMA}, {"d_chroma", 4, 0, CHROMA}, {"d_ctrl", 1, OUT, N3}},
                     [](const Args &a) { return args::alf_decide(P(0), a.n, P(1), a.n_luma, P(2), a.n_chroma, a.lambda_q4, P(3)); }, true});
    CALLS.push_back({"xAlfApplyGpu", 16, {{"d_in", 16, 0, TB}, {"d_class", 1, OPT, B4x1}, {"d_luma", 4, 0, LUMA}, {"d_chroma", 4, 0, CHROMA}, {"d_ctrl", 1, 0, CT3}, {"d_out", 16, OUT, TB}},
                     [](const Args &a) { return args::alf_apply(P(0), a.w, a.h, P(1), P(2), a.n_luma, P(3), a.n_chroma, P(4), P(5)); }});
    CALLS.push_back({"xIntra32RefsFromTilesGpu", 64, {{"d_frame", 16, 0, TB}, {"d_refs", 16, OUT, REFS}},
                     [](const Args &a) { return args::intra32_refs_from_tiles(P(0), a.w, a.h, a.component, P(1)); }});
    CALLS.push_back({"xIntra32CodeFrameGpu", 64, {{"d_cur", 16, 0, TB}, {"d_qp", 1, OPT, CT6}, {"d_mode_in", 1, OPT, CT6}, {"d_level", 16, OUT, CT12K}, {"d_nnz", 4, OUT | OPT, CT24},
                     {"d_mode", 1, OUT, CT6, "d_mode_in"}, {"d_recon", 16, OUT, TB}},
                     [](const Args &a) { return args::intra32_code_frame(P(0), a.w, a.h, P(1), a.qp, a.rounding, P(2), P(3), P(4), P(5), P(6)); }});
}

// ---- scalars, strides and the rules that are a call's own --------------------------------------------------------------------------
// one scalar of the bag one step inside and outside its range; null_at: with that pointer NULL
static void scalar(const Call &c, const char *what, int Args::*field, int lo, int hi, const char *reason = nullptr, int null_at = -1)
{
    range(c.name, what, lo, hi, [&](int v) { Args a = base(c); a.*field = v; if (null_at >= 0) a.p[null_at] = 0; return c.rule(a); }, reason);
}
static void qp_rule(const Call &c, int d_qp_at)
{
    scalar(c, "qp without d_qp", &Args::qp, 0, 51, nullptr, d_qp_at);
    Args a = base(c);
    a.qp = 99;
    expect(c.name, "qp 99 with d_qp", c.rule(a), false);
}
static void n_ctu_bounds(const Call &c)
{
    Args a = base(c);
    a.n = (size_t)0x7FFFFFFF;
    expect(c.name, "n_ctu 2^31 - 1", c.rule(a), false);
    a.n = (size_t)0x80000000ull;
    expect(c.name, "n_ctu 2^31", c.rule(a), true, "n_ctu must be below 2^31");
    a.n = ~(size_t)0;
    expect(c.name, "n_ctu 2^64 - 1", c.rule(a), true, "n_ctu must be below 2^31");
}

static void chroma_rule(const char *n, size_t block_bytes, const std::function<const char *(const Args &, size_t pitch)> &f)
{
    const Args one = base(call(n)), six = base(call(n), 3, 2);                 // one block per plane, six blocks per plane
    Args a = one;
    expect(n, "pitch 0", f(a, 0), true, args::kChroma);
    expect(n, "disjoint streams", f(six, 1), false);
    a = six;
    a.p[3] = a.p[2] + block_bytes;
    expect(n, "V one block after U, pitch 2", f(a, 2), false);
    expect(n, "V inside U's span, pitch 1", f(a, 1), true, args::kChroma);
    a.p[3] = a.p[2] + 6 * block_bytes;
    expect(n, "V behind U's span, pitch 1", f(a, 1), false);
    a.p[3] = a.p[2] + block_bytes / 2;
    expect(n, "V half a block after U, pitch 2", f(a, 2), true);              // (or misaligned, where half a block is)
    a.p[3] = a.p[2] + 2 * block_bytes;
    expect(n, "V two blocks after U, pitch 2", f(a, 2), true, args::kChroma);
    expect(n, "V two blocks after U, pitch 3", f(a, 3), false);
}

// every x266_wp_t field at the ends of its range and one step outside
static void weights(const Call &c)
{
    const x266_wp_t ok = {{{-128, 127, 1}, {0, -128, 127}}, {{127, -128, 0}, {-128, 127, 5}}, {0, 7}};
    Args a = base(c);
    a.wp = &ok;
    expect(c.name, "wp at the ends of every range", c.rule(a), false);
    x266_wp_t bad;
    a.wp = &bad;
    for (int l = 0; l < 2; ++l)
        for (int k = 0; k < 3; ++k)
            for (int v : {-129, 128, 32767, -32768}) {
                bad = ok;
                bad.w[l][k] = (int16_t)v;
                expect(c.name, "wp.w out of range", c.rule(a), true, args::kWp);
                bad = ok;
                bad.o[l][k] = (int16_t)v;
                expect(c.name, "wp.o out of range", c.rule(a), true, args::kWp);
            }
    for (int k = 0; k < 2; ++k)
        for (int v : {8, 255}) {
            bad = ok;
            bad.log2_denom[k] = (uint8_t)v;
            expect(c.name, "wp.log2_denom out of range", c.rule(a), true, args::kWp);
        }
}

// the ALF set arrays: each count 0..8, and a count of 0 with any pointer at all
static void counts(const Call &c, size_t luma_at, size_t chroma_at)
{
    scalar(c, "n_luma", &Args::n_luma, 0, 8, args::kAlfCounts);
    scalar(c, "n_chroma", &Args::n_chroma, 0, 8, args::kAlfCounts);
    for (U junk : {(U)0, (U)3, ~(U)0}) {
        Args a = base(c);
        a.n_luma = 0;
        a.p[luma_at] = junk;
        expect(c.name, "n_luma 0 with d_luma " + std::to_string(junk), c.rule(a), false);
        a = base(c);
        a.n_chroma = 0;
        a.p[chroma_at] = junk;
        expect(c.name, "n_chroma 0 with d_chroma " + std::to_string(junk), c.rule(a), false);
    }
}

static void own_rules()
{
    const char *n = "xDct32PassDev";
    scalar(call(n), "shift", &Args::shift, 1, 15);
    expect(n, "shift 0, n == 0", args::dct32_pass(nullptr, nullptr, 0, 0), true);

    n = "xDct32SatdFrameDev";
    { Args a = base(call(n)); expect(n, "NULL SATD half with n_satd_blocks == 0", args::dct32_satd_frame(P(0), P(1), 3, nullptr, nullptr, 0), false);
      expect(n, "NULL DCT half with n_dct_blocks == 0", args::dct32_satd_frame(nullptr, nullptr, 0, P(2), P(3), 3), false); }

    n = "xHipMemCeilingDev";
    { const Args a = base(call(n));
      range(n, "kind", X266_MEM_COPY, X266_MEM_READ_PROBE, [&](int v) { return args::mem_ceiling(v, P(0), P(1), 64); });
      expect(n, "bytes 24", args::mem_ceiling(X266_MEM_COPY, P(0), P(1), 24), true);
      expect(n, "bytes 0, NULL", args::mem_ceiling(X266_MEM_COPY, nullptr, nullptr, 0), false);
      expect(n, "WRITE, d_src NULL", args::mem_ceiling(X266_MEM_WRITE, nullptr, P(1), 64), false);
      expect(n, "WRITE, d_src misaligned", args::mem_ceiling(X266_MEM_WRITE, V(a.p[0] + 1), P(1), 64), false);
      expect(n, "READ, d_dst NULL", args::mem_ceiling(X266_MEM_READ, P(0), nullptr, 64), true, args::kNull); }

    for (const char *t : {"xTransformFwdBatchDev", "xTransformInvBatchDev"}) {
        const Args a = base(call(t));
        range(t, "type", 0, 3, [&](int v) { return args::transform_batch(v, 8, P(0), P(1), a.n, P(2)); });
        for (int size : {4, 8, 16}) expect(t, "size " + std::to_string(size), args::transform_batch(X266_TR_DCT2_DST7, size, P(0), P(1), a.n, P(2)), false);
        for (int size : {0, 2, 12, 64}) expect(t, "size " + std::to_string(size), args::transform_batch(X266_TR_DCT2, size, P(0), P(1), a.n, P(2)), true);
        expect(t, "size 32, DCT-II", args::transform_batch(X266_TR_DCT2, 32, P(0), P(1), a.n, P(2)), false);
        expect(t, "size 32, DST-VII", args::transform_batch(X266_TR_DST7, 32, P(0), P(1), a.n, P(2)), true);
        expect(t, "bad type, n == 0", args::transform_batch(4, 8, nullptr, nullptr, 0, nullptr), true);
    }
    n = "xSadBatchDev";
    { const Args a = base(call(n));
      for (int e : {4, 8, 16, 32, 64}) expect(n, "edge " + std::to_string(e), args::sad_batch(e, P(0), P(1), P(2), a.n), false);
      for (int e : {0, 2, 12, 128, -8}) expect(n, "edge " + std::to_string(e), args::sad_batch(e, P(0), P(1), P(2), a.n), true); }

    n = "xConvInputFmtDev";
    { const Args a = base(call(n), 3, 2);
      auto f = [&](intptr_t sy) { return args::tile_convert(true, P(0), P(1), P(2), P(3), sy, 0, a.w, a.h); };
      expect(n, "strdY = width + 16", f(a.w + 16), false);
      expect(n, "strdY = width - 16", f(a.w - 16), true);
      expect(n, "strdY = width + 8", f(a.w + 8), true); }
    n = "xConvOutput420Dev";
    { const Args a = base(call(n), 3, 2);
      auto f = [&](intptr_t sy, intptr_t sc) { return args::tile_convert(false, P(0), P(1), P(2), P(3), sy, sc, a.w, a.h); };
      expect(n, "strdC = width / 2 + 8", f(a.w, a.w / 2 + 8), false);
      expect(n, "strdC = width / 2 - 8", f(a.w, a.w / 2 - 8), true);
      expect(n, "strdC = width / 2 + 4", f(a.w, a.w / 2 + 4), true);
      expect(n, "strdY = width - 16", f(a.w - 16, a.w / 2), true);
      expect(n, "strdY = width + 8", f(a.w + 8, a.w / 2), true); }

    // block_edge 8 or 32; a 32x32 luma block needs multiples of 32, a 32x32 chroma block a 64x64 CTU
    n = "xResidualLumaDev";
    { const Args a = base(call(n));
      auto f = [&](int w, int h, int e) { return args::residual_luma(P(0), P(1), w, h, e, P(2)); };
      expect(n, "block_edge 32, 32x32", f(32, 32, 32), false); expect(n, "block_edge 32, 96x64", f(96, 64, 32), false);
      expect(n, "block_edge 32, 48x32", f(48, 32, 32), true); expect(n, "block_edge 32, 32x16", f(32, 16, 32), true);
      expect(n, "block_edge 16", f(32, 32, 16), true); expect(n, "block_edge 0", f(32, 32, 0), true); }
    n = "xReconLumaDev";
    { const Args a = base(call(n));
      auto f = [&](int w, int h, int e) { return args::recon_luma(P(0), P(1), w, h, e, P(2)); };
      expect(n, "block_edge 32, 32x32", f(32, 32, 32), false); expect(n, "block_edge 32, 48x32", f(48, 32, 32), true);
      expect(n, "block_edge 16", f(32, 32, 16), true); }
    n = "xResidualChromaDev";
    { const Args a = base(call(n));
      auto f = [&](int w, int h, int e) { return args::chroma_from_tiles(P(0), P(1), w, h, e, P(2), P(3), 16, (size_t)e * e * 2, 1); };
      expect(n, "block_edge 32, 64x64", f(64, 64, 32), false); expect(n, "block_edge 32, 192x128", f(192, 128, 32), false);
      expect(n, "block_edge 32, 96x64", f(96, 64, 32), true); expect(n, "block_edge 16", f(64, 64, 16), true); }
    n = "xReconChromaDev";
    { const Args a = base(call(n));
      auto f = [&](int w, int h, int e, size_t pitch) { return args::recon_chroma(P(0), P(1), P(2), pitch, w, h, e, P(3)); };
      expect(n, "block_edge 32, 64x64", f(64, 64, 32, 1), false); expect(n, "block_edge 32, 96x64", f(96, 64, 32, 1), true);
      expect(n, "block_edge 16", f(64, 64, 16, 1), true);
      expect(n, "pitch 0", f(16, 16, 8, 0), true);
      expect(n, "pitch 2", f(48, 32, 8, 2), false);
      expect(n, "a pitch whose stream wraps size_t", f(64, 64, 8, SIZE_MAX / 8), true, args::kNoFit);            // 16 blocks per plane
      expect(n, "the same pitch, one block per plane", f(64, 64, 32, SIZE_MAX / 8), false);
      Args b = base(call(n));                                                                                  // 48x32 at pitch 2: 11 blocks of 128 bytes
      b.p[3] = up(b.p[1] + 11 * 128 - 1, 16) - 16;
      expect(n, "d_recon in the last block of a pitched stream", args::recon_chroma(V(b.p[0]), V(b.p[1]), V(b.p[2]), 2, 48, 32, 8, V(b.p[3])), true, args::kOverlap);
      b.p[3] = up(b.p[1] + 11 * 128, 16);
      expect(n, "d_recon behind a pitched stream", args::recon_chroma(V(b.p[0]), V(b.p[1]), V(b.p[2]), 2, 48, 32, 8, V(b.p[3])), false); }

    chroma_rule("xResidualChromaDev", 128, [](const Args &a, size_t pitch) { return args::chroma_from_tiles(P(0), P(1), a.w, a.h, 8, P(2), P(3), 16, 128, pitch); });
    chroma_rule("xDct32FwdChromaFromTilesDev", 2048, [](const Args &a, size_t pitch) { return args::chroma_from_tiles(P(0), P(1), a.w, a.h, 32, P(2), P(3), 16, 2048, pitch); });
    chroma_rule("xSatd8x8ChromaFromTilesDev", 4, [](const Args &a, size_t pitch) { return args::chroma_from_tiles(P(0), P(1), a.w, a.h, 8, P(2), P(3), 4, 4, pitch); });

    for (int sad = 0; sad < 2; ++sad) {
        n = sad ? "xSad8x8SearchDev" : "xSatd8x8SearchDev";
        const Args a = base(call(n), 3, 2);
        auto f = [&](intptr_t cs, intptr_t rs, int r) { return args::plane_search(sad != 0, P(0), cs, P(1), rs, a.w, a.h, r, P(2), P(3)); };
        range(n, "range", 1, 64, [&](int r) { return f(a.w, a.w + 128, r); });
        expect(n, "cur_stride = width - 1", f(a.w - 1, a.w + 8, 4), true);
        expect(n, "cur_stride = width + 4", f(a.w + 4, a.w + 8, 4), false);
        expect(n, "cur_stride = width + 2", f(a.w + 2, a.w + 8, 4), sad != 0);
        expect(n, "ref_stride = width + 2 range - 1", f(a.w, a.w + 7, 4), true);
        expect(n, "ref_stride = width + 2 range + 1", f(a.w, a.w + 9, 4), false);
    }
    for (const char *t : {"xSatd8x8SearchFromTilesDev", "xSad8x8SearchFromTilesDev"}) {
        const Args a = base(call(t));
        scalar(call(t), "range", &Args::range, 1, 64);
        expect(t, "d_cur == d_ref", args::tile_search(P(0), P(0), a.w, a.h, 4, P(2), P(3)), false);
        // a cost map whose size wraps size_t: 2^49 blocks x 129 x 129 x 4 bytes; the frames (2^56 bytes) and d_best (2^52) are placed to fit
        const U cur = ((U)1 << 57) + 16, best = ((U)1 << 59) + 8, costs = ((U)1 << 60) + 4;
        expect(t, "cost map wraps size_t", args::tile_search(V(cur), V(cur), 1 << 28, 1 << 27, 64, V(best), V(costs)), true, args::kNoFit);
        expect(t, "the same frame without a cost map", args::tile_search(V(cur), V(cur), 1 << 28, 1 << 27, 64, V(best), nullptr), false);
    }

    n = "xQuantRegionsGpu";
    { const Args a = base(call(n));
      qp_rule(call(n), 3);
      scalar(call(n), "rounding", &Args::rounding, 0, 511, nullptr, 3);
      expect(n, "inverse with d_nnz", args::quant_regions(1, P(0), P(1), a.n, P(2), P(3), 30, 171, P(4)), true);
      expect(n, "inverse without d_nnz", args::quant_regions(1, P(0), P(1), a.n, P(2), P(3), 30, 171, nullptr), false);
      expect(n, "n_regions == 0, qp 52", args::quant_regions(0, nullptr, nullptr, 0, nullptr, nullptr, 52, 171, nullptr), true);   // scalar errors first
      expect(n, "n_regions == 0, rounding 512", args::quant_regions(0, nullptr, nullptr, 0, nullptr, nullptr, 30, 512, nullptr), true);
      expect(n, "a count whose bytes wrap size_t", args::quant_regions(0, P(0), P(1), SIZE_MAX / 2048 + 1, P(2), P(3), 30, 171, P(4)), true, args::kNoFit);
      expect(n, "a count whose d_nnz bytes wrap size_t", args::quant_regions(0, P(0), P(1), SIZE_MAX / 4 + 1, nullptr, nullptr, 30, 171, P(4)), true, args::kNoFit); }
    n = "xDct32CodeCtuTilesGpu";
    { const Args a = base(call(n));
      qp_rule(call(n), 2);
      scalar(call(n), "rounding", &Args::rounding, 0, 511, nullptr, 2);
      auto f = [&](U cur, U pred, U recon) { return args::dct32_code_ctu_tiles(V(cur), V(pred), a.w, a.h, P(2), 30, 171, P(3), P(4), V(recon)); };
      expect(n, "d_cur == d_pred", f(a.p[1], a.p[1], a.p[5]), false);
      expect(n, "d_cur == d_pred == d_recon", f(a.p[1], a.p[1], a.p[1]), false);
      expect(n, "d_recon == d_cur", f(a.p[0], a.p[1], a.p[0]), true, args::kOverlap);
      expect(n, "d_level on d_cur == d_pred", args::dct32_code_ctu_tiles(P(1), P(1), a.w, a.h, P(2), 30, 171, V(a.p[1] + 16), P(4), P(5)), true, args::kOverlap); }
    n = "xIntra32CodeFrameGpu";
    { const Args a = base(call(n));
      qp_rule(call(n), 1);
      scalar(call(n), "rounding", &Args::rounding, 0, 511, nullptr, 1);
      expect(n, "d_qp == d_mode_in == d_mode", args::intra32_code_frame(P(0), a.w, a.h, P(5), 30, 171, P(5), P(3), P(4), P(5), P(6)), true, args::kOverlap); }
    n = "xIntra32RefsFromTilesGpu";
    { const Args a = base(call(n));
      scalar(call(n), "component", &Args::component, 0, 2);
      // chroma: one reference set per CTU, a quarter of luma's extent
      expect(n, "component 1: a quarter of the luma extent in front of the frame", args::intra32_refs_from_tiles(P(0), a.w, a.h, 1, V(down(a.p[0] - sizeof(x266_intra_ref_t), 16))), false);
      expect(n, "component 0: the same place overlaps", args::intra32_refs_from_tiles(P(0), a.w, a.h, 0, V(down(a.p[0] - sizeof(x266_intra_ref_t), 16))), true, args::kOverlap); }

    for (const char *t : {"xDeblockLumaGpu", "xDeblockChromaGpu", "xDeblockGpu"}) {
        const Args a = base(call(t));
        expect(t, "NULL parameter struct", args::deblock(P(0), a.w, a.h, nullptr, P(1)), true);
        qp_rule(call(t), 5);
        scalar(call(t), "beta_offset_div2", &Args::beta, -6, 6);
        scalar(call(t), "tc_offset_div2", &Args::tc, -6, 6);
    }
    scalar(call("xSaoSearchGpu"), "lambda_q4", &Args::lambda_q4, 0, 65535, "lambda_q4 must be 0..65535");
    n = "xSaoDecideGpu";
    scalar(call(n), "lambda_q4", &Args::lambda_q4, 0, 65535, "lambda_q4 must be 0..65535");
    n_ctu_bounds(call(n));
    { const Args a = base(call(n)); expect(n, "n_ctu 0, lambda_q4 65536", args::sao_decide(P(0), 0, 65536, P(1)), true); }

    // the bi-directional calls: the inputs may be one frame; both outputs of the cost call NULL is refused, either alone is accepted
    for (const char *t : {"xMotionCompBiQpelTiles", "xSatd8x8BiCostsFromTiles", "xSatd8x8RefineBiQpelFromTiles"}) weights(call(t));
    scalar(call("xMotionCompBiQpelTiles"), "planes", &Args::planes, 1, 3);
    scalar(call("xSatd8x8BiCostsFromTiles"), "bi_penalty", &Args::bi_penalty, 0, 65535);
    scalar(call("xSatd8x8RefineBiQpelFromTiles"), "list", &Args::list, 0, 1);
    { const Call &mc = call("xMotionCompBiQpelTiles"), &costs = call("xSatd8x8BiCostsFromTiles"), &refine = call("xSatd8x8RefineBiQpelFromTiles");
      Args a = base(mc);
      a.p[1] = a.p[0];
      expect(mc.name, "d_ref1 == d_ref0", mc.rule(a), false);
      a = base(costs);
      a.p[5] = a.p[6] = 0;
      expect(costs.name, "both outputs NULL", costs.rule(a), true);
      a = base(costs);
      a.p[0] = a.p[1] = a.p[2];
      expect(costs.name, "one frame three times", costs.rule(a), false);
      a = base(refine);
      a.p[1] = a.p[3] = a.p[0];
      expect(refine.name, "one frame three times", refine.rule(a), false);
      a = base(refine);
      a.p[5] = a.p[2];
      expect(refine.name, "d_best == d_mv_fix", refine.rule(a), true, args::kOverlap); }

    // the adaptive loop filter: the two frames of the statistics are read-only and may be one
    { const Call &stats = call("xAlfStatsGpu");
      Args a = base(stats);
      a.p[0] = a.p[1];
      expect(stats.name, "d_org == d_dec", stats.rule(a), false); }
    counts(call("xAlfDecideGpu"), 1, 2);
    counts(call("xAlfApplyGpu"), 2, 3);
    scalar(call("xAlfDecideGpu"), "lambda_q4", &Args::lambda_q4, 0, 65535, "lambda_q4 must be 0..65535");
    n_ctu_bounds(call("xAlfSumStatsGpu"));
    n_ctu_bounds(call("xAlfDecideGpu"));
}

int main()
{
    build_table();
    for (const Call &c : CALLS) {
        generic(c);
        std::printf("%s:", c.name);
        for (const Ptr &p : c.ptrs) std::printf(" %s %u%s", p.name, p.align, &p == &c.ptrs.back() ? "\n" : ",");
    }
    own_rules();
    for (const Call &c : CALLS) std::printf("checks %s %d\n", c.name, g_per_call[c.name]);
    if (g_failures) {
        std::printf("%d of %d checks failed\n", g_failures, g_checks);
        return 1;
    }
    std::printf("%zu entry points, %d checks: the argument rules hold\n", CALLS.size(), g_checks);
    return 0;
}
