// CPU check of the device entry points' argument rules (x266_amd/csrc/x266_args.hpp).  The rule functions are pure integer
// arithmetic on addresses and sizes, so the addresses here are made-up integers: nothing is dereferenced and no device is needed.
//
// CALLS below is the contract written down once more, by hand, from include/x266hip.h and from the checks the entry points
// carried before the rules moved into the header: per entry point every pointer with its alignment, whether it may be NULL,
// whether it is written, its extent where the call's rules have one (none: the older calls check NULL and alignment only, and
// overlapping buffers are ACCEPTED there -- recorded as today's behaviour, so that tightening one is a visible diff of this
// table), whether the span's end is held against the address space, and the exact alias it may form.  The expected verdict of
// every perturbation follows from that table and from the literals in the per-call checks, never from the functions under test.
// Test infrastructure; built and run by tests/test_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "x266_args.hpp"

using namespace x266;

typedef uintptr_t U;
struct Args {
    std::vector<U> p;
    int w = 0, h = 0;       // frame calls
    size_t n = 0;           // batch calls
};
static const void *V(U x) { return (const void *)x; }

typedef size_t (*Extent)(size_t w, size_t h);      // batch calls: (n, 0)
enum { OPT = 1, OUT = 2, UNFIT = 4 };
struct Ptr {
    const char *name;
    unsigned align;
    int flags;
    Extent bytes;            // nullptr: no extent in this call's rules
    const char *alias;       // the input this output may exactly be
    const char *not_vs;      // an output the rules do not hold this one against
};
struct Call {
    const char *name;
    int granule;             // 0: a batch call (n blocks; n == 0 is accepted whatever the pointers are, unless zero_needs_ptrs)
    std::vector<Ptr> ptrs;
    std::function<const char *(const Args &)> rule;     // every scalar at a valid value
    bool zero_needs_ptrs = false;
    bool uv_rule = false;         // the last two pointers are the U / V output streams, which have a rule of their own
};

static int g_checks = 0, g_failures = 0;
static void expect(const char *call, const std::string &what, const char *got, bool refuse, const char *reason = nullptr)
{
    ++g_checks;
    if ((got != nullptr) == refuse && (!reason || !got || !std::strcmp(got, reason))) return;
    ++g_failures;
    std::printf("FAIL %s: %s: expected %s%s%s, got %s\n", call, what.c_str(), refuse ? "refuse" : "accept", reason ? " for " : "", reason ? reason : "",
                got ? got : "accept");
}
static void range(const char *call, const char *what, int lo, int hi, const std::function<const char *(int)> &f)
{
    expect(call, std::string(what) + " below", f(lo - 1), true);
    expect(call, std::string(what) + " lowest", f(lo), false);
    expect(call, std::string(what) + " highest", f(hi), false);
    expect(call, std::string(what) + " above", f(hi + 1), true);
}

// extents, as include/x266hip.h states them
static size_t TB(size_t w, size_t h) { return w * h * 2; }                       // a frame of tiles: 512 bytes per 16x16 pixels
static size_t B8(size_t w, size_t h) { return (w / 8) * (h / 8) * 8; }           // one 8-byte record per 8x8 block
static size_t CT(size_t w, size_t h) { return ((w + 63) / 64) * ((h + 63) / 64); }
static size_t CT6(size_t w, size_t h) { return CT(w, h) * 6; }
static size_t CT24(size_t w, size_t h) { return CT(w, h) * 24; }
static size_t CT12K(size_t w, size_t h) { return CT(w, h) * 12288; }
static size_t CT1152(size_t w, size_t h) { return CT(w, h) * 1152; }
static size_t REFS4(size_t w, size_t h) { return CT(w, h) * 4 * sizeof(x266_intra_ref_t); }
static size_t COSTS4(size_t w, size_t h) { return (w / 8) * (h / 8) * 9 * 9 * 4; }          // range 4
static size_t COSTS49(size_t w, size_t h) { return (w / 8) * (h / 8) * 49 * 4; }
static size_t CHROMA8(size_t w, size_t h) { return (w / 16) * (h / 16) * 128; }             // 8x8 int16 blocks at pitch 1
static size_t N2048(size_t n, size_t) { return n * 2048; }
static size_t N1(size_t n, size_t) { return n; }
static size_t N4(size_t n, size_t) { return n * 4; }
static size_t N24(size_t n, size_t) { return n * 24; }
static size_t N1152(size_t n, size_t) { return n * 1152; }

static U down(U x, unsigned a) { return x - x % a; }
static U up(U x, unsigned a) { return down(x + a - 1, a); }

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
static size_t extent(const Call &c, const Args &a, size_t i) { return c.granule ? c.ptrs[i].bytes((size_t)a.w, (size_t)a.h) : c.ptrs[i].bytes(a.n, 0); }

static void generic(const Call &c)
{
    const char *n = c.name;
    expect(n, "base", c.rule(base(c)), false);
    if (c.granule) expect(n, "second size", c.rule(base(c, 3, 2)), false);
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
                expect(n, std::string(dim ? "height " : "width ") + std::to_string(v), c.rule(a), true);
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
    for (int size = 0; size < (c.granule ? 2 : 1); ++size) {
        const Args b = size ? base(c, 3, 2) : base(c);
        for (size_t o = 0; o < c.ptrs.size(); ++o) {
            const Ptr &po = c.ptrs[o];
            if (!po.bytes) continue;
            const size_t no = extent(c, b, o);
            // the top of the address space: the highest aligned address whose span fits, and the highest aligned address
            Args a = b;
            a.p[o] = down(UINTPTR_MAX - no, po.align);
            expect(n, std::string(po.name) + " ends at the top of the address space", c.rule(a), false);
            a.p[o] = down(UINTPTR_MAX, po.align);
            expect(n, std::string(po.name) + " runs past the top of the address space", c.rule(a), !(po.flags & UNFIT), (po.flags & UNFIT) ? nullptr : args::kNoFit);
            if (!(po.flags & OUT)) continue;
            for (size_t i = 0; i < c.ptrs.size(); ++i) {
                const Ptr &pi = c.ptrs[i];
                if (i == o || !pi.bytes) continue;
                const size_t ni = extent(c, b, i);
                const bool held = !(po.not_vs && !std::strcmp(po.not_vs, pi.name));
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
                const bool alias = po.alias && !std::strcmp(po.alias, pi.name);
                a.p[o] = up(b.p[i], po.align);                      // the two are aligned alike wherever an alias is allowed
                if (alias || a.p[o] == b.p[i]) expect(n, pair + " at the same address", c.rule(a), !alias && held, alias || !held ? nullptr : args::kOverlap);
                if (alias) {
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
static x266_deblock_t deblock_params(const Args &a, int qp = 30, int beta = 0, int tc = 0)
{
    x266_deblock_t p;
    p.d_class = (const uint8_t *)a.p[2]; p.d_intra = (const uint8_t *)a.p[3]; p.d_nnz = (const uint32_t *)a.p[4]; p.d_qp = (const uint8_t *)a.p[5];
    p.d_mv = (const x266_me_result_t *)a.p[6]; p.qp = qp; p.beta_offset_div2 = beta; p.tc_offset_div2 = tc;
    return p;
}

static void build_table()
{
    const std::vector<Ptr> in_out16 = {{"d_in", 16, 0, nullptr, nullptr, nullptr}, {"d_out", 16, OUT, nullptr, nullptr, nullptr}};
    for (const char *n : {"xDct32FwdBatchDev", "xDct32InvBatchDev"})
        CALLS.push_back({n, 0, in_out16, [](const Args &a) { return args::batch(P(0), P(1), 16, a.n); }});
    CALLS.push_back({"xDct32SatdFrameDev", 0, {{"d_dct_in", 16, 0, nullptr, nullptr, nullptr}, {"d_dct_out", 16, OUT, nullptr, nullptr, nullptr},
                     {"d_diff", 16, 0, nullptr, nullptr, nullptr}, {"d_satd_out", 16, OUT, nullptr, nullptr, nullptr}},
                     [](const Args &a) { return args::dct32_satd_frame(P(0), P(1), a.n, P(2), P(3), a.n); }});
    CALLS.push_back({"xDct32PassDev", 0, in_out16, [](const Args &a) { return args::dct32_pass(P(0), P(1), a.n, 7); }});
    CALLS.push_back({"xDct32FwdInvBatchDev", 0, {{"d_in", 16, 0, nullptr, nullptr, nullptr}, {"d_coef", 16, OUT | OPT, nullptr, nullptr, nullptr},
                     {"d_recon", 16, OUT, nullptr, nullptr, nullptr}}, [](const Args &a) { return args::dct32_fwd_inv_batch(P(0), P(1), P(2), a.n); }});
    CALLS.push_back({"xSatd8x8BatchDev", 0, {{"d_diff", 16, 0, nullptr, nullptr, nullptr}, {"d_out", 4, OUT, nullptr, nullptr, nullptr}},
                     [](const Args &a) { return args::batch(P(0), P(1), 4, a.n); }});
    CALLS.push_back({"xHipMemCeilingDev", 0, {{"d_src", 16, 0, nullptr, nullptr, nullptr}, {"d_dst", 16, OUT, nullptr, nullptr, nullptr}},
                     [](const Args &a) { return args::mem_ceiling(X266_MEM_COPY, P(0), P(1), a.n * 16); }});
    CALLS.push_back({"xIntra32PredictDev", 0, {{"d_refs", 16, 0, nullptr, nullptr, nullptr}, {"d_modes", 1, 0, nullptr, nullptr, nullptr},
                     {"d_ref_index", 4, OPT, nullptr, nullptr, nullptr}, {"d_pred", 16, OUT, nullptr, nullptr, nullptr}},
                     [](const Args &a) { return args::intra32_predict(P(0), P(1), P(2), P(3), a.n); }});
    CALLS.push_back({"xIntra32ResidualDct32Dev", 0, {{"d_refs", 16, 0, nullptr, nullptr, nullptr}, {"d_modes", 1, 0, nullptr, nullptr, nullptr},
                     {"d_ref_index", 4, OPT, nullptr, nullptr, nullptr}, {"d_src", 16, 0, nullptr, nullptr, nullptr}, {"d_coef", 16, OUT, nullptr, nullptr, nullptr}},
                     [](const Args &a) { return args::intra32_residual_dct32(P(0), P(1), P(2), P(3), P(4), a.n); }});
    CALLS.push_back({"xIntra32CostsDev", 0, {{"d_refs", 16, 0, nullptr, nullptr, nullptr}, {"d_src", 16, 0, nullptr, nullptr, nullptr},
                     {"d_costs", 4, OUT, nullptr, nullptr, nullptr}, {"d_best_mode", 1, OUT | OPT, nullptr, nullptr, nullptr}},
                     [](const Args &a) { return args::intra32_costs(P(0), P(1), P(2), P(3), a.n); }});
    CALLS.push_back({"xFillResidualDev", 0, {{"d_dst", 16, OUT, nullptr, nullptr, nullptr}}, [](const Args &a) { return args::fill_residual(P(0), a.n); }});
    for (const char *n : {"xTransformFwdBatchDev", "xTransformInvBatchDev"})
        CALLS.push_back({n, 0, {{"d_in", 16, 0, nullptr, nullptr, nullptr}, {"d_out", 16, OUT, nullptr, nullptr, nullptr}, {"d_offsets", 4, OPT, nullptr, nullptr, nullptr}},
                         [](const Args &a) { return args::transform_batch(X266_TR_DST7, 8, P(0), P(1), a.n, P(2)); }});
    CALLS.push_back({"xTransformTilesDev", 0, {{"d_in", 16, 0, nullptr, nullptr, nullptr}, {"d_out", 16, OUT, nullptr, nullptr, nullptr},
                     {"d_tile_offsets", 4, OPT, nullptr, nullptr, nullptr}, {"d_tile_class", 1, 0, nullptr, nullptr, nullptr}},
                     [](const Args &a) { return args::transform_tiles(P(0), P(1), a.n, P(2), P(3)); }});
    CALLS.push_back({"xSadBatchDev", 0, {{"d_a", 16, 0, nullptr, nullptr, nullptr}, {"d_b", 16, 0, nullptr, nullptr, nullptr}, {"d_out", 4, OUT, nullptr, nullptr, nullptr}},
                     [](const Args &a) { return args::sad_batch(8, P(0), P(1), P(2), a.n); }});

    const std::vector<Ptr> planes = {{"d_tiles", 16, 0, nullptr, nullptr, nullptr}, {"d_y", 16, 0, nullptr, nullptr, nullptr}, {"d_u", 8, 0, nullptr, nullptr, nullptr},
                                     {"d_v", 8, 0, nullptr, nullptr, nullptr}};
    CALLS.push_back({"xConvInputFmtDev", 16, planes, [](const Args &a) { return args::tile_convert(true, P(0), P(1), P(2), P(3), a.w, 0, a.w, a.h); }});
    CALLS.push_back({"xConvOutput420Dev", 16, planes, [](const Args &a) { return args::tile_convert(false, P(0), P(1), P(2), P(3), a.w, a.w / 2, a.w, a.h); }});
    CALLS.push_back({"xResidualLumaDev", 16, {{"d_cur", 16, 0, nullptr, nullptr, nullptr}, {"d_pred", 16, 0, nullptr, nullptr, nullptr}, {"d_residual", 16, OUT, nullptr, nullptr, nullptr}},
                     [](const Args &a) { return args::residual_luma(P(0), P(1), a.w, a.h, 8, P(2)); }});
    CALLS.push_back({"xDct32FwdFromTilesDev", 32, {{"d_cur", 16, 0, nullptr, nullptr, nullptr}, {"d_pred", 16, 0, nullptr, nullptr, nullptr}, {"d_coef", 16, OUT, nullptr, nullptr, nullptr}},
                     [](const Args &a) { return args::from_tiles(P(0), P(1), a.w, a.h, 32, P(2), 16); }});
    CALLS.push_back({"xSatd8x8FromTilesDev", 16, {{"d_cur", 16, 0, nullptr, nullptr, nullptr}, {"d_pred", 16, 0, nullptr, nullptr, nullptr}, {"d_out", 4, OUT, nullptr, nullptr, nullptr}},
                     [](const Args &a) { return args::from_tiles(P(0), P(1), a.w, a.h, 16, P(2), 4); }});
    CALLS.push_back({"xDct32FwdCtuFromTilesDev", 64, {{"d_cur", 16, 0, nullptr, nullptr, nullptr}, {"d_pred", 16, 0, nullptr, nullptr, nullptr}, {"d_coef", 16, OUT, nullptr, nullptr, nullptr}},
                     [](const Args &a) { return args::from_tiles(P(0), P(1), a.w, a.h, 64, P(2), 16); }});
    CALLS.push_back({"xResidualChromaDev", 16, {{"d_cur", 16, 0, nullptr, nullptr, nullptr}, {"d_pred", 16, 0, nullptr, nullptr, nullptr}, {"d_res_u", 16, OUT, nullptr, nullptr, nullptr},
                     {"d_res_v", 16, OUT, nullptr, nullptr, nullptr}}, [](const Args &a) { return args::chroma_from_tiles(P(0), P(1), a.w, a.h, 8, P(2), P(3), 16, 128, 1); }, false, true});
    CALLS.push_back({"xDct32FwdChromaFromTilesDev", 64, {{"d_cur", 16, 0, nullptr, nullptr, nullptr}, {"d_pred", 16, 0, nullptr, nullptr, nullptr}, {"d_coef_u", 16, OUT, nullptr, nullptr, nullptr},
                     {"d_coef_v", 16, OUT, nullptr, nullptr, nullptr}}, [](const Args &a) { return args::chroma_from_tiles(P(0), P(1), a.w, a.h, 32, P(2), P(3), 16, 2048, 1); }, false, true});
    CALLS.push_back({"xSatd8x8ChromaFromTilesDev", 16, {{"d_cur", 16, 0, nullptr, nullptr, nullptr}, {"d_pred", 16, 0, nullptr, nullptr, nullptr}, {"d_out_u", 4, OUT, nullptr, nullptr, nullptr},
                     {"d_out_v", 4, OUT, nullptr, nullptr, nullptr}}, [](const Args &a) { return args::chroma_from_tiles(P(0), P(1), a.w, a.h, 8, P(2), P(3), 4, 4, 1); }, false, true});

    CALLS.push_back({"xReconLumaDev", 16, {{"d_pred", 16, UNFIT, TB, nullptr, nullptr}, {"d_residual", 16, UNFIT, TB, nullptr, nullptr}, {"d_recon", 16, OUT | UNFIT, TB, "d_pred", nullptr}},
                     [](const Args &a) { return args::recon_luma(P(0), P(1), a.w, a.h, 8, P(2)); }});
    CALLS.push_back({"xReconChromaDev", 16, {{"d_pred", 16, UNFIT, TB, nullptr, nullptr}, {"d_res_u", 16, 0, CHROMA8, nullptr, nullptr}, {"d_res_v", 16, 0, CHROMA8, nullptr, nullptr},
                     {"d_recon", 16, OUT | UNFIT, TB, "d_pred", nullptr}}, [](const Args &a) { return args::recon_chroma(P(0), P(1), P(2), 1, a.w, a.h, 8, P(3)); }});
    CALLS.push_back({"xDct32InvToTilesDev", 32, {{"d_coef", 16, UNFIT, TB, nullptr, nullptr}, {"d_pred", 16, UNFIT, TB, nullptr, nullptr}, {"d_recon", 16, OUT | UNFIT, TB, "d_pred", nullptr}},
                     [](const Args &a) { return args::inv_to_tiles(P(0), P(1), a.w, a.h, 32, P(2)); }});
    CALLS.push_back({"xDct32InvCtuToTilesDev", 64, {{"d_coef", 16, UNFIT, CT12K, nullptr, nullptr}, {"d_pred", 16, UNFIT, TB, nullptr, nullptr}, {"d_recon", 16, OUT | UNFIT, TB, "d_pred", nullptr}},
                     [](const Args &a) { return args::inv_to_tiles(P(0), P(1), a.w, a.h, 64, P(2)); }});
    CALLS.push_back({"xTransformCtuFromTilesDev", 16, {{"d_cur", 16, 0, TB, nullptr, nullptr}, {"d_pred", 16, 0, TB, nullptr, nullptr}, {"d_class", 1, 0, CT6, nullptr, nullptr},
                     {"d_coef", 16, OUT, CT12K, nullptr, nullptr}}, [](const Args &a) { return args::transform_ctu_from_tiles(P(0), P(1), a.w, a.h, P(2), P(3)); }});
    CALLS.push_back({"xTransformCtuToTilesDev", 16, {{"d_coef", 16, 0, CT12K, nullptr, nullptr}, {"d_class", 1, 0, CT6, nullptr, nullptr}, {"d_pred", 16, 0, TB, nullptr, nullptr},
                     {"d_recon", 16, OUT, TB, "d_pred", nullptr}}, [](const Args &a) { return args::transform_ctu_to_tiles(P(0), P(1), P(2), a.w, a.h, P(3)); }});

    CALLS.push_back({"xSatd8x8SearchDev", 8, {{"d_cur", 1, 0, nullptr, nullptr, nullptr}, {"d_ref", 1, 0, nullptr, nullptr, nullptr}, {"d_best", 8, OUT, nullptr, nullptr, nullptr},
                     {"d_costs", 4, OUT | OPT, nullptr, nullptr, nullptr}}, [](const Args &a) { return args::plane_search(false, P(0), a.w, P(1), a.w + 8, a.w, a.h, 4, P(2), P(3)); }});
    CALLS.push_back({"xSad8x8SearchDev", 8, {{"d_cur", 4, 0, nullptr, nullptr, nullptr}, {"d_ref", 1, 0, nullptr, nullptr, nullptr}, {"d_best", 8, OUT, nullptr, nullptr, nullptr},
                     {"d_costs", 4, OUT | OPT, nullptr, nullptr, nullptr}}, [](const Args &a) { return args::plane_search(true, P(0), a.w, P(1), a.w + 8, a.w, a.h, 4, P(2), P(3)); }});
    // today's behaviour: each output is held against the two frames only, and only the cost map's end against the address space
    for (const char *n : {"xSatd8x8SearchFromTilesDev", "xSad8x8SearchFromTilesDev"})
        CALLS.push_back({n, 16, {{"d_cur", 16, UNFIT, TB, nullptr, nullptr}, {"d_ref", 16, UNFIT, TB, nullptr, nullptr}, {"d_best", 8, OUT | UNFIT, B8, nullptr, "d_costs"},
                         {"d_costs", 4, OUT | OPT, COSTS4, nullptr, "d_best"}}, [](const Args &a) { return args::tile_search(P(0), P(1), a.w, a.h, 4, P(2), P(3)); }});
    for (const char *n : {"xMotionCompLumaDev", "xMotionCompChromaDev", "xMotionCompDev"})
        CALLS.push_back({n, 16, {{"d_ref", 16, UNFIT, TB, nullptr, nullptr}, {"d_mv", 8, UNFIT, B8, nullptr, nullptr}, {"d_pred", 16, OUT | UNFIT, TB, nullptr, nullptr}},
                         [](const Args &a) { return args::motion_comp(false, P(0), P(1), a.w, a.h, P(2)); }});
    for (const char *n : {"xMotionCompQpelLumaGpu", "xMotionCompQpelChromaGpu", "xMotionCompQpelGpu"})
        CALLS.push_back({n, 16, {{"d_ref", 16, 0, TB, nullptr, nullptr}, {"d_mv", 8, 0, B8, nullptr, nullptr}, {"d_pred", 16, OUT, TB, nullptr, nullptr}},
                         [](const Args &a) { return args::motion_comp(true, P(0), P(1), a.w, a.h, P(2)); }});
    CALLS.push_back({"xSatd8x8RefineQpelFromTilesGpu", 16, {{"d_cur", 16, 0, TB, nullptr, nullptr}, {"d_ref", 16, 0, TB, nullptr, nullptr}, {"d_int", 8, 0, B8, nullptr, nullptr},
                     {"d_best", 8, OUT, B8, "d_int", nullptr}, {"d_costs", 4, OUT | OPT, COSTS49, nullptr, nullptr}},
                     [](const Args &a) { return args::refine_qpel(P(0), P(1), a.w, a.h, P(2), P(3), P(4)); }});

    CALLS.push_back({"xQuantRegionsGpu", 0, {{"d_in", 16, 0, N2048, nullptr, nullptr}, {"d_out", 16, OUT, N2048, "d_in", nullptr}, {"d_class", 1, OPT, N1, nullptr, nullptr},
                     {"d_qp", 1, OPT, N1, nullptr, nullptr}, {"d_nnz", 4, OUT | OPT, N4, nullptr, nullptr}},
                     [](const Args &a) { return args::quant_regions(0, P(0), P(1), a.n, P(2), P(3), 30, 171, P(4)); }});
    CALLS.push_back({"xDct32CodeCtuTilesGpu", 64, {{"d_cur", 16, 0, TB, nullptr, nullptr}, {"d_pred", 16, 0, TB, nullptr, nullptr}, {"d_qp", 1, OPT, CT6, nullptr, nullptr},
                     {"d_level", 16, OUT, CT12K, nullptr, nullptr}, {"d_nnz", 4, OUT | OPT, CT24, nullptr, nullptr}, {"d_recon", 16, OUT, TB, "d_pred", nullptr}},
                     [](const Args &a) { return args::dct32_code_ctu_tiles(P(0), P(1), a.w, a.h, P(2), 30, 171, P(3), P(4), P(5)); }});
    for (const char *n : {"xDeblockLumaGpu", "xDeblockChromaGpu", "xDeblockGpu"})
        CALLS.push_back({n, 16, {{"d_in", 16, 0, TB, nullptr, nullptr}, {"d_out", 16, OUT, TB, "d_in", nullptr}, {"d_class", 1, OPT, CT6, nullptr, nullptr}, {"d_intra", 1, OPT, CT6, nullptr, nullptr},
                         {"d_nnz", 4, OPT, CT24, nullptr, nullptr}, {"d_qp", 1, OPT, CT6, nullptr, nullptr}, {"d_mv", 8, OPT, B8, nullptr, nullptr}},
                         [](const Args &a) { const x266_deblock_t p = deblock_params(a); return args::deblock(P(0), a.w, a.h, &p, P(1)); }});
    CALLS.push_back({"xSaoStatsGpu", 16, {{"d_org", 16, 0, TB, nullptr, nullptr}, {"d_dec", 16, 0, TB, nullptr, nullptr}, {"d_stats", 4, OUT, CT1152, nullptr, nullptr}},
                     [](const Args &a) { return args::sao_stats(false, P(0), P(1), a.w, a.h, 0, nullptr, P(2)); }});
    CALLS.push_back({"xSaoSearchGpu", 16, {{"d_org", 16, 0, TB, nullptr, nullptr}, {"d_dec", 16, 0, TB, nullptr, nullptr}, {"d_param", 8, OUT, CT24, nullptr, nullptr},
                     {"d_stats", 4, OUT | OPT, CT1152, nullptr, nullptr}}, [](const Args &a) { return args::sao_stats(true, P(0), P(1), a.w, a.h, 100, P(2), P(3)); }});
    CALLS.push_back({"xSaoDecideGpu", 0, {{"d_stats", 4, 0, N1152, nullptr, nullptr}, {"d_param", 8, OUT, N24, nullptr, nullptr}},
                     [](const Args &a) { return args::sao_decide(P(0), a.n, 100, P(1)); }, true});
    CALLS.push_back({"xSaoApplyGpu", 16, {{"d_in", 16, 0, TB, nullptr, nullptr}, {"d_param", 8, 0, CT24, nullptr, nullptr}, {"d_out", 16, OUT, TB, nullptr, nullptr}},
                     [](const Args &a) { return args::sao_apply(P(0), a.w, a.h, P(1), P(2)); }});
    CALLS.push_back({"xIntra32RefsFromTilesGpu", 64, {{"d_frame", 16, 0, TB, nullptr, nullptr}, {"d_refs", 16, OUT, REFS4, nullptr, nullptr}},
                     [](const Args &a) { return args::intra32_refs_from_tiles(P(0), a.w, a.h, 0, P(1)); }});
    CALLS.push_back({"xIntra32CodeFrameGpu", 64, {{"d_cur", 16, 0, TB, nullptr, nullptr}, {"d_qp", 1, OPT, CT6, nullptr, nullptr}, {"d_mode_in", 1, OPT, CT6, nullptr, nullptr},
                     {"d_level", 16, OUT, CT12K, nullptr, nullptr}, {"d_nnz", 4, OUT | OPT, CT24, nullptr, nullptr}, {"d_mode", 1, OUT, CT6, "d_mode_in", nullptr},
                     {"d_recon", 16, OUT, TB, nullptr, nullptr}},
                     [](const Args &a) { return args::intra32_code_frame(P(0), a.w, a.h, P(1), 30, 171, P(2), P(3), P(4), P(5), P(6)); }});
}

// ---- scalars, strides and the rules that are a call's own --------------------------------------------------------------------------
static void quant_scalars(const char *n, const std::function<const char *(U d_qp, int qp, int rounding)> &f)
{
    range(n, "qp without d_qp", 0, 51, [&](int v) { return f(0, v, 171); });
    expect(n, "qp 99 with d_qp", f((U)1 << 50, 99, 171), false);
    range(n, "rounding", 0, 511, [&](int v) { return f(0, 30, v); });
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

static void own_rules()
{
    const char *n = "xDct32PassDev";
    range(n, "shift", 1, 15, [&](int v) { const Args a = base(call(n)); return args::dct32_pass(P(0), P(1), a.n, v); });
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
        range(t, "range", 1, 64, [&](int r) { return args::tile_search(P(0), P(1), a.w, a.h, r, P(2), P(3)); });
        expect(t, "d_cur == d_ref", args::tile_search(P(0), P(0), a.w, a.h, 4, P(2), P(3)), false);
        // a cost map whose size wraps size_t: 2^49 blocks x 129 x 129 x 4 bytes; the frames (2^56 bytes) and d_best (2^52) are placed to fit
        const U cur = ((U)1 << 57) + 16, best = ((U)1 << 59) + 8, costs = ((U)1 << 60) + 4;
        expect(t, "cost map wraps size_t", args::tile_search(V(cur), V(cur), 1 << 28, 1 << 27, 64, V(best), V(costs)), true, args::kNoFit);
        expect(t, "the same frame without a cost map", args::tile_search(V(cur), V(cur), 1 << 28, 1 << 27, 64, V(best), nullptr), false);
    }

    n = "xQuantRegionsGpu";
    { const Args a = base(call(n));
      quant_scalars(n, [&](U d_qp, int qp, int r) { return args::quant_regions(0, P(0), P(1), a.n, P(2), V(d_qp), qp, r, P(4)); });
      expect(n, "inverse with d_nnz", args::quant_regions(1, P(0), P(1), a.n, P(2), P(3), 30, 171, P(4)), true);
      expect(n, "inverse without d_nnz", args::quant_regions(1, P(0), P(1), a.n, P(2), P(3), 30, 171, nullptr), false);
      expect(n, "n_regions == 0, qp 52", args::quant_regions(0, nullptr, nullptr, 0, nullptr, nullptr, 52, 171, nullptr), true);   // scalar errors first
      expect(n, "n_regions == 0, rounding 512", args::quant_regions(0, nullptr, nullptr, 0, nullptr, nullptr, 30, 512, nullptr), true);
      expect(n, "a count whose bytes wrap size_t", args::quant_regions(0, P(0), P(1), SIZE_MAX / 2048 + 1, P(2), P(3), 30, 171, P(4)), true, args::kNoFit);
      expect(n, "a count whose d_nnz bytes wrap size_t", args::quant_regions(0, P(0), P(1), SIZE_MAX / 4 + 1, nullptr, nullptr, 30, 171, P(4)), true, args::kNoFit); }
    n = "xDct32CodeCtuTilesGpu";
    { const Args a = base(call(n));
      quant_scalars(n, [&](U d_qp, int qp, int r) { return args::dct32_code_ctu_tiles(P(0), P(1), a.w, a.h, V(d_qp), qp, r, P(3), P(4), P(5)); });
      auto f = [&](U cur, U pred, U recon) { return args::dct32_code_ctu_tiles(V(cur), V(pred), a.w, a.h, P(2), 30, 171, P(3), P(4), V(recon)); };
      expect(n, "d_cur == d_pred", f(a.p[1], a.p[1], a.p[5]), false);
      expect(n, "d_cur == d_pred == d_recon", f(a.p[1], a.p[1], a.p[1]), false);
      expect(n, "d_recon == d_cur", f(a.p[0], a.p[1], a.p[0]), true, args::kOverlap);
      expect(n, "d_level on d_cur == d_pred", args::dct32_code_ctu_tiles(P(1), P(1), a.w, a.h, P(2), 30, 171, V(a.p[1] + 16), P(4), P(5)), true, args::kOverlap); }
    n = "xIntra32CodeFrameGpu";
    { const Args a = base(call(n));
      quant_scalars(n, [&](U d_qp, int qp, int r) { return args::intra32_code_frame(P(0), a.w, a.h, V(d_qp), qp, r, P(2), P(3), P(4), P(5), P(6)); });
      expect(n, "d_qp == d_mode_in == d_mode", args::intra32_code_frame(P(0), a.w, a.h, P(5), 30, 171, P(5), P(3), P(4), P(5), P(6)), true, args::kOverlap); }
    n = "xIntra32RefsFromTilesGpu";
    { const Args a = base(call(n));
      range(n, "component", 0, 2, [&](int v) { return args::intra32_refs_from_tiles(P(0), a.w, a.h, v, P(1)); });
      // chroma: one reference set per CTU, a quarter of luma's extent
      expect(n, "component 1: a quarter of the luma extent in front of the frame", args::intra32_refs_from_tiles(P(0), a.w, a.h, 1, V(down(a.p[0] - sizeof(x266_intra_ref_t), 16))), false);
      expect(n, "component 0: the same place overlaps", args::intra32_refs_from_tiles(P(0), a.w, a.h, 0, V(down(a.p[0] - sizeof(x266_intra_ref_t), 16))), true, args::kOverlap); }

    for (const char *t : {"xDeblockLumaGpu", "xDeblockChromaGpu", "xDeblockGpu"}) {
        const Args a = base(call(t));
        auto f = [&](U d_qp, int qp, int beta, int tc) { Args b = a; b.p[5] = d_qp; const x266_deblock_t p = deblock_params(b, qp, beta, tc); return args::deblock(P(0), a.w, a.h, &p, P(1)); };
        expect(t, "NULL parameter struct", args::deblock(P(0), a.w, a.h, nullptr, P(1)), true);
        range(t, "qp without d_qp", 0, 51, [&](int v) { return f(0, v, 0, 0); });
        expect(t, "qp 99 with d_qp", f(a.p[5], 99, 0, 0), false);
        range(t, "beta_offset_div2", -6, 6, [&](int v) { return f(a.p[5], 30, v, 0); });
        range(t, "tc_offset_div2", -6, 6, [&](int v) { return f(a.p[5], 30, 0, v); });
    }
    n = "xSaoSearchGpu";
    { const Args a = base(call(n)); range(n, "lambda_q4", 0, 65535, [&](int v) { return args::sao_stats(true, P(0), P(1), a.w, a.h, v, P(2), P(3)); }); }
    n = "xSaoDecideGpu";
    { const Args a = base(call(n));
      range(n, "lambda_q4", 0, 65535, [&](int v) { return args::sao_decide(P(0), a.n, v, P(1)); });
      expect(n, "n_ctu 2^31 - 1", args::sao_decide(P(0), 0x7FFFFFFFull, 100, P(1)), false);
      expect(n, "n_ctu 2^31", args::sao_decide(P(0), 0x80000000ull, 100, P(1)), true);
      expect(n, "n_ctu 0, lambda_q4 65536", args::sao_decide(P(0), 0, 65536, P(1)), true); }
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
    if (g_failures) {
        std::printf("%d of %d checks failed\n", g_failures, g_checks);
        return 1;
    }
    std::printf("%zu entry points, %d checks: the argument rules hold\n", CALLS.size(), g_checks);
    return 0;
}
