// CPU check of the argument rules of xTransformDecideCtuTilesGpu (x266_amd/csrc/x266_args.hpp: transform_decide), the call whose device
// pointers are the fields of the host-read x266_tdecide_t.  The contract is written down once more by hand from include/x266hip.h -- the
// pointer fields in struct order with their alignments, which are written and which may be NULL, their extents -- and one walk perturbs a
// base tuple one field at a time, with and without each optional buffer: NULL, half an alignment, one alignment further, the top of the
// address space, every overlap of an output with any other buffer, the frame sizes, the scalar ranges and the mask rules.  The addresses
// are made-up integers, nothing is dereferenced, no device is needed; the expected verdict of every check follows from these tables and
// from literals, never from the function under test.
// Test infrastructure; built and run by tests/test_tdecide_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <climits>
#include <string>

#include "rules_expect.hpp"
#include "x266_args.hpp"

using namespace x266;

static const char *CALL = "xTransformDecideCtuTilesGpu";
enum { CUR, PRED, QP, CAND, CLASS, LEVEL, NNZ, STAT, COST, N_FIELDS };
struct Field {
    const char *name;
    unsigned align;
    bool optional, output;
    size_t per_region;              // bytes per region; 0: a frame of width * height * 2 bytes
};
static const Field FIELDS[N_FIELDS] = {{"d_cur", 16, false, false, 0}, {"d_pred", 16, false, false, 0}, {"d_qp", 1, true, false, 1},
                                       {"d_cand", 2, true, false, 2},  {"d_class", 1, false, true, 1},  {"d_level", 16, false, true, 2048},
                                       {"d_nnz", 4, true, true, 4},    {"d_stat", 8, true, true, 16},   {"d_cost", 8, true, true, 128}};
struct Tuple {
    U p[N_FIELDS];
    int w, h, qp, lambda;
    unsigned luma, chroma;
};

static size_t extent(int f, const Tuple &t)
{
    const size_t regions = 6 * (((size_t)t.w + 63) / 64) * (((size_t)t.h + 63) / 64);
    return FIELDS[f].per_region ? regions * FIELDS[f].per_region : (size_t)t.w * (size_t)t.h * 2;
}
static const char *rule(const Tuple &t)
{
    x266_tdecide_t s = {};
    s.d_cur = (const x266_ref_block_t *)t.p[CUR];
    s.d_pred = (const x266_ref_block_t *)t.p[PRED];
    s.d_qp = (const uint8_t *)t.p[QP];
    s.d_cand = (const uint16_t *)t.p[CAND];
    s.d_class = (uint8_t *)t.p[CLASS];
    s.d_level = (int16_t *)t.p[LEVEL];
    s.d_nnz = (uint32_t *)t.p[NNZ];
    s.d_stat = (x266_rdoq_region_t *)t.p[STAT];
    s.d_cost = (uint64_t *)t.p[COST];
    s.width = t.w;
    s.height = t.h;
    s.qp = t.qp;
    s.lambda = t.lambda;
    s.cand_luma = (uint16_t)t.luma;
    s.cand_chroma = (uint16_t)t.chroma;
    for (int k = 0; k < 16; ++k) s.class_bits[k] = (uint16_t)(65535 - k);   // any value is accepted
    return args::transform_decide(&s);
}
// every pointer in a region of its own, at exactly its alignment times an odd number
static Tuple placed(int w, int h)
{
    Tuple t = {};
    for (int i = 0; i < N_FIELDS; ++i) t.p[i] = ((U)(i + 1) << 44) + (U)FIELDS[i].align * (2 * i + 1);
    t.w = w;
    t.h = h;
    t.qp = 30;
    t.lambda = 368;
    t.luma = 0x777F;
    t.chroma = 0x0008;
    return t;
}

// `without`: a bit per optional field that is NULL in this walk's base
static void walk(const Tuple &base, unsigned without, const std::string &label)
{
    Tuple b = base;
    std::string at = label + "without";
    for (int f = 0; f < N_FIELDS; ++f)
        if ((without >> f) & 1u) {
            b.p[f] = 0;
            at += std::string(" ") + FIELDS[f].name;
        }
    at += ": ";
    expect(CALL, at + "base", rule(b), false);
    for (int f = 0; f < N_FIELDS; ++f) {
        if (!b.p[f]) continue;
        const unsigned align = FIELDS[f].align;
        const std::string name = at + FIELDS[f].name;
        Tuple t = b;
        t.p[f] = 0;
        // d_qp NULL brings the scalar qp into the rules: 30 is in range
        expect(CALL, name + " NULL", rule(t), !FIELDS[f].optional, args::kNull);
        if (align > 1) {
            t = b;
            t.p[f] += align / 2;
            expect(CALL, name + " at half its alignment", rule(t), true, args::kMisaligned);
        }
        t = b;
        t.p[f] += align;
        expect(CALL, name + " one alignment further", rule(t), false);
        const size_t bytes = extent(f, b);
        if (bytes <= align) ++g_failures, std::printf("FAIL the driver's own extent of %s\n", name.c_str());
        t = b;
        t.p[f] = (U)0 - align;                                              // the last aligned address: every extent here is larger and wraps
        expect(CALL, name + " running past the top of the address space", rule(t), true, args::kNoFit);
        t.p[f] = down((U)0 - bytes - align, align);                         // the span ends just below the top
        expect(CALL, name + " ending just below the top", rule(t), false);
        t.p[f] = down((U)0 - bytes + align, align);                         // ... and just above it
        expect(CALL, name + " ending just above the top", rule(t), true, args::kNoFit);
        // overlaps: field f placed onto every other buffer g -- refused iff one of the two is an output
        for (int g = 0; g < N_FIELDS; ++g) {
            if (g == f || !b.p[g]) continue;
            const bool bad = FIELDS[f].output || FIELDS[g].output;
            const size_t other = extent(g, b);
            const std::string on = name + " on " + FIELDS[g].name;
            t = b;
            t.p[f] = b.p[g];
            if (t.p[f] % align == 0) expect(CALL, on + ": same address", rule(t), bad, args::kOverlap);
            t.p[f] = down(b.p[g] + other - 1, align);                       // onto g's last byte
            expect(CALL, on + ": its last bytes", rule(t), bad, args::kOverlap);
            t.p[f] = up(b.p[g] + other, align);                             // right behind g
            expect(CALL, on + ": right behind it", rule(t), false);
            t.p[f] = down(b.p[g] - bytes, align);                           // ending where g begins, or before
            expect(CALL, on + ": right in front of it", rule(t), false);
            t.p[f] = down(b.p[g] - bytes, align) + align;                   // f's last bytes reach into g ...
            if (t.p[f] + bytes > b.p[g]) expect(CALL, on + ": its last bytes reach in", rule(t), bad, args::kOverlap);
        }
    }
}

static void sizes_scalars_masks(const Tuple &b)
{
    const char *size_why = "width/height must be positive multiples of 16";
    for (int bad : {0, -16, 8, 24, 63, 65, INT_MIN, INT_MAX}) {
        Tuple t = b;
        t.w = bad;
        expect(CALL, "width " + std::to_string(bad), rule(t), true, size_why);
        t = b;
        t.h = bad;
        expect(CALL, "height " + std::to_string(bad), rule(t), true, size_why);
    }
    for (auto wh : {std::pair<int, int>{16, 16}, {48, 16}, {80, 48}, {144, 80}, {1920, 1088}, {3840, 2176}, {7680, 4320}}) {
        Tuple t = placed(wh.first, wh.second);
        expect(CALL, "frame " + std::to_string(wh.first) + "x" + std::to_string(wh.second), rule(t), false);
    }
    {   // the largest frame an int describes: the extents are exact (no product wraps 64 bits), and the frames no longer fit beside each other
        Tuple t = placed(INT_MAX - 15, INT_MAX - 15);
        expect(CALL, "the largest frame", rule(t), true, args::kOverlap);
        t.p[COST] = (U)0 - 8 * 4096;                                        // n * 128 bytes do not fit behind it
        expect(CALL, "the largest frame, d_cost near the top", rule(t), true, args::kNoFit);
    }
    range(CALL, "lambda", 0, 8192, [&](int v) { Tuple t = b; t.lambda = v; return rule(t); }, args::kRdoqScalars);
    range(CALL, "qp without d_qp", 0, 51, [&](int v) { Tuple t = b; t.p[QP] = 0; t.qp = v; return rule(t); }, args::kRdoqScalars);
    for (int v : {-1, 52, INT_MIN, INT_MAX}) {
        Tuple t = b;
        t.qp = v;
        expect(CALL, "qp " + std::to_string(v) + " beside d_qp", rule(t), b.p[QP] == 0, args::kRdoqScalars);
    }
    // the masks: every single valid bit is accepted, every single invalid one refused, alone and beside valid ones; an empty mask is refused
    for (int luma = 0; luma < 2; ++luma) {
        auto with = [&](unsigned m) { Tuple t = b; (luma ? t.luma : t.chroma) = m; return rule(t); };
        const std::string which = luma ? "cand_luma " : "cand_chroma ";
        expect(CALL, which + "empty", with(0), true, args::kTDecideMasks);
        expect(CALL, which + "all 13", with(0x777F), false);
        expect(CALL, which + "all 16", with(0xFFFF), true, args::kTDecideMasks);
        for (unsigned k = 0; k < 16; ++k) {
            const bool valid = k != 7 && k != 11 && k != 15;                // size 32 exists as class 3 only
            expect(CALL, which + "bit " + std::to_string(k), with(1u << k), !valid, args::kTDecideMasks);
            expect(CALL, which + "bit " + std::to_string(k) + " beside class 3", with((1u << k) | 8u), !valid, args::kTDecideMasks);
        }
    }
}

int main()
{
    std::printf("%s:", CALL);
    for (int f = 0; f < N_FIELDS; ++f)
        std::printf("%s %s %u %s%s", f ? "," : "", FIELDS[f].name, FIELDS[f].align, FIELDS[f].optional ? "opt " : "", FIELDS[f].output ? "out" : "in");
    std::printf("\n");
    ++g_checks;
    if (!args::transform_decide(nullptr)) ++g_failures, std::printf("FAIL a NULL parameter struct is accepted\n");
    unsigned optional = 0;
    for (int f = 0; f < N_FIELDS; ++f)
        if (FIELDS[f].optional) optional |= 1u << f;
    for (auto wh : {std::pair<int, int>{144, 80}, {64, 64}, {1920, 1088}}) {
        const Tuple b = placed(wh.first, wh.second);
        const std::string label = std::to_string(wh.first) + "x" + std::to_string(wh.second) + " ";
        walk(b, 0, label);
        walk(b, optional, label);
        for (int f = 0; f < N_FIELDS; ++f)
            if (FIELDS[f].optional) walk(b, 1u << f, label);
        sizes_scalars_masks(b);
        Tuple t = b;
        t.p[QP] = 0;
        sizes_scalars_masks(t);
        t = b;
        t.p[PRED] = b.p[CUR];                                               // two inputs may be the same frame
        expect(CALL, label + "d_pred == d_cur", rule(t), false);
    }
    std::printf("checks x266_tdecide_t %d\n", g_checks);
    if (g_failures) {
        std::printf("%d of %d checks FAILED\n", g_failures, g_checks);
        return 1;
    }
    std::printf("the argument rules hold (%d checks)\n", g_checks);
    return 0;
}
