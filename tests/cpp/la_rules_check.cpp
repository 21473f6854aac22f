// CPU check of the argument rules of the five lookahead calls (x266_amd/csrc/x266_args.hpp: la_downscale, la_intra_costs, la_frame_cost,
// la_propagate, la_tree_qp) and of xSceneCutFromTotals.  The calls take their device pointers in a host-read struct, so the one table of
// tests/cpp/arg_rules_check.cpp does not count them; this driver holds them the way tests/cpp/aq_rules_check.cpp holds the source
// analysis'.  The rules are integer arithmetic on addresses and sizes: the addresses are made-up integers, nothing is dereferenced, no
// device is needed.
//
// FIELDS is the contract written down once more by hand from include/x266hip.h: every pointer field's alignment and, per call, whether
// the call looks at it, whether it may be NULL and whether the call writes (or adds into) it.  One walk perturbs a base tuple one field
// at a time; the expected verdict of every perturbation follows from that table, never from the functions under test.
// Test infrastructure; built and run by tests/test_la_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>

#include "x266_args.hpp"

using namespace x266;

typedef uintptr_t U;
enum Field { SRC, LOW, INTRA, MODE, INTER0, INTER1, BLOCK, TOTAL, PROP, REF0, REF1, AQ, OFFSET, QP, N_FIELDS };
enum Call { DOWNSCALE, INTRA_COSTS, FRAME_COST, PROPAGATE, TREE_QP, N_CALLS };
enum { IN = 0, OPT = 1, OUT = 2, UNUSED = 4 };
static const char *const CALLS[N_CALLS] = {"xLaDownscaleGpu", "xLaIntraCostsGpu", "xLaFrameCostGpu", "xLaPropagateGpu", "xLaTreeQpGpu"};
struct Ptr {
    const char *name;
    unsigned align;
    int flags[N_CALLS];
};
static const Ptr FIELDS[N_FIELDS] = {
    {"d_src", 16, {IN, UNUSED, UNUSED, UNUSED, UNUSED}},
    {"d_low", 16, {OUT, IN, UNUSED, UNUSED, UNUSED}},
    {"d_intra", 4, {UNUSED, OUT, IN, UNUSED, UNUSED}},
    {"d_mode", 1, {UNUSED, OPT | OUT, OPT, UNUSED, UNUSED}},
    {"d_inter0", 8, {UNUSED, UNUSED, OPT, UNUSED, UNUSED}},
    {"d_inter1", 8, {UNUSED, UNUSED, OPT, UNUSED, UNUSED}},
    {"d_block", 16, {UNUSED, UNUSED, OUT, IN, IN}},
    {"d_total", 8, {UNUSED, UNUSED, OUT, UNUSED, UNUSED}},
    {"d_prop", 8, {UNUSED, UNUSED, UNUSED, OPT, OPT}},
    {"d_prop_ref0", 8, {UNUSED, UNUSED, UNUSED, OPT | OUT, UNUSED}},
    {"d_prop_ref1", 8, {UNUSED, UNUSED, UNUSED, OPT | OUT, UNUSED}},
    {"d_aq_offset", 2, {UNUSED, UNUSED, UNUSED, UNUSED, OPT}},
    {"d_offset", 2, {UNUSED, UNUSED, UNUSED, UNUSED, OPT | OUT}},
    {"d_qp", 1, {UNUSED, UNUSED, UNUSED, UNUSED, OPT | OUT}},
};
static size_t extent(int f, int w, int h)
{
    const size_t n = (size_t)(w / 16) * (size_t)(h / 16), n_ctu = (size_t)((w + 63) / 64) * (size_t)((h + 63) / 64);
    switch (f) {
    case SRC: return n * 512;
    case LOW: return n * 128;
    case INTRA: return n * 4;
    case MODE: return n;
    case BLOCK: return n * 16;
    case TOTAL: return 64;
    case AQ:
    case OFFSET: return n * 2;
    case QP: return n_ctu * 6;
    default: return n * 8;                                                  // the search records and the three accumulators
    }
}

struct Tuple {
    U p[N_FIELDS];
    int w, h, penalty, strength, qp, chroma;
};
static x266_la_t make(const Tuple &t)
{
    x266_la_t s;
    s.d_src = (const x266_ref_block_t *)t.p[SRC];
    s.d_low = (x266_ref_block_t *)t.p[LOW];
    s.d_intra = (uint32_t *)t.p[INTRA];
    s.d_mode = (uint8_t *)t.p[MODE];
    s.d_inter0 = (const x266_me_result_t *)t.p[INTER0];
    s.d_inter1 = (const x266_me_result_t *)t.p[INTER1];
    s.d_block = (x266_la_block_t *)t.p[BLOCK];
    s.d_total = (int64_t *)t.p[TOTAL];
    s.d_prop = (const uint64_t *)t.p[PROP];
    s.d_prop_ref0 = (uint64_t *)t.p[REF0];
    s.d_prop_ref1 = (uint64_t *)t.p[REF1];
    s.d_aq_offset = (const int16_t *)t.p[AQ];
    s.d_offset = (int16_t *)t.p[OFFSET];
    s.d_qp = (uint8_t *)t.p[QP];
    s.width = t.w;
    s.height = t.h;
    s.intra_penalty = t.penalty;
    s.strength_q8 = t.strength;
    s.qp = t.qp;
    s.chroma_qp_offset = t.chroma;
    return s;
}
// every pointer in a region of its own, at exactly its alignment times an odd number; a frame of 10 x 6 tiles, 3 x 2 CTUs
static Tuple base()
{
    Tuple t;
    for (int i = 0; i < N_FIELDS; ++i) t.p[i] = ((U)(i + 1) << 44) + (U)FIELDS[i].align * (2 * i + 1);
    t.w = 160;
    t.h = 96;
    t.penalty = 300;
    t.strength = 256;
    t.qp = 30;
    t.chroma = -2;
    return t;
}

static int g_checks = 0, g_failures = 0;
static void expect(const char *call, const std::string &what, const char *got, bool refuse, const char *reason = nullptr)
{
    ++g_checks;
    if ((got != nullptr) == refuse && (!refuse || !reason || !std::strcmp(got, reason))) return;
    ++g_failures;
    std::printf("FAIL %s: %s: expected %s%s%s, got %s\n", call, what.c_str(), refuse ? "refuse" : "accept", refuse && reason ? " for " : "",
                refuse && reason ? reason : "", got ? got : "accept");
}

static const char *rule_of(int c, const x266_la_t *s)
{
    switch (c) {
    case DOWNSCALE: return args::la_downscale(s);
    case INTRA_COSTS: return args::la_intra_costs(s);
    case FRAME_COST: return args::la_frame_cost(s);
    case PROPAGATE: return args::la_propagate(s);
    default: return args::la_tree_qp(s);
    }
}

static void walk(int c)
{
    const char *call = CALLS[c];
    auto rule = [&](const Tuple &t) {
        const x266_la_t s = make(t);
        return rule_of(c, &s);
    };
    auto flags = [&](int f) { return FIELDS[f].flags[c]; };
    const Tuple b = base();
    expect(call, "NULL p", rule_of(c, nullptr), true, "NULL parameter struct");
    expect(call, "base", rule(b), false);
    for (int f = 0; f < N_FIELDS; ++f) {
        const std::string name = FIELDS[f].name;
        const bool used = !(flags(f) & UNUSED);
        Tuple t = b;
        t.p[f] = 0;
        expect(call, name + " NULL", rule(t), used && !(flags(f) & OPT), args::kNull);
        if (FIELDS[f].align > 1) {
            t = b;
            t.p[f] += FIELDS[f].align / 2;
            expect(call, name + " at half its alignment", rule(t), used, args::kMisaligned);
            t = b;
            t.p[f] += FIELDS[f].align;                                          // aligned to exactly that, and to twice it: both fine
            expect(call, name + " one alignment further", rule(t), false);
        } else {
            t = b;
            t.p[f] += 1;
            expect(call, name + " at an odd address", rule(t), false);
        }
        // the span's end against the end of the address space
        const size_t bytes = extent(f, b.w, b.h);
        t = b;
        t.p[f] = (U)0 - FIELDS[f].align;                                        // the last aligned address: every extent here is larger and wraps
        expect(call, name + " running past the top of the address space", rule(t), used && bytes > FIELDS[f].align, args::kNoFit);
        t = b;
        t.p[f] = ((U)0 - 2 * bytes) - ((U)0 - 2 * bytes) % FIELDS[f].align;     // high up, with room to spare
        expect(call, name + " near the top of the address space", rule(t), false);
        // overlap: field g moved onto the first byte, and onto the last byte, of field f; refused when either is an output
        for (int g = 0; g < N_FIELDS; ++g) {
            if (g == f) continue;
            const bool both = used && !(flags(g) & UNUSED), any_out = (flags(f) & OUT) || (flags(g) & OUT);
            const size_t gb = extent(g, b.w, b.h);
            t = b;
            t.p[g] = t.p[f] - t.p[f] % FIELDS[g].align;                         // g starts at or just before f's first byte, and is longer than that step
            if (gb <= t.p[f] - t.p[g]) ++g_failures, std::printf("FAIL the driver's own overlap case %s / %s\n", FIELDS[g].name, name.c_str());
            expect(call, std::string(FIELDS[g].name) + " over the start of " + name, rule(t), both && any_out, args::kOverlap);
            t = b;
            t.p[g] = t.p[f] + bytes - 1;
            t.p[g] -= t.p[g] % FIELDS[g].align;                                 // g's first byte among f's last
            expect(call, std::string(FIELDS[g].name) + " over the end of " + name, rule(t), both && any_out, args::kOverlap);
            t = b;
            t.p[g] = t.p[f] + bytes + FIELDS[g].align - 1;
            t.p[g] -= t.p[g] % FIELDS[g].align;                                 // right behind f
            expect(call, std::string(FIELDS[g].name) + " right behind " + name, rule(t), false);
        }
    }
    // the very same address twice: two accumulators, an accumulator and what the frame received; two lists may be one array
    {
        Tuple t = b;
        t.p[REF1] = t.p[REF0];
        expect(call, "d_prop_ref1 == d_prop_ref0", rule(t), c == PROPAGATE, args::kOverlap);
        t = b;
        t.p[REF0] = t.p[PROP];
        expect(call, "d_prop_ref0 == d_prop", rule(t), c == PROPAGATE, args::kOverlap);
        t = b;
        t.p[INTER1] = t.p[INTER0];
        expect(call, "d_inter1 == d_inter0", rule(t), false);
        t = b;
        t.p[OFFSET] = t.p[AQ];
        expect(call, "d_offset == d_aq_offset", rule(t), c == TREE_QP, args::kOverlap);
    }
    // the optional fields all NULL at once; tree qp needs one of its two outputs
    {
        Tuple t = b;
        for (int f = 0; f < N_FIELDS; ++f)
            if ((flags(f) & OPT) && f != QP) t.p[f] = 0;
        expect(call, "every optional field NULL (but d_qp)", rule(t), false);
        t.p[QP] = 0;
        expect(call, "d_offset and d_qp both NULL", rule(t), c == TREE_QP, "d_offset and d_qp are both NULL");
        t = b;
        t.p[OFFSET] = 0;
        t.p[QP] = (U)0 - 37;                                                    // 6 CTUs, 36 bytes: the span ends one byte below the top
        expect(call, "d_qp ending just below the top", rule(t), false);
        t.p[QP] = (U)0 - 35;
        expect(call, "d_qp one byte too far", rule(t), c == TREE_QP, args::kNoFit);
    }
    // frame sizes
    {
        const int bad[] = {0, -32, 8, 16, 48, 144, 159, 161, INT_MIN, INT_MAX};
        for (int v : bad) {
            Tuple t = b;
            t.w = v;
            expect(call, "width " + std::to_string(v), rule(t), true, "width/height must be positive multiples of 32");
            t = b;
            t.h = v;
            expect(call, "height " + std::to_string(v), rule(t), true, "width/height must be positive multiples of 32");
        }
        const int good[][2] = {{32, 32}, {64, 32}, {32, 64}, {96, 160}, {160, 96}, {32, 32800}, {3840, 2176}, {7680, 4320}};
        for (const auto &g : good) {
            Tuple t = b;
            t.w = g[0];
            t.h = g[1];
            expect(call, "frame " + std::to_string(g[0]) + "x" + std::to_string(g[1]), rule(t), false);
        }
    }
    // scalars: the call that reads one holds it to its range, the others read none of them
    {
        struct Scalar {
            const char *name;
            int Tuple::*field;
            int lo, hi, call;
            const char *reason;
        };
        const Scalar scalars[] = {{"intra_penalty", &Tuple::penalty, 0, 65535, FRAME_COST, args::kLaPenalty},
                                  {"strength_q8", &Tuple::strength, 0, 1024, TREE_QP, args::kLaScalars},
                                  {"qp", &Tuple::qp, 0, 51, TREE_QP, args::kLaScalars},
                                  {"chroma_qp_offset", &Tuple::chroma, -12, 12, TREE_QP, args::kLaScalars}};
        for (const Scalar &s : scalars) {
            const int values[] = {s.lo, s.hi, s.lo - 1, s.hi + 1, INT_MIN, INT_MAX};
            for (int v : values) {
                Tuple t = b;
                t.*(s.field) = v;
                expect(call, std::string(s.name) + " " + std::to_string(v), rule(t), c == s.call && (v < s.lo || v > s.hi), s.reason);
            }
        }
    }
    // the largest frame an int describes: its spans fit behind addresses of 2^44 and cover every buffer above them; high up they do not fit
    {
        const int side = INT_MAX - INT_MAX % 32;
        Tuple t = b;
        t.w = t.h = side;
        expect(call, "the largest frame", rule(t), true, args::kOverlap);
        const int first[N_CALLS] = {SRC, LOW, INTRA, BLOCK, BLOCK};
        t.p[first[c]] = (U)0 - ((U)1 << 40);
        expect(call, "the largest frame, high up", rule(t), true, args::kNoFit);
    }
}

static void scene_cut()
{
    const char *call = "xSceneCutFromTotals";
    const int64_t good[8] = {90000, 100000, 10, 40, 10, 95000, 97000, 60};
    expect(call, "base", args::scene_cut_from_totals(good, 102, 100, 25, 250), false);
    expect(call, "NULL total", args::scene_cut_from_totals(nullptr, 102, 100, 25, 250), true, args::kNull);
    const int thresholds[] = {0, 256, -1, 257, INT_MIN, INT_MAX};
    for (int v : thresholds) expect(call, "threshold_q8 " + std::to_string(v), args::scene_cut_from_totals(good, v, 100, 25, 250), v < 0 || v > 256);
    const int gs[] = {0, INT_MAX, -1, INT_MIN};
    for (int v : gs) expect(call, "frames_since_key " + std::to_string(v), args::scene_cut_from_totals(good, 102, v, 25, 250), v < 0);
    const int keyints[][2] = {{1, 1}, {25, 25}, {1, INT_MAX}, {INT_MAX, INT_MAX}, {0, 250}, {-1, 250}, {25, 24}, {INT_MAX, 1}};
    for (const auto &k : keyints)
        expect(call, "keyints " + std::to_string(k[0]) + " / " + std::to_string(k[1]), args::scene_cut_from_totals(good, 102, 100, k[0], k[1]), k[0] < 1 || k[1] < k[0]);
    for (int i = 0; i < 8; ++i) {
        int64_t t[8];
        std::memcpy(t, good, sizeof t);
        t[i] = -1;
        expect(call, "total[" + std::to_string(i) + "] negative", args::scene_cut_from_totals(t, 102, 100, 25, 250), true);
    }
    const int64_t counts[] = {1, (int64_t)1 << 24, 0, ((int64_t)1 << 24) + 1, INT64_MAX};
    for (int64_t v : counts) {
        int64_t t[8];
        std::memcpy(t, good, sizeof t);
        t[7] = v;
        expect(call, "total[7] " + std::to_string(v), args::scene_cut_from_totals(t, 102, 100, 25, 250), v < 1 || v > ((int64_t)1 << 24));
    }
    for (int i = 0; i < 2; ++i) {
        const int64_t costs[] = {0, (int64_t)1 << 40, ((int64_t)1 << 40) + 1, INT64_MAX};
        for (int64_t v : costs) {
            int64_t t[8];
            std::memcpy(t, good, sizeof t);
            t[i] = v;
            expect(call, "total[" + std::to_string(i) + "] " + std::to_string(v), args::scene_cut_from_totals(t, 102, 100, 25, 250), v > ((int64_t)1 << 40));
        }
    }
}

int main()
{
    for (int c = 0; c < N_CALLS; ++c) walk(c);
    scene_cut();
    std::printf("the lookahead calls: %d checks, %d failures\n", g_checks, g_failures);
    if (g_failures) return 1;
    std::printf("the argument rules hold\n");
    return 0;
}
