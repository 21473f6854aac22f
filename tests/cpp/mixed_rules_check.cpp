// CPU check of the argument rules of mixed inter / intra frame coding, xDct32CodeMixedFrameGpu (x266_amd/csrc/x266_args.hpp:
// mixed_code_frame).  The call takes its device pointers in a host-read struct, so the one table of tests/cpp/arg_rules_check.cpp does not
// count it; this driver holds it the way tests/cpp/seed_rules_check.cpp holds the seeded search's.  The rules are integer arithmetic on
// addresses and sizes: the addresses are made-up integers, nothing is dereferenced, no device is needed.
//
// FIELDS is the contract written down once more by hand from include/x266hip.h: every pointer field's alignment, whether it may be NULL,
// whether the call writes it, and the one input an output may BE.  One walk perturbs a base tuple one field at a time, with and without
// the optional buffers; the expected verdict of every perturbation follows from that table, never from the function under test.
// Test infrastructure; built and run by tests/test_mixed_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>

#include "x266_args.hpp"

using namespace x266;

typedef uintptr_t U;
enum Field { CUR, PRED, QP, KIND_IN, MODE_IN, LEVEL, NNZ, KIND, MODE, COST, RECON, N_FIELDS };
enum { IN = 0, OPT = 1, OUT = 2 };
static const char *const CALL = "xDct32CodeMixedFrameGpu";
struct Ptr {
    const char *name;
    unsigned align;
    int flags;
    int same;                       // the input this output may be (the very same address), or -1
};
static const Ptr FIELDS[N_FIELDS] = {
    {"d_cur", 16, IN, -1},
    {"d_pred", 16, IN, -1},
    {"d_qp", 1, OPT | IN, -1},
    {"d_kind_in", 1, OPT | IN, -1},
    {"d_mode_in", 1, OPT | IN, -1},
    {"d_level", 16, OUT, -1},
    {"d_nnz", 4, OPT | OUT, -1},
    {"d_kind", 1, OUT, KIND_IN},
    {"d_mode", 1, OUT, MODE_IN},
    {"d_cost", 4, OPT | OUT, -1},
    {"d_recon", 16, OUT, PRED},
};
static size_t extent(int f, int w, int h)
{
    const size_t tiles = (size_t)(w / 16) * (size_t)(h / 16), regions = (size_t)(w / 64) * (size_t)(h / 64) * 6;
    switch (f) {
    case CUR:
    case PRED:
    case RECON: return tiles * 512;
    case LEVEL: return regions * 2048;
    case NNZ: return regions * 4;
    case COST: return regions * 8;
    default: return regions;
    }
}

struct Tuple {
    U p[N_FIELDS];
    int w, h, qp, rounding, penalty;
};
static x266_mixed_t make(const Tuple &t)
{
    x266_mixed_t s;
    s.d_cur = (const x266_ref_block_t *)t.p[CUR];
    s.d_pred = (const x266_ref_block_t *)t.p[PRED];
    s.d_qp = (const uint8_t *)t.p[QP];
    s.d_kind_in = (const uint8_t *)t.p[KIND_IN];
    s.d_mode_in = (const uint8_t *)t.p[MODE_IN];
    s.d_level = (int16_t *)t.p[LEVEL];
    s.d_nnz = (uint32_t *)t.p[NNZ];
    s.d_kind = (uint8_t *)t.p[KIND];
    s.d_mode = (uint8_t *)t.p[MODE];
    s.d_cost = (uint32_t *)t.p[COST];
    s.d_recon = (x266_ref_block_t *)t.p[RECON];
    s.width = t.w;
    s.height = t.h;
    s.qp = t.qp;
    s.rounding = t.rounding;
    s.intra_penalty = t.penalty;
    return s;
}
// every pointer in a region of its own, at exactly its alignment times an odd number; a frame of 3 x 2 CTUs
static Tuple base()
{
    Tuple t;
    for (int i = 0; i < N_FIELDS; ++i) t.p[i] = ((U)(i + 1) << 44) + (U)FIELDS[i].align * (2 * i + 1);
    t.w = 192;
    t.h = 128;
    t.qp = 22;
    t.rounding = 171;
    t.penalty = 4096;
    return t;
}

static int g_checks = 0, g_failures = 0;
static void expect(const std::string &what, const char *got, bool refuse, const char *reason = nullptr)
{
    ++g_checks;
    if ((got != nullptr) == refuse && (!refuse || !reason || !std::strcmp(got, reason))) return;
    ++g_failures;
    std::printf("FAIL %s: %s: expected %s%s%s, got %s\n", CALL, what.c_str(), refuse ? "refuse" : "accept", refuse && reason ? " for " : "",
                refuse && reason ? reason : "", got ? got : "accept");
}
static const char *rule(const Tuple &t)
{
    const x266_mixed_t s = make(t);
    return args::mixed_code_frame(&s);
}
static U align_down(U x, unsigned a) { return x - x % a; }

// `without`: a bit per optional field that is NULL in this walk's base
static void walk(unsigned without)
{
    Tuple b = base();
    std::string at = "without";
    for (int f = 0; f < N_FIELDS; ++f)
        if ((without >> f) & 1u) {
            b.p[f] = 0;
            at += std::string(" ") + FIELDS[f].name;
        }
    at += ": ";
    expect(at + "base", rule(b), false);
    for (int f = 0; f < N_FIELDS; ++f) {
        if (!b.p[f]) continue;
        const std::string name = at + FIELDS[f].name;
        Tuple t = b;
        t.p[f] = 0;
        expect(name + " NULL", rule(t), !(FIELDS[f].flags & OPT), args::kNull);
        if (FIELDS[f].align > 1) {
            t = b;
            t.p[f] += FIELDS[f].align / 2;
            expect(name + " at half its alignment", rule(t), true, args::kMisaligned);
        }
        t = b;
        t.p[f] += FIELDS[f].align;                                              // aligned to exactly that, and to twice it: both fine
        expect(name + " one alignment further", rule(t), false);
        // the span's end against the end of the address space
        const size_t bytes = extent(f, b.w, b.h);
        t = b;
        t.p[f] = (U)0 - FIELDS[f].align;                                        // the last aligned address: every extent here is larger and wraps
        expect(name + " running past the top of the address space", rule(t), true, args::kNoFit);
        t = b;
        t.p[f] = align_down((U)0 - 2 * bytes, FIELDS[f].align);                 // high up, with room to spare
        expect(name + " near the top of the address space", rule(t), false);
        t.p[f] = align_down((U)0 - bytes - FIELDS[f].align, FIELDS[f].align);   // the span ends just below the top
        expect(name + " ending just below the top", rule(t), false);
        t.p[f] += 2 * FIELDS[f].align;
        expect(name + " two alignments further", rule(t), true, args::kNoFit);
        // overlap: field g moved onto the first byte, onto the last byte and right behind field f; refused when either is an output --
        // except the very same address of an output and the one input it may be
        for (int g = 0; g < N_FIELDS; ++g) {
            if (g == f || !b.p[g]) continue;
            const bool any_out = (FIELDS[f].flags & OUT) || (FIELDS[g].flags & OUT);
            const bool pair = FIELDS[f].same == g || FIELDS[g].same == f;
            const size_t gb = extent(g, b.w, b.h);
            t = b;
            t.p[g] = align_down(t.p[f], FIELDS[g].align);                       // g starts at or just before f's first byte, and is longer than that step
            if (gb <= t.p[f] - t.p[g]) ++g_failures, std::printf("FAIL the driver's own overlap case %s / %s\n", FIELDS[g].name, name.c_str());
            expect(std::string(FIELDS[g].name) + " over the start of " + name, rule(t), any_out && !(pair && t.p[g] == t.p[f]), args::kOverlap);
            t = b;
            t.p[g] = align_down(t.p[f] + bytes - 1, FIELDS[g].align);           // g's first byte among f's last
            expect(std::string(FIELDS[g].name) + " over the end of " + name, rule(t), any_out && !(pair && t.p[g] == t.p[f]), args::kOverlap);
            t = b;
            t.p[g] = align_down(t.p[f] + bytes + FIELDS[g].align - 1, FIELDS[g].align);   // right behind f
            expect(std::string(FIELDS[g].name) + " right behind " + name, rule(t), false);
            if (pair) {                                                         // one step off the allowed address is an overlap like any other
                t = b;
                t.p[g] = t.p[f] + FIELDS[g].align;
                expect(std::string(FIELDS[g].name) + " one alignment into " + name, rule(t), true, args::kOverlap);
            }
        }
    }
}

// the very same address twice, for every pair of fields: accepted for two inputs and for the three pairs of the header
static void same_address()
{
    const Tuple b = base();
    for (int f = 0; f < N_FIELDS; ++f)
        for (int g = 0; g < N_FIELDS; ++g) {
            if (g == f) continue;
            Tuple t = b;
            t.p[g] = t.p[f] = ((U)1 << 50) + 4096;                              // aligned for every field
            const bool any_out = (FIELDS[f].flags & OUT) || (FIELDS[g].flags & OUT);
            const bool pair = FIELDS[f].same == g || FIELDS[g].same == f;
            expect(std::string(FIELDS[g].name) + " == " + FIELDS[f].name, rule(t), any_out && !pair, args::kOverlap);
        }
    Tuple t = b;                                                                // the encoder's form: all three at once, the optional outputs NULL
    t.p[RECON] = t.p[PRED];
    t.p[KIND] = t.p[KIND_IN];
    t.p[MODE] = t.p[MODE_IN];
    expect("all three allowed overlaps", rule(t), false);
    t.p[NNZ] = t.p[COST] = 0;
    expect("all three allowed overlaps, d_nnz and d_cost NULL", rule(t), false);
    t.p[CUR] = t.p[PRED];                                                       // ... but then the source is the reconstruction
    expect("d_recon == d_pred == d_cur", rule(t), true, args::kOverlap);
    t = b;
    t.p[PRED] = t.p[CUR];
    expect("d_pred == d_cur", rule(t), false);
    t = b;
    t.p[KIND] = t.p[MODE_IN];
    expect("d_kind == d_mode_in", rule(t), true, args::kOverlap);
    t = b;
    t.p[MODE] = t.p[KIND_IN];
    expect("d_mode == d_kind_in", rule(t), true, args::kOverlap);
    t = b;
    t.p[RECON] = t.p[CUR];
    expect("d_recon == d_cur", rule(t), true, args::kOverlap);
}

static void sizes_and_scalars()
{
    const Tuple b = base();
    const char *const why = "width/height must be positive multiples of 64";
    const int bad[] = {0, -64, 8, 16, 32, 96, 191, 193, 200, INT_MIN, INT_MAX};
    for (int v : bad) {
        Tuple t = b;
        t.w = v;
        expect("width " + std::to_string(v), rule(t), true, why);
        t = b;
        t.h = v;
        expect("height " + std::to_string(v), rule(t), true, why);
    }
    const int good[][2] = {{64, 64}, {128, 64}, {64, 128}, {192, 128}, {64, 32768}, {1920, 1088}, {3840, 2176}, {7680, 4352}};
    for (const auto &g : good) {
        Tuple t = b;
        t.w = g[0];
        t.h = g[1];
        expect("frame " + std::to_string(g[0]) + "x" + std::to_string(g[1]), rule(t), false);
    }
    struct Scalar {
        const char *name;
        int Tuple::*field;
        int lo, hi;
        const char *reason;
    };
    const Scalar scalars[] = {{"qp", &Tuple::qp, 0, 51, args::kQuantScalars}, {"rounding", &Tuple::rounding, 0, 511, args::kQuantScalars},
                              {"intra_penalty", &Tuple::penalty, 0, 1 << 24, args::kMixedPenalty}};
    for (const Scalar &s : scalars) {
        const int values[] = {s.lo, s.hi, s.lo + 1, s.hi - 1, s.lo - 1, s.hi + 1, INT_MIN, INT_MAX};
        for (int v : values) {
            Tuple t = b;
            t.p[QP] = 0;                                                        // the scalar qp counts
            t.*(s.field) = v;
            expect(std::string(s.name) + " " + std::to_string(v), rule(t), v < s.lo || v > s.hi, s.reason);
        }
    }
    for (int qp = 0; qp <= 51; ++qp) {
        Tuple t = b;
        t.p[QP] = 0;
        t.qp = qp;
        expect("qp " + std::to_string(qp), rule(t), false);
    }
    const int any_qp[] = {-1, 52, 99, INT_MIN, INT_MAX};                        // with d_qp the scalar qp is not looked at; the rounding still is
    for (int v : any_qp) {
        Tuple t = b;
        t.qp = v;
        expect("qp " + std::to_string(v) + " under d_qp", rule(t), false);
        t.rounding = 512;
        expect("qp " + std::to_string(v) + " under d_qp, rounding 512", rule(t), true, args::kQuantScalars);
    }
    // the extents follow the frame: a buffer right behind another one of this frame is fine, one byte (alignment) earlier is not
    {
        Tuple t = b;
        t.p[COST] = t.p[NNZ] + extent(NNZ, b.w, b.h);
        expect("d_cost right behind d_nnz", rule(t), false);
        t.p[COST] -= 4;
        expect("d_cost on the last count", rule(t), true, args::kOverlap);
        t = b;
        t.p[MODE] = t.p[KIND] + extent(KIND, b.w, b.h);
        expect("d_mode right behind d_kind", rule(t), false);
        t.p[MODE] -= 1;
        expect("d_mode on the last kind", rule(t), true, args::kOverlap);
        t = b;
        t.p[LEVEL] = t.p[RECON] + extent(RECON, b.w, b.h);
        expect("d_level right behind d_recon", rule(t), false);
        t.p[LEVEL] -= 16;
        expect("d_level on the last tile", rule(t), true, args::kOverlap);
    }
    // the largest frame an int describes: its spans fit behind addresses of 2^44 and cover every buffer above them; high up they do not fit
    {
        const int side = INT_MAX - INT_MAX % 64;
        Tuple t = b;
        t.w = t.h = side;
        expect("the largest frame", rule(t), true, args::kOverlap);
        t.p[CUR] = (U)0 - ((U)1 << 40);
        expect("the largest frame, high up", rule(t), true, args::kNoFit);
    }
}

int main()
{
    expect("NULL p", args::mixed_code_frame(nullptr), true, "NULL parameter struct");
    const unsigned optional[] = {0u, 1u << QP, 1u << KIND_IN, 1u << MODE_IN, 1u << NNZ, 1u << COST,
                                 (1u << QP) | (1u << KIND_IN) | (1u << MODE_IN) | (1u << NNZ) | (1u << COST)};
    for (unsigned without : optional) walk(without);
    same_address();
    sizes_and_scalars();
    std::printf("mixed frame coding: %d checks, %d failures\n", g_checks, g_failures);
    if (g_failures) return 1;
    std::printf("the argument rules hold\n");
    return 0;
}
