// CPU check of the argument rules of the seeded search, xSatd8x8SeededSearchGpu (x266_amd/csrc/x266_args.hpp: seeded_search).  The call
// takes its device pointers in a host-read struct, so the one table of tests/cpp/arg_rules_check.cpp does not count it; this driver
// holds it the way tests/cpp/la_rules_check.cpp holds the lookahead's.  The rules are integer arithmetic on addresses and sizes: the
// addresses are made-up integers, nothing is dereferenced, no device is needed.
//
// FIELDS is the contract written down once more by hand from include/x266hip.h: every pointer field's alignment, whether it may be NULL
// and whether the call writes it.  One walk perturbs a base tuple one field at a time, at both seed scales; the expected verdict of every
// perturbation follows from that table, never from the function under test.
// Test infrastructure; built and run by tests/test_seed_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>

#include "x266_args.hpp"

using namespace x266;

typedef uintptr_t U;
enum Field { CUR, REF, SEED, BEST, J, N_FIELDS };
enum { IN = 0, OPT = 1, OUT = 2 };
static const char *const CALL = "xSatd8x8SeededSearchGpu";
struct Ptr {
    const char *name;
    unsigned align;
    int flags;
};
static const Ptr FIELDS[N_FIELDS] = {
    {"d_cur", 16, IN},
    {"d_ref", 16, IN},
    {"d_seed", 8, IN},
    {"d_best", 8, OUT},
    {"d_j", 4, OPT | OUT},
};
static size_t extent(int f, int w, int h, int scale)
{
    const size_t tiles = (size_t)(w / 16) * (size_t)(h / 16), blocks = (size_t)(w / 8) * (size_t)(h / 8);
    switch (f) {
    case CUR:
    case REF: return tiles * 512;
    case SEED: return (scale ? tiles : blocks) * 8;
    case BEST: return blocks * 8;
    default: return blocks * 4;
    }
}

struct Tuple {
    U p[N_FIELDS];
    int w, h, scale, centres, range, lambda;
};
static x266_seed_t make(const Tuple &t)
{
    x266_seed_t s;
    s.d_cur = (const x266_ref_block_t *)t.p[CUR];
    s.d_ref = (const x266_ref_block_t *)t.p[REF];
    s.d_seed = (const x266_me_result_t *)t.p[SEED];
    s.d_best = (x266_me_result_t *)t.p[BEST];
    s.d_j = (uint32_t *)t.p[J];
    s.width = t.w;
    s.height = t.h;
    s.seed_scale = t.scale;
    s.centres = t.centres;
    s.range = t.range;
    s.lambda_q4 = t.lambda;
    return s;
}
// every pointer in a region of its own, at exactly its alignment times an odd number; a frame of 10 x 6 tiles
static Tuple base(int scale)
{
    Tuple t;
    for (int i = 0; i < N_FIELDS; ++i) t.p[i] = ((U)(i + 1) << 44) + (U)FIELDS[i].align * (2 * i + 1);
    t.w = 160;
    t.h = 96;
    t.scale = scale;
    t.centres = 31;
    t.range = 2;
    t.lambda = 16;
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
    const x266_seed_t s = make(t);
    return args::seeded_search(&s);
}

static void walk(int scale)
{
    const Tuple b = base(scale);
    const std::string at = "seed_scale " + std::to_string(scale) + ": ";
    expect(at + "NULL p", args::seeded_search(nullptr), true, "NULL parameter struct");
    expect(at + "base", rule(b), false);
    for (int f = 0; f < N_FIELDS; ++f) {
        const std::string name = at + FIELDS[f].name;
        Tuple t = b;
        t.p[f] = 0;
        expect(name + " NULL", rule(t), !(FIELDS[f].flags & OPT), args::kNull);
        t = b;
        t.p[f] += FIELDS[f].align / 2;
        expect(name + " at half its alignment", rule(t), true, args::kMisaligned);
        t = b;
        t.p[f] += FIELDS[f].align;                                              // aligned to exactly that, and to twice it: both fine
        expect(name + " one alignment further", rule(t), false);
        // the span's end against the end of the address space
        const size_t bytes = extent(f, b.w, b.h, scale);
        t = b;
        t.p[f] = (U)0 - FIELDS[f].align;                                        // the last aligned address: every extent here is larger and wraps
        expect(name + " running past the top of the address space", rule(t), true, args::kNoFit);
        t = b;
        t.p[f] = ((U)0 - 2 * bytes) - ((U)0 - 2 * bytes) % FIELDS[f].align;     // high up, with room to spare
        expect(name + " near the top of the address space", rule(t), false);
        t.p[f] = ((U)0 - bytes - FIELDS[f].align) - ((U)0 - bytes - FIELDS[f].align) % FIELDS[f].align;   // the span ends just below the top
        expect(name + " ending just below the top", rule(t), false);
        t.p[f] += 2 * FIELDS[f].align;
        expect(name + " two alignments further", rule(t), true, args::kNoFit);
        // overlap: field g moved onto the first byte, and onto the last byte, of field f; refused when either is an output
        for (int g = 0; g < N_FIELDS; ++g) {
            if (g == f) continue;
            const bool any_out = (FIELDS[f].flags & OUT) || (FIELDS[g].flags & OUT);
            const size_t gb = extent(g, b.w, b.h, scale);
            t = b;
            t.p[g] = t.p[f] - t.p[f] % FIELDS[g].align;                         // g starts at or just before f's first byte, and is longer than that step
            if (gb <= t.p[f] - t.p[g]) ++g_failures, std::printf("FAIL the driver's own overlap case %s / %s\n", FIELDS[g].name, name.c_str());
            expect(std::string(FIELDS[g].name) + " over the start of " + name, rule(t), any_out, args::kOverlap);
            t = b;
            t.p[g] = t.p[f] + bytes - 1;
            t.p[g] -= t.p[g] % FIELDS[g].align;                                 // g's first byte among f's last
            expect(std::string(FIELDS[g].name) + " over the end of " + name, rule(t), any_out, args::kOverlap);
            t = b;
            t.p[g] = t.p[f] + bytes + FIELDS[g].align - 1;
            t.p[g] -= t.p[g] % FIELDS[g].align;                                 // right behind f
            expect(std::string(FIELDS[g].name) + " right behind " + name, rule(t), false);
        }
    }
    // the very same address twice: the two frames may be one; in place is refused, and so is d_j on anything
    {
        Tuple t = b;
        t.p[REF] = t.p[CUR];
        expect(at + "d_ref == d_cur", rule(t), false);
        t = b;
        t.p[BEST] = t.p[SEED];
        expect(at + "d_best == d_seed (in place)", rule(t), true, args::kOverlap);
        t = b;
        t.p[J] = t.p[BEST];
        expect(at + "d_j == d_best", rule(t), true, args::kOverlap);
        t = b;
        t.p[J] = t.p[SEED];
        expect(at + "d_j == d_seed", rule(t), true, args::kOverlap);
        t = b;
        t.p[J] = 0;
        t.p[REF] = t.p[CUR];
        expect(at + "d_j NULL and one frame", rule(t), false);
    }
    // frame sizes
    {
        const int bad[] = {0, -16, 8, 24, 152, 159, 161, INT_MIN, INT_MAX};
        for (int v : bad) {
            Tuple t = b;
            t.w = v;
            expect(at + "width " + std::to_string(v), rule(t), true, "width/height must be positive multiples of 16");
            t = b;
            t.h = v;
            expect(at + "height " + std::to_string(v), rule(t), true, "width/height must be positive multiples of 16");
        }
        const int good[][2] = {{16, 16}, {32, 16}, {16, 32}, {48, 32}, {96, 80}, {16, 32784}, {3840, 2176}, {7680, 4320}};
        for (const auto &g : good) {
            Tuple t = b;
            t.w = g[0];
            t.h = g[1];
            expect(at + "frame " + std::to_string(g[0]) + "x" + std::to_string(g[1]), rule(t), false);
        }
    }
    // scalars
    {
        struct Scalar {
            const char *name;
            int Tuple::*field;
            int lo, hi;
        };
        const Scalar scalars[] = {{"seed_scale", &Tuple::scale, 0, 1}, {"centres", &Tuple::centres, 0, 31}, {"range", &Tuple::range, 0, 8},
                                  {"lambda_q4", &Tuple::lambda, 0, 65535}};
        for (const Scalar &s : scalars) {
            const int values[] = {s.lo, s.hi, s.lo - 1, s.hi + 1, INT_MIN, INT_MAX};
            for (int v : values) {
                Tuple t = b;
                t.*(s.field) = v;
                expect(at + std::string(s.name) + " " + std::to_string(v), rule(t), v < s.lo || v > s.hi, args::kSeedScalars);
            }
        }
        for (int c = 0; c < 32; ++c)
            for (int r = 0; r <= 8; ++r) {
                Tuple t = b;
                t.centres = c;
                t.range = r;
                expect(at + "centres " + std::to_string(c) + ", range " + std::to_string(r), rule(t), false);
            }
    }
    // the seeds' extent follows the scale: a d_best right behind the seeds of this scale is fine, one inside them is not
    {
        Tuple t = b;
        t.p[BEST] = t.p[SEED] + extent(SEED, b.w, b.h, scale);
        expect(at + "d_best right behind the seeds", rule(t), false);
        t.p[BEST] -= 8;
        expect(at + "d_best on the last seed", rule(t), true, args::kOverlap);
    }
    // the largest frame an int describes: its spans fit behind addresses of 2^44 and cover every buffer above them; high up they do not fit
    {
        const int side = INT_MAX - INT_MAX % 16;
        Tuple t = b;
        t.w = t.h = side;
        expect(at + "the largest frame", rule(t), true, args::kOverlap);
        t.p[CUR] = (U)0 - ((U)1 << 40);
        expect(at + "the largest frame, high up", rule(t), true, args::kNoFit);
    }
}

int main()
{
    for (int scale = 0; scale < 2; ++scale) walk(scale);
    std::printf("the seeded search: %d checks, %d failures\n", g_checks, g_failures);
    if (g_failures) return 1;
    std::printf("the argument rules hold\n");
    return 0;
}
