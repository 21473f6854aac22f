// CPU check of the argument rules of xAqStatsGpu and xAqDecideGpu (x266_amd/csrc/x266_args.hpp: aq_stats, aq_decide).  The two calls take
// their device pointers in a host-read struct, so the one table of tests/cpp/arg_rules_check.cpp does not count them; this driver holds
// them the way tests/cpp/levels_rules_check.cpp holds the level stream's.  The rules are integer arithmetic on addresses and sizes: the
// addresses are made-up integers, nothing is dereferenced, no device is needed.
//
// FIELDS is the contract written down once more by hand from include/x266hip.h: every pointer field's alignment, whether it may be
// NULL, whether the call writes it, and its extent.  One walk perturbs a base tuple one field at a time; the expected verdict of
// every perturbation follows from that table, never from the functions under test.
// Test infrastructure; built and run by tests/test_aq_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>

#include "x266_args.hpp"

using namespace x266;

typedef uintptr_t U;
enum Field { SRC, TILE, TOTAL, OFFSET, QP, N_FIELDS };
enum { OPT = 1, OUT = 2, UNUSED = 4 };
struct Ptr {
    const char *name;
    unsigned align;
    int stats, decide;             // flags per call
};
static const Ptr FIELDS[N_FIELDS] = {
    {"d_src", 16, 0, UNUSED}, {"d_tile", 16, OUT, 0}, {"d_total", 8, OUT, 0}, {"d_offset", 2, UNUSED, OPT | OUT}, {"d_qp", 1, UNUSED, OPT | OUT},
};
static size_t extent(int f, int w, int h)
{
    const size_t n_tiles = (size_t)(w / 16) * (size_t)(h / 16), n_ctu = (size_t)((w + 63) / 64) * (size_t)((h + 63) / 64);
    switch (f) {
    case SRC: return n_tiles * 512;
    case TILE: return n_tiles * 32;
    case TOTAL: return 64;
    case OFFSET: return n_tiles * 2;
    default: return n_ctu * 6;
    }
}

struct Tuple {
    U p[N_FIELDS];
    int w, h, mode, strength, qp, chroma;
};
static x266_aq_t make(const Tuple &t)
{
    x266_aq_t s;
    s.d_src = (const x266_ref_block_t *)t.p[SRC];
    s.d_tile = (x266_aq_tile_t *)t.p[TILE];
    s.d_total = (int64_t *)t.p[TOTAL];
    s.d_offset = (int16_t *)t.p[OFFSET];
    s.d_qp = (uint8_t *)t.p[QP];
    s.width = t.w;
    s.height = t.h;
    s.mode = t.mode;
    s.strength_q8 = t.strength;
    s.qp = t.qp;
    s.chroma_qp_offset = t.chroma;
    return s;
}
// every pointer in a region of its own, at exactly its alignment times an odd number; a frame of 9 x 5 tiles, 3 x 2 CTUs
static Tuple base()
{
    Tuple t;
    for (int i = 0; i < N_FIELDS; ++i) t.p[i] = ((U)(i + 1) << 44) + (U)FIELDS[i].align * (2 * i + 1);
    t.w = 144;
    t.h = 80;
    t.mode = 2;
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

static void walk(bool decide)
{
    const char *call = decide ? "xAqDecideGpu" : "xAqStatsGpu";
    auto rule = [&](const Tuple &t) {
        const x266_aq_t s = make(t);
        return decide ? args::aq_decide(&s) : args::aq_stats(&s);
    };
    auto flags = [&](int f) { return decide ? FIELDS[f].decide : FIELDS[f].stats; };
    const Tuple b = base();
    expect(call, "NULL p", decide ? args::aq_decide(nullptr) : args::aq_stats(nullptr), true, "NULL parameter struct");
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
    // the two outputs of decide: either alone is enough, none is refused; stats looks at neither
    {
        Tuple t = b;
        t.p[OFFSET] = t.p[QP] = 0;
        expect(call, "d_offset and d_qp both NULL", rule(t), decide, "d_offset and d_qp are both NULL");
        t.p[OFFSET] = 3;
        t.p[QP] = (U)0 - 1;
        expect(call, "d_offset odd and d_qp at the last byte", rule(t), decide);
        t = b;
        t.p[SRC] = 8;
        expect(call, "d_src misaligned", rule(t), !decide, args::kMisaligned);
    }
    // frame sizes
    {
        const int bad[] = {0, -16, 8, 24, 143, 145, INT_MIN, INT_MAX};
        for (int v : bad) {
            Tuple t = b;
            t.w = v;
            expect(call, "width " + std::to_string(v), rule(t), true, "width/height must be positive multiples of 16");
            t = b;
            t.h = v;
            expect(call, "height " + std::to_string(v), rule(t), true, "width/height must be positive multiples of 16");
        }
        const int good[][2] = {{16, 16}, {48, 80}, {64, 64}, {16, 16400}, {3840, 2176}, {7680, 4320}};
        for (const auto &g : good) {
            Tuple t = b;
            t.w = g[0];
            t.h = g[1];
            expect(call, "frame " + std::to_string(g[0]) + "x" + std::to_string(g[1]), rule(t), false);
        }
    }
    // scalars: decide holds each to its range, stats reads none of them
    {
        struct Scalar {
            const char *name;
            int Tuple::*field;
            int lo, hi;
        };
        const Scalar scalars[] = {{"mode", &Tuple::mode, 1, 2}, {"strength_q8", &Tuple::strength, 0, 1024}, {"qp", &Tuple::qp, 0, 51},
                                  {"chroma_qp_offset", &Tuple::chroma, -12, 12}};
        for (const Scalar &s : scalars) {
            const int values[] = {s.lo, s.hi, s.lo - 1, s.hi + 1, INT_MIN, INT_MAX};
            for (int v : values) {
                Tuple t = b;
                t.*(s.field) = v;
                expect(call, std::string(s.name) + " " + std::to_string(v), rule(t), decide && (v < s.lo || v > s.hi), args::kAqScalars);
            }
        }
    }
    // the largest frame an int describes: 2^63 bytes of tiles and 2^59 of records fit behind an address of 2^44 and cover every buffer above
    // it; higher up they do not fit
    {
        const int side = INT_MAX - INT_MAX % 16;
        Tuple t = b;
        t.w = t.h = side;
        expect(call, "the largest frame", rule(t), true, args::kOverlap);
        const int first = decide ? TILE : SRC;
        t.p[first] = ((U)1 << 63) + ((U)1 << 40);
        if (decide) t.p[first] = (U)0 - ((U)1 << 58);
        expect(call, "the largest frame, high up", rule(t), true, args::kNoFit);
    }
}

int main()
{
    walk(false);
    walk(true);
    std::printf("xAqStatsGpu xAqDecideGpu: %d checks, %d failures\n", g_checks, g_failures);
    if (g_failures) return 1;
    std::printf("the argument rules hold\n");
    return 0;
}
