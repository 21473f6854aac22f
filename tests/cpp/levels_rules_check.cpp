// CPU check of the argument rules of xLevelsPackGpu and xLevelsUnpackGpu (x266_amd/csrc/x266_args.hpp: levels_pack, levels_unpack).
// The two calls take their device pointers in a host-read struct, so the one table of tests/cpp/arg_rules_check.cpp does not count
// them; this driver holds them in the same way until that table can grow.  The rules are integer arithmetic on addresses and sizes:
// the addresses are made-up integers, nothing is dereferenced, no device is needed.
//
// FIELDS is the contract written down once more by hand from include/x266hip.h: every pointer field's alignment, whether it may be
// NULL, whether the call writes it, and its extent.  One walk perturbs a base tuple one field at a time; the expected verdict of
// every perturbation follows from that table, never from the functions under test.
// Test infrastructure; built and run by tests/test_levels_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "x266_args.hpp"

using namespace x266;

typedef uintptr_t U;
enum Field { LEVEL, CLASS, NNZ, REGION, STREAM, TOTAL, N_FIELDS };
enum { OPT = 1, OUT = 2, UNUSED = 4 };
struct Ptr {
    const char *name;
    unsigned align;
    int pack, unpack;              // flags per call
};
static const Ptr FIELDS[N_FIELDS] = {
    {"d_level", 16, 0, OUT},  {"d_class", 1, OPT, OPT}, {"d_nnz", 4, OPT, OPT | OUT},
    {"d_region", 8, OUT, 0},  {"d_stream", 16, OUT, 0}, {"d_total", 8, OUT, UNUSED},
};
static size_t extent(int f, size_t n, uint64_t cap)
{
    switch (f) {
    case LEVEL: return n * 2048;
    case CLASS: return n;
    case NNZ: return n * 4;
    case REGION: return n * 32;
    case STREAM: return (size_t)cap * 2;
    default: return 16;
    }
}

struct Tuple {
    U p[N_FIELDS];
    size_t n;
    uint64_t cap;
};
static x266_levels_t make(const Tuple &t)
{
    x266_levels_t s;
    s.d_level = (int16_t *)t.p[LEVEL];
    s.d_class = (const uint8_t *)t.p[CLASS];
    s.d_nnz = (uint32_t *)t.p[NNZ];
    s.d_region = (x266_level_region_t *)t.p[REGION];
    s.d_stream = (uint16_t *)t.p[STREAM];
    s.d_total = (uint64_t *)t.p[TOTAL];
    s.n_regions = t.n;
    s.cap_words = t.cap;
    return s;
}
// every pointer in a region of its own, at exactly its alignment times an odd number
static Tuple base()
{
    Tuple t;
    for (int i = 0; i < N_FIELDS; ++i) t.p[i] = ((U)(i + 1) << 44) + (U)FIELDS[i].align * (2 * i + 1);
    t.n = 7;
    t.cap = 5000;
    return t;
}

static int g_checks = 0, g_failures = 0;
static void expect(const char *call, const std::string &what, const char *got, bool refuse, const char *reason = nullptr)
{
    ++g_checks;
    if ((got != nullptr) == refuse && (!reason || !got || !std::strcmp(got, reason))) return;
    ++g_failures;
    std::printf("FAIL %s: %s: expected %s%s%s, got %s\n", call, what.c_str(), refuse ? "refuse" : "accept", reason ? " for " : "", reason ? reason : "",
                got ? got : "accept");
}

static void walk(bool unpack)
{
    const char *call = unpack ? "xLevelsUnpackGpu" : "xLevelsPackGpu";
    auto rule = [&](const Tuple &t) {
        const x266_levels_t s = make(t);
        return unpack ? args::levels_unpack(&s) : args::levels_pack(&s);
    };
    auto flags = [&](int f) { return unpack ? FIELDS[f].unpack : FIELDS[f].pack; };
    expect(call, "NULL p", unpack ? args::levels_unpack(nullptr) : args::levels_pack(nullptr), true, "NULL parameter struct");
    expect(call, "base", rule(base()), false);
    for (int f = 0; f < N_FIELDS; ++f) {
        const std::string name = FIELDS[f].name;
        const bool used = !(flags(f) & UNUSED);
        Tuple t = base();
        t.p[f] = 0;
        expect(call, name + " NULL", rule(t), used && !(flags(f) & OPT), args::kNull);
        if (FIELDS[f].align > 1) {
            t = base();
            t.p[f] += FIELDS[f].align / 2;
            expect(call, name + " at half its alignment", rule(t), used, args::kMisaligned);
            t = base();
            t.p[f] += FIELDS[f].align;                                          // aligned to exactly that, and to twice it: both fine
            expect(call, name + " one alignment further", rule(t), false);
        } else {
            t = base();
            t.p[f] += 1;
            expect(call, name + " at an odd address", rule(t), false);
        }
        // the span's end against the end of the address space
        const size_t bytes = extent(f, base().n, base().cap);
        t = base();
        t.p[f] = (U)0 - FIELDS[f].align;                                        // the last aligned address: every extent here is larger and wraps
        expect(call, name + " running past the top of the address space", rule(t), used && bytes > FIELDS[f].align, args::kNoFit);
        t = base();
        t.p[f] = ((U)0 - 2 * bytes) - ((U)0 - 2 * bytes) % FIELDS[f].align;     // high up, with room to spare
        expect(call, name + " near the top of the address space", rule(t), false);
        // overlap: field g moved onto the first byte, and onto the last byte, of field f; refused when either is an output
        for (int g = 0; g < N_FIELDS; ++g) {
            if (g == f) continue;
            const bool both = used && !(flags(g) & UNUSED), any_out = (flags(f) & OUT) || (flags(g) & OUT);
            const size_t gb = extent(g, base().n, base().cap);
            t = base();
            t.p[g] = t.p[f] - t.p[f] % FIELDS[g].align;                         // g starts at or just before f's first byte, and is longer than that step
            if (gb <= t.p[f] - t.p[g]) ++g_failures, std::printf("FAIL the driver's own overlap case %s / %s\n", FIELDS[g].name, name.c_str());
            expect(call, std::string(FIELDS[g].name) + " over the start of " + name, rule(t), both && any_out, args::kOverlap);
            t = base();
            t.p[g] = t.p[f] + bytes - 1;
            t.p[g] -= t.p[g] % FIELDS[g].align;                                 // g's first byte among f's last
            expect(call, std::string(FIELDS[g].name) + " over the end of " + name, rule(t), both && any_out, args::kOverlap);
            t = base();
            t.p[g] = t.p[f] + bytes + FIELDS[g].align - 1;
            t.p[g] -= t.p[g] % FIELDS[g].align;                                 // right behind f
            expect(call, std::string(FIELDS[g].name) + " right behind " + name, rule(t), false);
        }
    }
    // n_regions == 0: pack looks at d_total alone, unpack at nothing
    {
        Tuple t = base();
        t.n = 0;
        for (int f = 0; f < N_FIELDS; ++f)
            if (f != TOTAL) t.p[f] = f % 2 ? 0 : 3;                             // NULL or misaligned: not looked at
        expect(call, "no regions, the other pointers NULL or odd", rule(t), false);
        t.p[TOTAL] = 0;
        expect(call, "no regions, d_total NULL", rule(t), !unpack, args::kNull);
        t.p[TOTAL] = base().p[TOTAL] + 4;
        expect(call, "no regions, d_total misaligned", rule(t), !unpack, args::kMisaligned);
    }
    // cap_words == 0: d_stream may be NULL (pack: the count-only call), and is still held to its alignment when given
    {
        Tuple t = base();
        t.cap = 0;
        expect(call, "no capacity", rule(t), false);
        t.p[STREAM] = 0;
        expect(call, "no capacity, d_stream NULL", rule(t), false);
        t.p[STREAM] = base().p[STREAM] + 8;
        expect(call, "no capacity, d_stream misaligned", rule(t), true, args::kMisaligned);
        t = base();
        t.cap = 1;
        t.p[STREAM] = 0;
        expect(call, "one word of capacity, d_stream NULL", rule(t), true, args::kNull);
    }
    // extents that saturate: no pointer has room for them
    {
        Tuple t = base();
        t.n = SIZE_MAX / 2048 + 1;                                              // n * 2048 wraps size_t
        expect(call, "n_regions * 2048 wraps", rule(t), true, args::kNoFit);
        t.n = SIZE_MAX / 32 + 1;                                                // n * 32 wraps too
        expect(call, "n_regions * 32 wraps", rule(t), true, args::kNoFit);
        t.n = ((size_t)1 << 52);                                                // 2^63 bytes of levels behind an address of 2^44: fits, and covers everything above it
        expect(call, "2^52 regions", rule(t), true, args::kOverlap);
        t = base();
        t.cap = UINT64_MAX;
        expect(call, "cap_words * 2 wraps", rule(t), true, args::kNoFit);
        t.cap = (uint64_t)1 << 63;
        expect(call, "cap_words = 2^63", rule(t), true, args::kNoFit);
    }
}

int main()
{
    walk(false);
    walk(true);
    std::printf("xLevelsPackGpu xLevelsUnpackGpu: %d checks, %d failures\n", g_checks, g_failures);
    if (g_failures) return 1;
    std::printf("the argument rules hold\n");
    return 0;
}
