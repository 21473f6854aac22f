// CPU check of the argument rules of xRdoQuantRegionsGpu and xLevelsBitsGpu (x266_amd/csrc/x266_args.hpp: rdoq_regions, levels_bits).
// The two calls take their device pointers in a host-read struct, so the one table of tests/cpp/arg_rules_check.cpp does not count
// them; this driver holds them the way tests/cpp/levels_rules_check.cpp holds the level stream's.  The rules are integer arithmetic on
// addresses and sizes: the addresses are made-up integers, nothing is dereferenced, no device is needed.
//
// FIELDS is the contract written down once more by hand from include/x266hip.h: every pointer field's alignment, whether it may be
// NULL, whether the call writes it, and its extent.  One walk perturbs a base tuple one field at a time; the expected verdict of
// every perturbation follows from that table, never from the functions under test.
// Test infrastructure; built and run by tests/test_rdoq_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <cstdio>
#include <cstring>
#include <string>

#include "x266_args.hpp"

using namespace x266;

typedef uintptr_t U;
enum Field { COEF, LEVEL, CLASS, QP, NNZ, STAT, N_FIELDS };
enum { OPT = 1, OUT = 2, UNUSED = 4 };
struct Ptr {
    const char *name;
    unsigned align;
    int rdoq, bits;                // flags per call
};
static const Ptr FIELDS[N_FIELDS] = {
    {"d_coef", 16, 0, UNUSED}, {"d_level", 16, OUT, 0},        {"d_class", 1, OPT, OPT},
    {"d_qp", 1, OPT, UNUSED},  {"d_nnz", 4, OPT | OUT, OPT},   {"d_stat", 8, OPT | OUT, OUT},
};
static size_t extent(int f, size_t n)
{
    switch (f) {
    case COEF: case LEVEL: return n * 2048;
    case CLASS: case QP: return n;
    case NNZ: return n * 4;
    default: return n * 16;
    }
}

struct Tuple {
    U p[N_FIELDS];
    size_t n;
    int qp, lambda;
};
static x266_rdoq_t make(const Tuple &t)
{
    x266_rdoq_t s;
    s.d_coef = (const int16_t *)t.p[COEF];
    s.d_level = (int16_t *)t.p[LEVEL];
    s.d_class = (const uint8_t *)t.p[CLASS];
    s.d_qp = (const uint8_t *)t.p[QP];
    s.d_nnz = (uint32_t *)t.p[NNZ];
    s.d_stat = (x266_rdoq_region_t *)t.p[STAT];
    s.n_regions = t.n;
    s.qp = t.qp;
    s.lambda = t.lambda;
    return s;
}
// every pointer in a region of its own, at exactly its alignment times an odd number
static Tuple base()
{
    Tuple t;
    for (int i = 0; i < N_FIELDS; ++i) t.p[i] = ((U)(i + 1) << 44) + (U)FIELDS[i].align * (2 * i + 1);
    t.n = 7;
    t.qp = 30;
    t.lambda = 368;
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

static void walk(bool bits)
{
    const char *call = bits ? "xLevelsBitsGpu" : "xRdoQuantRegionsGpu";
    auto rule = [&](const Tuple &t) {
        const x266_rdoq_t s = make(t);
        return bits ? args::levels_bits(&s) : args::rdoq_regions(&s);
    };
    auto flags = [&](int f) { return bits ? FIELDS[f].bits : FIELDS[f].rdoq; };
    expect(call, "NULL p", bits ? args::levels_bits(nullptr) : args::rdoq_regions(nullptr), true, "NULL parameter struct");
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
        const size_t bytes = extent(f, base().n);
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
            const bool in_place_pair = !bits && ((f == COEF && g == LEVEL) || (f == LEVEL && g == COEF));
            const size_t gb = extent(g, base().n);
            t = base();
            t.p[g] = t.p[f] - t.p[f] % FIELDS[g].align;                         // g starts at or just before f's first byte, and is longer than that step
            if (gb <= t.p[f] - t.p[g]) ++g_failures, std::printf("FAIL the driver's own overlap case %s / %s\n", FIELDS[g].name, name.c_str());
            // d_level == d_coef, the very same address, is the one overlap that is allowed
            expect(call, std::string(FIELDS[g].name) + " over the start of " + name, rule(t), both && any_out && !(in_place_pair && t.p[g] == t.p[f]),
                   args::kOverlap);
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
    // in place: d_level == d_coef is accepted by the optimisation, one chunk apart is not
    {
        Tuple t = base();
        t.p[LEVEL] = t.p[COEF];
        expect(call, "d_level == d_coef", rule(t), false);
        t.p[LEVEL] = t.p[COEF] + 16;
        expect(call, "d_level one chunk into d_coef", rule(t), !bits, args::kOverlap);
        t.p[LEVEL] = t.p[COEF] - 16;
        expect(call, "d_level one chunk before d_coef", rule(t), !bits, args::kOverlap);
    }
    // the scalars: looked at by the optimisation alone, qp only without d_qp
    {
        const int lambdas[] = {-1, 0, 8192, 8193};
        for (int l : lambdas) {
            Tuple t = base();
            t.lambda = l;
            expect(call, "lambda " + std::to_string(l), rule(t), !bits && (l < 0 || l > 8192), args::kRdoqScalars);
        }
        const int qps[] = {-1, 0, 51, 52};
        for (int q : qps) {
            Tuple t = base();
            t.qp = q;
            expect(call, "qp " + std::to_string(q) + " beside d_qp", rule(t), false);
            t.p[QP] = 0;
            expect(call, "qp " + std::to_string(q) + " without d_qp", rule(t), !bits && (q < 0 || q > 51), args::kRdoqScalars);
        }
    }
    // n_regions == 0: nothing is looked at
    {
        Tuple t = base();
        t.n = 0;
        t.qp = 99;
        t.lambda = -1;
        for (int f = 0; f < N_FIELDS; ++f) t.p[f] = f % 2 ? 0 : 3;              // NULL or misaligned
        expect(call, "no regions, the pointers NULL or odd, the scalars out of range", rule(t), false);
    }
    // extents that saturate: no pointer has room for them
    {
        Tuple t = base();
        t.n = SIZE_MAX / 2048 + 1;                                              // n * 2048 wraps size_t
        expect(call, "n_regions * 2048 wraps", rule(t), true, args::kNoFit);
        t.n = SIZE_MAX / 16 + 1;                                                // n * 16 wraps too
        expect(call, "n_regions * 16 wraps", rule(t), true, args::kNoFit);
        t.n = ((size_t)1 << 52);                                                // 2^63 bytes of levels behind an address of 2^45: fits, and covers everything above it
        expect(call, "2^52 regions", rule(t), true, args::kOverlap);
    }
}

int main()
{
    walk(false);
    walk(true);
    std::printf("xRdoQuantRegionsGpu xLevelsBitsGpu: %d checks, %d failures\n", g_checks, g_failures);
    if (g_failures) return 1;
    std::printf("the argument rules hold\n");
    return 0;
}
