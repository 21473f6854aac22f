// CPU check of the argument rules of the three bi-directional calls (x266_amd/csrc/x266_args.hpp: mc_bi_qpel, bi_costs,
// refine_bi_qpel).  As in arg_rules_check.cpp the rule functions are integer arithmetic on addresses and sizes, so the addresses
// are made-up integers and nothing is dereferenced.  Per call: a base tuple that must be accepted, and single perturbations of it
// whose verdict follows from include/x266hip.h -- NULL, half the alignment, a span past the end of the address space, an output over
// every other buffer, the allowed aliases, sizes, and every scalar and x266_wp_t field one step inside and outside its range.
// Test infrastructure; built and run by tests/test_bipred_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "x266_args.hpp"

using namespace x266;

typedef uintptr_t U;
static const void *V(U x) { return (const void *)x; }

enum { OPT = 1, OUT = 2 };
struct Ptr {
    const char *name;
    unsigned align;
    int flags;
    size_t bytes;           // at the base size
    const char *alias;      // the input this output may exactly be
};
struct Scalars {
    int w = 32, h = 16, planes = 3, penalty = 7, list = 1;
    const x266_wp_t *wp = nullptr;
};
typedef std::function<const char *(const std::vector<U> &, const Scalars &)> Rule;
struct Call {
    const char *name;
    std::vector<Ptr> ptrs;
    Rule rule;
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

// 32x16: two tiles (1024 bytes), eight 8x8 blocks
static const size_t TILES = 32 * 16 * 2, NB = 8;

static std::vector<U> base(const Call &c)
{
    std::vector<U> p;
    for (size_t i = 0; i < c.ptrs.size(); ++i) p.push_back(((U)(i + 1) << 44) + (U)c.ptrs[i].align * (2 * i + 1));   // exactly its alignment, no more
    return p;
}

static void pointers(const Call &c)
{
    const char *n = c.name;
    const Scalars s;
    expect(n, "base", c.rule(base(c), s), false);
    for (size_t i = 0; i < c.ptrs.size(); ++i) {
        const Ptr &p = c.ptrs[i];
        std::vector<U> a = base(c);
        a[i] = 0;
        expect(n, std::string(p.name) + " NULL", c.rule(a, s), !(p.flags & OPT), (p.flags & OPT) ? nullptr : args::kNull);
        if (p.align > 1) {
            a = base(c);
            a[i] += p.align / 2;
            expect(n, std::string(p.name) + " at half its alignment", c.rule(a, s), true, args::kMisaligned);
        }
        a = base(c);
        a[i] = (U)0 - p.bytes;                                             // the span ends exactly at 2^64: one byte too far
        a[i] -= a[i] % p.align;
        a[i] += p.align;
        if (a[i] != 0) expect(n, std::string(p.name) + " runs past the address space", c.rule(a, s), true, args::kNoFit);
        a = base(c);
        a[i] = ((U)0 - p.bytes - 4096) & ~(U)15;
        expect(n, std::string(p.name) + " ends below the top", c.rule(a, s), false);
        if (!(p.flags & OUT)) continue;
        for (size_t j = 0; j < c.ptrs.size(); ++j) {
            if (j == i) continue;
            const Ptr &q = c.ptrs[j];
            const unsigned al = p.align > q.align ? p.align : q.align;
            const U at = ((U)9 << 44);                                      // both aligned here
            const bool may_alias = p.alias && !std::strcmp(p.alias, q.name);
            a = base(c);
            a[i] = a[j] = at;
            expect(n, std::string(p.name) + " == " + q.name, c.rule(a, s), !may_alias, may_alias ? nullptr : args::kOverlap);
            a[j] = at;
            a[i] = at + q.bytes - al;                                       // the output's first bytes are the other's last
            if (q.bytes > al) expect(n, std::string(p.name) + " over the end of " + q.name, c.rule(a, s), true, args::kOverlap);
            a[i] = at + q.bytes;                                            // adjacent: accepted
            if (q.bytes % p.align == 0) expect(n, std::string(p.name) + " right behind " + q.name, c.rule(a, s), false);
            a[i] = at;
            a[j] = at + p.bytes - al;                                       // the other's first bytes are the output's last
            if (p.bytes > al) expect(n, std::string(q.name) + " over the end of " + p.name, c.rule(a, s), true, args::kOverlap);
        }
    }
}

static void sizes(const Call &c)
{
    for (int dim = 0; dim < 2; ++dim)
        for (int v : {0, -16, 8, 24}) {
            Scalars s;
            (dim ? s.h : s.w) = v;
            expect(c.name, std::string(dim ? "height " : "width ") + std::to_string(v), c.rule(base(c), s), true, "width/height must be positive multiples of 16");
        }
    Scalars s;
    s.w = 16;
    s.h = 16;                                                               // a smaller frame fits wherever the base fits
    expect(c.name, "one tile", c.rule(base(c), s), false);
}

static void weights(const Call &c)
{
    const x266_wp_t ok = {{{-128, 127, 1}, {0, -128, 127}}, {{127, -128, 0}, {-128, 127, 5}}, {0, 7}};
    Scalars s;
    s.wp = &ok;
    expect(c.name, "wp at the ends of every range", c.rule(base(c), s), false);
    for (int l = 0; l < 2; ++l)
        for (int k = 0; k < 3; ++k)
            for (int v : {-129, 128, 32767, -32768}) {
                x266_wp_t bad = ok;
                bad.w[l][k] = (int16_t)v;
                s.wp = &bad;
                expect(c.name, "wp.w out of range", c.rule(base(c), s), true, args::kWp);
                bad = ok;
                bad.o[l][k] = (int16_t)v;
                s.wp = &bad;
                expect(c.name, "wp.o out of range", c.rule(base(c), s), true, args::kWp);
            }
    for (int k = 0; k < 2; ++k)
        for (int v : {8, 255}) {
            x266_wp_t bad = ok;
            bad.log2_denom[k] = (uint8_t)v;
            s.wp = &bad;
            expect(c.name, "wp.log2_denom out of range", c.rule(base(c), s), true, args::kWp);
        }
}

static void scalar(const Call &c, const char *what, int Scalars::*field, int lo, int hi)
{
    for (int v : {lo - 1, lo, hi, hi + 1}) {
        Scalars s;
        s.*field = v;
        expect(c.name, std::string(what) + " " + std::to_string(v), c.rule(base(c), s), v < lo || v > hi);
    }
}

int main()
{
    const Call mc = {"xMotionCompBiQpelTiles",
                     {{"d_ref0", 16, 0, TILES, nullptr}, {"d_ref1", 16, 0, TILES, nullptr}, {"d_mv0", 8, 0, NB * 8, nullptr}, {"d_mv1", 8, 0, NB * 8, nullptr},
                      {"d_dir", 1, OPT, NB, nullptr}, {"d_pred", 16, OUT, TILES, nullptr}},
                     [](const std::vector<U> &p, const Scalars &s) {
                         return args::mc_bi_qpel(V(p[0]), V(p[1]), V(p[2]), V(p[3]), V(p[4]), s.wp, s.planes, s.w, s.h, V(p[5]));
                     }};
    const Call costs = {"xSatd8x8BiCostsFromTiles",
                        {{"d_cur", 16, 0, TILES, nullptr}, {"d_ref0", 16, 0, TILES, nullptr}, {"d_ref1", 16, 0, TILES, nullptr}, {"d_mv0", 8, 0, NB * 8, nullptr},
                         {"d_mv1", 8, 0, NB * 8, nullptr}, {"d_costs", 4, OPT | OUT, NB * 12, nullptr}, {"d_dir", 1, OPT | OUT, NB, nullptr}},
                        [](const std::vector<U> &p, const Scalars &s) {
                            return args::bi_costs(V(p[0]), V(p[1]), V(p[2]), s.w, s.h, V(p[3]), V(p[4]), s.wp, s.penalty, V(p[5]), V(p[6]));
                        }};
    const Call refine = {"xSatd8x8RefineBiQpelFromTiles",
                         {{"d_cur", 16, 0, TILES, nullptr}, {"d_ref_fix", 16, 0, TILES, nullptr}, {"d_mv_fix", 8, 0, NB * 8, nullptr}, {"d_ref", 16, 0, TILES, nullptr},
                          {"d_int", 8, 0, NB * 8, nullptr}, {"d_best", 8, OUT, NB * 8, "d_int"}, {"d_costs", 4, OPT | OUT, NB * 49 * 4, nullptr}},
                         [](const std::vector<U> &p, const Scalars &s) {
                             return args::refine_bi_qpel(V(p[0]), V(p[1]), V(p[2]), V(p[3]), V(p[4]), s.list, s.wp, s.w, s.h, V(p[5]), V(p[6]));
                         }};
    for (const Call *c : {&mc, &costs, &refine}) {
        pointers(*c);
        sizes(*c);
        weights(*c);
        std::printf("%s:", c->name);
        for (size_t i = 0; i < c->ptrs.size(); ++i) std::printf("%s %s %u", i ? "," : "", c->ptrs[i].name, c->ptrs[i].align);
        std::printf("\n");
    }
    scalar(mc, "planes", &Scalars::planes, 1, 3);
    scalar(costs, "bi_penalty", &Scalars::penalty, 0, 65535);
    scalar(refine, "list", &Scalars::list, 0, 1);
    {   // the inputs may be one frame; both outputs of the cost call NULL is refused, either alone is accepted
        std::vector<U> a = base(mc);
        a[1] = a[0];
        expect(mc.name, "d_ref1 == d_ref0", mc.rule(a, Scalars()), false);
        a = base(costs);
        a[5] = a[6] = 0;
        expect(costs.name, "both outputs NULL", costs.rule(a, Scalars()), true);
        a = base(costs);
        a[0] = a[1] = a[2];
        expect(costs.name, "one frame three times", costs.rule(a, Scalars()), false);
        a = base(refine);
        a[1] = a[3] = a[0];
        expect(refine.name, "one frame three times", refine.rule(a, Scalars()), false);
        a = base(refine);
        a[5] = a[2];
        expect(refine.name, "d_best == d_mv_fix", refine.rule(a, Scalars()), true, args::kOverlap);
    }
    std::printf("%d checks, %d failures\n", g_checks, g_failures);
    if (g_failures) return 1;
    std::printf("the bi-directional argument rules hold\n");
    return 0;
}
