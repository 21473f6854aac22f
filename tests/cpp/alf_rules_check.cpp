// CPU check of the argument rules of the five adaptive-loop-filter calls (x266_amd/csrc/x266_args.hpp: alf_classify, alf_stats,
// alf_sum_stats, alf_decide, alf_apply).  As in bipred_rules_check.cpp the rule functions are integer arithmetic on addresses and
// sizes, so the addresses are made-up integers and nothing is dereferenced.  Per call: a base tuple that must be accepted, and single
// perturbations of it whose verdict follows from include/x266hip.h -- NULL, half the alignment, a span past the end of the address
// space, an output over every other buffer, sizes, counts, lambda_q4 and n_ctu one step inside and outside their ranges, and the set
// arrays that are not looked at when their count is 0.
// Test infrastructure; built and run by tests/test_alf_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
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
};
struct Scalars {
    int w = 80, h = 48, n_luma = 3, n_chroma = 8, lambda = 37;
    size_t n_ctu = 2;
};
typedef std::function<const char *(const std::vector<U> &, const Scalars &)> Rule;
struct Call {
    const char *name;
    std::vector<Ptr> ptrs;
    Rule rule;
    bool framed;            // takes width and height
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

// 80x48: 15 tiles, two CTUs (the second cut), 240 class bytes
static const size_t TILES = 80 * 48 * 2, NB = 20 * 12, STATS = 2 * 9432, CTRL = 6, TOTAL = 2358 * 8, LUMA = 3 * 600, CHROMA = 8 * 16;

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
            a = base(c);
            a[i] = a[j] = at;
            expect(n, std::string(p.name) + " == " + q.name, c.rule(a, s), true, args::kOverlap);
            a[j] = at;
            a[i] = at + q.bytes - al;                                       // the output's first bytes are the other's last
            if (q.bytes > al && (q.bytes - al) % p.align == 0) expect(n, std::string(p.name) + " over the end of " + q.name, c.rule(a, s), true, args::kOverlap);
            a[i] = at + q.bytes;                                            // adjacent: accepted
            if (q.bytes % p.align == 0) expect(n, std::string(p.name) + " right behind " + q.name, c.rule(a, s), false);
            a[i] = at;
            a[j] = at + p.bytes - al;                                       // the other's first bytes are the output's last
            if (p.bytes > al && (p.bytes - al) % q.align == 0) expect(n, std::string(q.name) + " over the end of " + p.name, c.rule(a, s), true, args::kOverlap);
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

static void scalar(const Call &c, const char *what, int Scalars::*field, int lo, int hi, const char *reason)
{
    for (int v : {lo - 1, lo, hi, hi + 1}) {
        Scalars s;
        s.*field = v;
        expect(c.name, std::string(what) + " " + std::to_string(v), c.rule(base(c), s), v < lo || v > hi, v < lo || v > hi ? reason : nullptr);
    }
}

// the counts at 8 and 9, and a count of 0 with any pointer at all
static void counts(const Call &c, size_t luma_at, size_t chroma_at)
{
    for (int k = 0; k < 2; ++k)
        for (int v : {8, 9}) {
            Scalars s;
            (k ? s.n_chroma : s.n_luma) = v;
            expect(c.name, std::string(k ? "n_chroma " : "n_luma ") + std::to_string(v), c.rule(base(c), s), v == 9, v == 9 ? args::kAlfCounts : nullptr);
        }
    for (U junk : {(U)0, (U)3, ~(U)0}) {
        Scalars s;
        s.n_luma = 0;
        std::vector<U> a = base(c);
        a[luma_at] = junk;
        expect(c.name, "n_luma 0 with d_luma " + std::to_string(junk), c.rule(a, s), false);
        s = Scalars();
        s.n_chroma = 0;
        a = base(c);
        a[chroma_at] = junk;
        expect(c.name, "n_chroma 0 with d_chroma " + std::to_string(junk), c.rule(a, s), false);
    }
}

int main()
{
    const Call classify = {"xAlfClassifyGpu", {{"d_dec", 16, 0, TILES}, {"d_class", 1, OUT, NB}},
                           [](const std::vector<U> &p, const Scalars &s) { return args::alf_classify(V(p[0]), s.w, s.h, V(p[1])); }, true};
    const Call stats = {"xAlfStatsGpu", {{"d_org", 16, 0, TILES}, {"d_dec", 16, 0, TILES}, {"d_class", 1, OPT, NB}, {"d_stats", 4, OUT, STATS}},
                        [](const std::vector<U> &p, const Scalars &s) { return args::alf_stats(V(p[0]), V(p[1]), s.w, s.h, V(p[2]), V(p[3])); }, true};
    const Call sum = {"xAlfSumStatsGpu", {{"d_stats", 4, 0, STATS}, {"d_mask", 1, OPT, 2}, {"d_total", 8, OUT, TOTAL}},
                      [](const std::vector<U> &p, const Scalars &s) { return args::alf_sum_stats(V(p[0]), s.n_ctu, V(p[1]), V(p[2])); }, false};
    const Call decide = {"xAlfDecideGpu", {{"d_stats", 4, 0, STATS}, {"d_luma", 4, 0, LUMA}, {"d_chroma", 4, 0, CHROMA}, {"d_ctrl", 1, OUT, CTRL}},
                         [](const std::vector<U> &p, const Scalars &s) {
                             return args::alf_decide(V(p[0]), s.n_ctu, V(p[1]), s.n_luma, V(p[2]), s.n_chroma, s.lambda, V(p[3]));
                         }, false};
    const Call apply = {"xAlfApplyGpu",
                        {{"d_in", 16, 0, TILES}, {"d_class", 1, OPT, NB}, {"d_luma", 4, 0, LUMA}, {"d_chroma", 4, 0, CHROMA}, {"d_ctrl", 1, 0, CTRL}, {"d_out", 16, OUT, TILES}},
                        [](const std::vector<U> &p, const Scalars &s) {
                            return args::alf_apply(V(p[0]), s.w, s.h, V(p[1]), V(p[2]), s.n_luma, V(p[3]), s.n_chroma, V(p[4]), V(p[5]));
                        }, true};
    for (const Call *c : {&classify, &stats, &sum, &decide, &apply}) {
        pointers(*c);
        if (c->framed) sizes(*c);
        std::printf("%s:", c->name);
        for (size_t i = 0; i < c->ptrs.size(); ++i) std::printf("%s %s %u", i ? "," : "", c->ptrs[i].name, c->ptrs[i].align);
        std::printf("\n");
    }
    counts(decide, 1, 2);
    counts(apply, 2, 3);
    scalar(decide, "n_luma", &Scalars::n_luma, 0, 8, args::kAlfCounts);
    scalar(decide, "n_chroma", &Scalars::n_chroma, 0, 8, args::kAlfCounts);
    scalar(apply, "n_luma", &Scalars::n_luma, 0, 8, args::kAlfCounts);
    scalar(apply, "n_chroma", &Scalars::n_chroma, 0, 8, args::kAlfCounts);
    scalar(decide, "lambda_q4", &Scalars::lambda, 0, 65535, "lambda_q4 must be 0..65535");
    for (const Call *c : {&sum, &decide}) {
        Scalars s;
        s.n_ctu = 0;                                                        // accepted by the rules; the entry point then launches nothing
        expect(c->name, "n_ctu 0", c->rule(base(*c), s), false);
        s.n_ctu = (size_t)0x7FFFFFFF;
        expect(c->name, "n_ctu 2^31 - 1", c->rule(base(*c), s), false);
        s.n_ctu = (size_t)0x80000000ull;
        expect(c->name, "n_ctu 2^31", c->rule(base(*c), s), true, "n_ctu must be below 2^31");
        s.n_ctu = ~(size_t)0;
        expect(c->name, "n_ctu 2^64 - 1", c->rule(base(*c), s), true, "n_ctu must be below 2^31");
    }
    {   // the two frames of the statistics are read-only and may be one
        std::vector<U> a = base(stats);
        a[0] = a[1];
        expect(stats.name, "d_org == d_dec", stats.rule(a, Scalars()), false);
    }
    std::printf("%d checks, %d failures\n", g_checks, g_failures);
    if (g_failures) return 1;
    std::printf("the adaptive loop filter argument rules hold\n");
    return 0;
}
