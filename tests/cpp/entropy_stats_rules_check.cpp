// CPU check of the argument rules of xEntropyStatsLevelsGpu and xEntropyStatsSideGpu (x266_amd/csrc/x266_args.hpp: entropy_stats_levels,
// entropy_stats_side), the calls whose device pointers are the fields of the host-read x266_entropy_stats_t and x266_entropy_side_stats_t,
// and of what the statistics share with the host through x266_amd/csrc/x266_entropy.hpp and x266_entropy_side.hpp: the table rule and
// the counting sink under the two syntax walks, run here as plain C++ against literals.  The contract is written down once more by hand
// from the header -- per call the pointer fields in struct order with their alignments, which are written, which may be NULL, their
// extents -- and one walk perturbs a base tuple one field at a time: NULL, half an alignment, one alignment further, the top of the address
// space, every overlap of an output with any other buffer, d_kind without d_mode, qp at -1 and 52, chroma_qp_offset at -13 and 13, counts
// that saturate, no unit at all.
// The addresses are made-up integers, nothing is dereferenced, no device is needed; the expected verdict of every check follows from
// these tables and from literals, never from the function under test.
// Test infrastructure; built and run by tests/test_entropy_stats_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <climits>
#include <cstddef>
#include <string>
#include <vector>

#include "rules_expect.hpp"
#include "x266_args.hpp"
#include "x266_entropy_side.hpp"

using namespace x266;

static const char *SHARED = "x266_entropy.hpp";
enum { MAX_FIELDS = 7 };
struct Field {
    const char *name;
    unsigned align;
    bool output, optional;
    size_t per_unit;                                                        // bytes per region or CTU; 0: d_counts and d_part, see extent()
};
struct Call {
    const char *name;
    int n_fields, counts, part;                                             // the indices of d_counts and d_part
    size_t per_row, contexts;
    Field f[MAX_FIELDS];
};
static const Call CALLS[2] = {
    {"xEntropyStatsLevelsGpu", 5, 3, 4, 32, 100,
     {{"d_level", 16, false, false, 2048}, {"d_class", 1, false, true, 1}, {"d_nnz", 4, false, true, 4}, {"d_counts", 8, true, false, 0}, {"d_part", 16, true, false, 0}}},
    {"xEntropyStatsSideGpu", 7, 5, 6, 64, 16,
     {{"d_kind", 1, false, true, 6}, {"d_mode", 1, false, true, 6}, {"d_class", 1, false, true, 6}, {"d_qp", 1, false, true, 6}, {"d_nnz", 4, false, true, 24},
      {"d_counts", 8, true, false, 0}, {"d_part", 16, true, false, 0}}}};
struct Tuple {
    U p[MAX_FIELDS];
    size_t n;
    int qp, off;
};

static size_t times(size_t a, size_t b) { return b && a > SIZE_MAX / b ? SIZE_MAX : a * b; }
static size_t rows_of(size_t n, size_t per_row) { return n / per_row + (n % per_row != 0); }
static size_t extent(const Call &c, int f, const Tuple &t)
{
    if (f == c.counts) return 16 * c.contexts;
    if (f == c.part) return times(rows_of(t.n, c.per_row), 8 * c.contexts);
    return times(t.n, c.f[f].per_unit);
}
static const char *rule(int call, const Tuple &t)
{
    if (call == 0) {
        x266_entropy_stats_t s = {};
        s.d_level = (const int16_t *)t.p[0];
        s.d_class = (const uint8_t *)t.p[1];
        s.d_nnz = (const uint32_t *)t.p[2];
        s.d_counts = (uint64_t *)t.p[3];
        s.d_part = (uint32_t *)t.p[4];
        s.n_regions = t.n;
        return args::entropy_stats_levels(&s);
    }
    x266_entropy_side_stats_t s = {};
    s.d_kind = (const uint8_t *)t.p[0];
    s.d_mode = (const uint8_t *)t.p[1];
    s.d_class = (const uint8_t *)t.p[2];
    s.d_qp = (const uint8_t *)t.p[3];
    s.d_nnz = (const uint32_t *)t.p[4];
    s.d_counts = (uint64_t *)t.p[5];
    s.d_part = (uint32_t *)t.p[6];
    s.n_ctu = t.n;
    s.qp = t.qp;
    s.chroma_qp_offset = t.off;
    return args::entropy_stats_side(&s);
}
// every pointer in a region of its own (2^48 bytes: 2^33 regions of levels are 2^44), at exactly its alignment times an odd number
static Tuple placed(const Call &c, size_t n)
{
    Tuple t = {};
    for (int i = 0; i < c.n_fields; ++i) t.p[i] = ((U)(i + 1) << 48) + (U)c.f[i].align * (2 * i + 1);
    t.n = n;
    t.qp = 32;
    t.off = -3;
    return t;
}

// do [x, x + n) and [y, y + m) share a byte
static bool meet(U x, size_t n, U y, size_t m) { return x < y + m && y < x + n; }

static void walk(int call, const Tuple &b, const std::string &label)
{
    const Call &c = CALLS[call];
    expect(c.name, label + "base", rule(call, b), false);
    for (int f = 0; f < c.n_fields; ++f) {
        const unsigned align = c.f[f].align;
        const std::string name = label + c.f[f].name;
        const size_t bytes = extent(c, f, b);
        Tuple t = b;
        t.p[f] = 0;
        if (call == 1 && f == 1) expect(c.name, name + " NULL with d_kind present", rule(call, t), true, args::kEntropySideModes);
        else expect(c.name, name + " NULL", rule(call, t), !c.f[f].optional, args::kNull);
        if (align > 1) {
            t = b;
            t.p[f] += align / 2;
            expect(c.name, name + " at half its alignment", rule(call, t), true, args::kMisaligned);
        }
        t = b;
        t.p[f] += align;
        expect(c.name, name + " one alignment further", rule(call, t), false);
        if (bytes > align) {
            t = b;
            t.p[f] = (U)0 - align;                                          // the last aligned address: the extent is larger and wraps
            expect(c.name, name + " running past the top of the address space", rule(call, t), true, args::kNoFit);
        }
        t = b;
        t.p[f] = down((U)0 - bytes - align, align);                         // the span ends just below the top
        expect(c.name, name + " ending just below the top", rule(call, t), false);
        t.p[f] = down((U)0 - bytes + align, align);                         // ... and just above it
        if (t.p[f]) expect(c.name, name + " ending just above the top", rule(call, t), true, args::kNoFit);
        // overlaps: field f placed onto every other buffer g of the call -- refused iff one of the two is an output
        for (int g = 0; g < c.n_fields; ++g) {
            if (g == f) continue;
            const size_t other = extent(c, g, b);
            const bool bad = c.f[f].output || c.f[g].output;
            const std::string on = name + " on " + c.f[g].name;
            t = b;
            t.p[f] = b.p[g];
            if (t.p[f] % align == 0) expect(c.name, on + ": same address", rule(call, t), bad, args::kOverlap);
            t.p[f] = down(b.p[g] + other - 1, align);                       // onto g's last byte, if rounding down leaves f long enough to reach it
            expect(c.name, on + ": its last bytes", rule(call, t), bad && meet(t.p[f], bytes, b.p[g], other), args::kOverlap);
            t.p[f] = up(b.p[g] + other, align);                             // right behind g
            expect(c.name, on + ": right behind it", rule(call, t), false);
            t.p[f] = down(b.p[g] - bytes, align);                           // ending where g begins, or before
            expect(c.name, on + ": right in front of it", rule(call, t), false);
            t.p[f] = down(b.p[g] - bytes, align) + align;                   // f's last bytes reach into g ...
            if (t.p[f] + bytes > b.p[g]) expect(c.name, on + ": its last bytes reach in", rule(call, t), bad && meet(t.p[f], bytes, b.p[g], other), args::kOverlap);
        }
    }
}

static void scalars_and_counts(int call, const Tuple &b)
{
    const Call &c = CALLS[call];
    Tuple t = b;
    if (call == 1) {
        range(c.name, "qp", 0, 51, [&](int v) {
            Tuple u = b;
            u.qp = v;
            return rule(call, u);
        }, args::kEntropySideScalars);
        range(c.name, "chroma_qp_offset", -12, 12, [&](int v) {
            Tuple u = b;
            u.off = v;
            return rule(call, u);
        }, args::kEntropySideScalars);
        for (int v : {INT_MIN, INT_MAX}) {
            t = b;
            t.qp = v;
            expect(c.name, "qp " + std::to_string(v), rule(call, t), true, args::kEntropySideScalars);
            t = b;
            t.off = v;
            expect(c.name, "chroma_qp_offset " + std::to_string(v), rule(call, t), true, args::kEntropySideScalars);
        }
        t = b;                                                              // kinds need modes; modes alone are fine
        t.p[1] = 0;
        expect(c.name, "d_mode NULL with d_kind present", rule(call, t), true, args::kEntropySideModes);
        t.p[0] = 0;
        expect(c.name, "d_mode and d_kind NULL", rule(call, t), false);
        t = b;
        t.p[0] = 0;
        expect(c.name, "d_kind NULL with d_mode present", rule(call, t), false);
    }
    t = b;                                                                  // every optional array NULL
    for (int f = 0; f < c.n_fields; ++f)
        if (c.f[f].optional) t.p[f] = 0;
    expect(c.name, "every optional array NULL", rule(call, t), false);
    t = b;
    t.n = SIZE_MAX / 4;                                                     // the inputs' spans saturate
    expect(c.name, "n 2^62 - 1", rule(call, t), true, args::kNoFit);
    t = b;                                                                  // the rows of d_part: one more unit than a row holds is one more row
    for (size_t n : {c.per_row, c.per_row + 1, 2 * c.per_row, 2 * c.per_row + 1}) {
        t.n = n;
        const size_t rows = rows_of(n, c.per_row), row_bytes = 8 * c.contexts;
        t.p[c.part] = down((U)0 - rows * row_bytes - 16, 16);
        expect(c.name, "d_part of " + std::to_string(rows) + " rows just below the top", rule(call, t), false);
        t.p[c.part] = down((U)0 - rows * row_bytes + 16, 16);
        expect(c.name, "d_part of " + std::to_string(rows) + " rows reaching over the top", rule(call, t), true, args::kNoFit);
        t.p[c.part] = b.p[c.part];
        t.p[c.counts] = up(b.p[c.part] + rows * row_bytes, 8);
        expect(c.name, "d_counts right behind " + std::to_string(rows) + " rows", rule(call, t), false);
        t.p[c.counts] = up(b.p[c.part] + rows * row_bytes, 8) - 8;
        expect(c.name, "d_counts on the last bytes of " + std::to_string(rows) + " rows", rule(call, t), true, args::kOverlap);
        t.p[c.counts] = b.p[c.counts];
    }
    t = b;                                                                  // no unit: only d_counts (and the side call's scalars)
    t.n = 0;
    for (int f = 0; f < c.n_fields; ++f)
        if (f != c.counts) t.p[f] = 0;
    expect(c.name, "n 0 with every other buffer NULL", rule(call, t), false);
    for (int f = 0; f < c.n_fields; ++f)
        if (f != c.counts) t.p[f] = 3;
    expect(c.name, "n 0 with every other buffer misaligned", rule(call, t), false);
    for (int f = 0; f < c.n_fields; ++f)
        if (f != c.counts) t.p[f] = b.p[c.counts];
    expect(c.name, "n 0 with every other buffer on d_counts", rule(call, t), false);
    t.p[c.counts] = 0;
    expect(c.name, "n 0 without d_counts", rule(call, t), true, args::kNull);
    t.p[c.counts] = b.p[c.counts] + 4;
    expect(c.name, "n 0 with d_counts at half its alignment", rule(call, t), true, args::kMisaligned);
    t.p[c.counts] = (U)0 - 8;
    expect(c.name, "n 0 with d_counts over the top", rule(call, t), true, args::kNoFit);
    if (call == 1) {
        t = b;
        t.n = 0;
        t.qp = 52;
        expect(c.name, "n 0 with qp 52", rule(call, t), true, args::kEntropySideScalars);
    }
}

// ---- the table rule and the counting sink --------------------------------------------------------------------------------------------------------
static void truth(const std::string &what, bool ok) { expect(SHARED, what, ok ? nullptr : "differs from the literal", false); }

static void shared_code()
{
    truth("rows", args::entropy_stats_rows(0, 32) == 0 && args::entropy_stats_rows(1, 32) == 1 && args::entropy_stats_rows(32, 32) == 1 &&
                      args::entropy_stats_rows(33, 32) == 2 && args::entropy_stats_rows(12240, 32) == 383 && args::entropy_stats_rows(2040, 64) == 32 &&
                      args::entropy_stats_rows(5, 0) == 0 && args::entropy_stats_rows(SIZE_MAX, 32) == SIZE_MAX / 32 + 1);
    const uint64_t big = (uint64_t)1 << 40, top = ((uint64_t)1 << 51) - 1;
    truth("the table rule", entropy_init_from_counts(0, 0) == 1024 && entropy_init_from_counts(1, 0) == 2017 && entropy_init_from_counts(0, 1) == 31 &&
                                entropy_init_from_counts(1, 1) == 1024 && entropy_init_from_counts(1, 4095) == 31 && entropy_init_from_counts(3, 1) == 1536 &&
                                entropy_init_from_counts(1, 3) == 512 && entropy_init_from_counts(2, 1) == 1365 && entropy_init_from_counts(1, 2) == 683);
    truth("the table rule at 2^40 and below 2^51", entropy_init_from_counts(big, big) == 1024 && entropy_init_from_counts(3 * big, big) == 1536 &&
                                                      entropy_init_from_counts(big, 0) == 2017 && entropy_init_from_counts(top, top) == 1024 &&
                                                      entropy_init_from_counts(top, 1) == 2017 && entropy_init_from_counts(1, top) == 31);
    // the level walk under the counting sink: the header's three worked regions, whose context bins are 4, 5 and 114
    {
        struct {
            unsigned at;
            int16_t v;
            uint64_t bins;
        } worked[3] = {{0, 1, 4}, {0, -32768, 5}, {1023, 3, 114}};
        for (auto &w : worked) {
            std::vector<int16_t> level(1024, 0);
            level[w.at] = w.v;
            uint64_t counts[2 * kEntropyCtxPerSize] = {};
            uint16_t ctx[kEntropyCtxPerSize] = {};
            EntropyCounter<uint64_t, 1> e = {counts, ctx};
            entropy_encode_region(e, level.data(), 3, entropy_cg_mask(level.data(), 3), ctx);
            uint64_t sum = 0;
            for (uint64_t v : counts) sum += v;
            bool untouched = true;
            for (uint16_t v : ctx) untouched = untouched && v == 0;
            truth("a worked region's context bins, counted", sum == w.bins && counts[2 * kCtxCbf + 1] == 1 && untouched);
            if (w.at == 0) truth("DC alone: last x and y are one zero bin each, no sig bin", counts[2 * kCtxLastX] == 1 && counts[2 * kCtxLastY] == 1 && counts[2 * kCtxSig] == 0);
        }
        for (unsigned k = 0; k < 4; ++k) {                                  // an uncoded region: one zero cbf bin per block, nothing read
            uint64_t counts[2 * kEntropyCtxPerSize] = {};
            uint16_t ctx[kEntropyCtxPerSize] = {};
            EntropyCounter<uint64_t, 1> e = {counts, ctx};
            entropy_encode_region(e, (const int16_t *)nullptr, k, 0ull, ctx);
            uint64_t sum = 0;
            for (uint64_t v : counts) sum += v;
            truth("an uncoded region of size " + std::to_string(k), counts[0] == (64u >> (2 * k)) && sum == counts[0]);
        }
    }
    // the side walk under the counting sink, through a pitch as the kernel's: the flat CTU is 11 zero bins, the worst CTU 64 bins
    {
        const EntropySideCtu flat = entropy_side_flat_ctu(27, -12);
        uint32_t counts[2 * kEntropySideContexts * 4] = {};
        uint16_t ctx[kEntropySideContexts] = {};
        EntropyCounter<uint32_t, 4> e = {counts + 1, ctx};
        entropy_side_encode_ctu(e, flat, ctx, 1u, 27, -12);
        uint64_t zeros = 0, ones = 0, elsewhere = 0;
        for (unsigned i = 0; i < 2 * kEntropySideContexts * 4; ++i) (i % 4 != 1 ? elsewhere : (i / 4) % 2 ? ones : zeros) += counts[i];
        truth("the flat CTU, counted through a pitch", zeros == 11 && ones == 0 && elsewhere == 0 && counts[4 * 2 * kSideCtxKind + 1] == 4 &&
                                                           counts[4 * 2 * (kSideCtxKind + 1) + 1] == 1 && counts[4 * 2 * kSideCtxCoded + 1] == 4 &&
                                                           counts[4 * 2 * (kSideCtxCoded + 1) + 1] == 2);
        const uint8_t kind[6] = {1, 1, 1, 1, 1, 1}, mode[6] = {34, 33, 32, 31, 33, 33}, cls[6] = {12, 12, 12, 12, 12, 12}, qp_in[6] = {51, 0, 51, 0, 51, 0};
        const EntropySideCtu worst = entropy_side_canon(kind, mode, cls, qp_in, nullptr, 0, 0);
        uint64_t all[2 * kEntropySideContexts] = {};
        EntropyCounter<uint64_t, 1> w = {all, ctx};
        entropy_side_encode_ctu(w, worst, ctx, 1u, 0, 0);
        uint64_t sum = 0;
        for (uint64_t v : all) sum += v;
        truth("the worst CTU, counted", sum == 64);
    }
}

int main()
{
    for (int call = 0; call < 2; ++call) {
        const Call &c = CALLS[call];
        std::printf("%s:", c.name);
        for (int f = 0; f < c.n_fields; ++f) std::printf("%s %s %u %s%s", f ? "," : "", c.f[f].name, c.f[f].align, c.f[f].optional ? "opt " : "", c.f[f].output ? "out" : "in");
        std::printf("\n");
    }
    static_assert(offsetof(x266_entropy_stats_t, d_counts) == 24 && offsetof(x266_entropy_stats_t, d_part) == 32 && offsetof(x266_entropy_stats_t, n_regions) == 40 &&
                      sizeof(x266_entropy_stats_t) == 48,
                  "the struct of the header");
    static_assert(offsetof(x266_entropy_side_stats_t, d_nnz) == 32 && offsetof(x266_entropy_side_stats_t, d_counts) == 40 && offsetof(x266_entropy_side_stats_t, d_part) == 48 &&
                      offsetof(x266_entropy_side_stats_t, n_ctu) == 56 && offsetof(x266_entropy_side_stats_t, qp) == 64 &&
                      offsetof(x266_entropy_side_stats_t, chroma_qp_offset) == 68 && sizeof(x266_entropy_side_stats_t) == 72,
                  "the struct of the header");
    static_assert(X266_ENTROPY_STATS_REGIONS == 32 && X266_ENTROPY_SIDE_STATS_CTUS == 64, "the header's constants");
    // a row cannot pass 32 bits: 3456 context bins a region, 64 a CTU
    static_assert((uint64_t)X266_ENTROPY_STATS_REGIONS * 3456 < ((uint64_t)1 << 32) && (uint64_t)X266_ENTROPY_SIDE_STATS_CTUS * 64 < ((uint64_t)1 << 32), "the rows' counters");
    std::printf("sizeof(x266_entropy_stats_t) %zu\nsizeof(x266_entropy_side_stats_t) %zu\n", sizeof(x266_entropy_stats_t), sizeof(x266_entropy_side_stats_t));
    for (int call = 0; call < 2; ++call) {
        ++g_checks;
        if (!(call == 0 ? args::entropy_stats_levels(nullptr) : args::entropy_stats_side(nullptr))) ++g_failures, std::printf("FAIL a NULL parameter struct is accepted\n");
        for (size_t n : {(size_t)1, (size_t)33, (size_t)65, (size_t)12240, (size_t)1 << 33}) {
            const Tuple b = placed(CALLS[call], n);
            walk(call, b, "n " + std::to_string(n) + " ");
            if (n == 65) scalars_and_counts(call, b);
        }
    }
    shared_code();
    std::printf("checks entropy statistics %d\n", g_checks);
    if (g_failures) {
        std::printf("%d of %d checks FAILED\n", g_failures, g_checks);
        return 1;
    }
    std::printf("the argument rules hold (%d checks)\n", g_checks);
    return 0;
}
