// CPU check of the argument rules of xQualityStatsGpu (x266_amd/csrc/x266_args.hpp: quality_stats), the call whose device pointers are the
// fields of the host-read x266_quality_t, and of the host call xQualityFromTotals (quality_from_totals).  The contract is written down once
// more by hand from include/x266hip.h -- the pointer fields in struct order with their alignments, which are written and which may be NULL,
// their extents -- and one walk perturbs a base tuple one field at a time, with and without d_total: NULL, half an alignment, one alignment
// further, the top of the address space, every overlap of an output with any other buffer, the frame sizes and the flags.  The addresses
// are made-up integers, nothing is dereferenced, no device is needed; the expected verdict of every check follows from these tables and
// from literals, never from the function under test.
// Test infrastructure; built and run by tests/test_quality_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <climits>
#include <string>

#include "rules_expect.hpp"
#include "x266_args.hpp"

using namespace x266;

static const char *CALL = "xQualityStatsGpu";
static const char *HOST = "xQualityFromTotals";
enum { SRC, DEC, CTU, TOTAL, N_FIELDS };
struct Field {
    const char *name;
    unsigned align;
    bool optional, output;
};
static const Field FIELDS[N_FIELDS] = {{"d_src", 16, false, false}, {"d_dec", 16, false, false}, {"d_ctu", 16, false, true}, {"d_total", 8, true, true}};
struct Tuple {
    U p[N_FIELDS];
    int w, h, flags;
};

static size_t extent(int f, const Tuple &t)
{
    if (f == TOTAL) return 64;
    if (f == CTU) return 48 * (((size_t)t.w + 63) / 64) * (((size_t)t.h + 63) / 64);
    return (size_t)t.w * (size_t)t.h * 2;
}
static const char *rule(const Tuple &t)
{
    x266_quality_t s = {};
    s.d_src = (const x266_ref_block_t *)t.p[SRC];
    s.d_dec = (const x266_ref_block_t *)t.p[DEC];
    s.d_ctu = (x266_quality_ctu_t *)t.p[CTU];
    s.d_total = (int64_t *)t.p[TOTAL];
    s.width = t.w;
    s.height = t.h;
    s.flags = t.flags;
    return args::quality_stats(&s);
}
// every pointer in a region of its own, at exactly its alignment times an odd number
static Tuple placed(int w, int h)
{
    Tuple t = {};
    for (int i = 0; i < N_FIELDS; ++i) t.p[i] = ((U)(i + 1) << 44) + (U)FIELDS[i].align * (2 * i + 1);
    t.w = w;
    t.h = h;
    t.flags = X266_QUALITY_SSE | X266_QUALITY_SSIM;
    return t;
}

static void walk(const Tuple &base, bool with_total, const std::string &label)
{
    Tuple b = base;
    if (!with_total) b.p[TOTAL] = 0;
    const std::string at = label + (with_total ? "with d_total: " : "without d_total: ");
    expect(CALL, at + "base", rule(b), false);
    for (int f = 0; f < N_FIELDS; ++f) {
        if (!b.p[f]) continue;
        const unsigned align = FIELDS[f].align;
        const std::string name = at + FIELDS[f].name;
        Tuple t = b;
        t.p[f] = 0;
        expect(CALL, name + " NULL", rule(t), !FIELDS[f].optional, args::kNull);
        t = b;
        t.p[f] += align / 2;
        expect(CALL, name + " at half its alignment", rule(t), true, args::kMisaligned);
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

static void sizes_and_flags(const Tuple &b)
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
    for (auto wh : {std::pair<int, int>{16, 16}, {48, 80}, {64, 64}, {144, 80}, {1920, 1088}, {3840, 2176}, {7680, 4320}}) {
        Tuple t = placed(wh.first, wh.second);
        t.p[TOTAL] = b.p[TOTAL];
        expect(CALL, "frame " + std::to_string(wh.first) + "x" + std::to_string(wh.second), rule(t), false);
    }
    {   // the largest frame an int describes: the extents are exact (no product wraps 64 bits), and the frames no longer fit beside each other
        Tuple t = placed(INT_MAX - 15, INT_MAX - 15);
        t.p[TOTAL] = b.p[TOTAL];
        expect(CALL, "the largest frame", rule(t), true, args::kOverlap);
        t.p[DEC] = t.p[SRC];                                                // one frame as both inputs: the records still lie inside it
        expect(CALL, "the largest frame against itself", rule(t), true, args::kOverlap);
        t.p[CTU] = (U)0 - 16 * 4096;                                        // 48 n_ctu bytes do not fit behind it
        expect(CALL, "the largest frame, d_ctu near the top", rule(t), true, args::kNoFit);
    }
    for (int flags : {X266_QUALITY_SSE, X266_QUALITY_SSIM, X266_QUALITY_SSE | X266_QUALITY_SSIM}) {
        Tuple t = b;
        t.flags = flags;
        expect(CALL, "flags " + std::to_string(flags), rule(t), false);
    }
    for (int flags : {0, 4, 5, 7, 8, 0x103, -1, INT_MIN, INT_MAX}) {
        Tuple t = b;
        t.flags = flags;
        expect(CALL, "flags " + std::to_string(flags), rule(t), true, args::kQualityFlags);
    }
}

// xQualityFromTotals: NULL pointers, sides, negative squared errors, window counts that are not the frame's (0: a run without SSIM)
static void from_totals()
{
    const int w = 144, h = 80;
    const int64_t win_y = 35 * 19, win_c = 17 * 9;
    const int64_t good[8] = {5, 6, 7, (int64_t)1 << 30, (int64_t)2 << 30, -((int64_t)3 << 30), win_y, win_c};
    double psnr[4] = {}, ssim[3] = {};
    auto with = [&](int i, int64_t v) {
        int64_t t[8];
        for (int k = 0; k < 8; ++k) t[k] = good[k];
        t[i] = v;
        return args::quality_from_totals(t, w, h, psnr, ssim);
    };
    expect(HOST, "base", args::quality_from_totals(good, w, h, psnr, ssim), false);
    expect(HOST, "total NULL", args::quality_from_totals(nullptr, w, h, psnr, ssim), true, args::kNull);
    expect(HOST, "psnr NULL", args::quality_from_totals(good, w, h, nullptr, ssim), true, args::kNull);
    expect(HOST, "ssim NULL", args::quality_from_totals(good, w, h, psnr, nullptr), true, args::kNull);
    for (int bad : {0, -16, 8, 152, INT_MIN, INT_MAX}) {
        expect(HOST, "width " + std::to_string(bad), args::quality_from_totals(good, bad, h, psnr, ssim), true);
        expect(HOST, "height " + std::to_string(bad), args::quality_from_totals(good, w, bad, psnr, ssim), true);
    }
    for (int i = 0; i < 3; ++i) {
        expect(HOST, "sse " + std::to_string(i) + " negative", with(i, -1), true);
        expect(HOST, "sse " + std::to_string(i) + " zero", with(i, 0), false);
        expect(HOST, "sse " + std::to_string(i) + " at its largest", with(i, INT64_MAX), false);
        expect(HOST, "ssim " + std::to_string(i) + " negative", with(3 + i, -((int64_t)1 << 40)), false);    // a sum of signed values
    }
    expect(HOST, "win_y zero", with(6, 0), false);
    expect(HOST, "win_c zero", with(7, 0), false);
    for (int64_t d : {(int64_t)-1, (int64_t)1}) {
        expect(HOST, "win_y off by one", with(6, win_y + d), true);
        expect(HOST, "win_c off by one", with(7, win_c + d), true);
    }
    expect(HOST, "win_y negative", with(6, -win_y), true);
    expect(HOST, "win_y the chroma count", with(6, win_c), true);
    expect(HOST, "the counts of another frame", args::quality_from_totals(good, 160, 80, psnr, ssim), true);
    {   // the largest frame: its counts do not wrap
        const int64_t big = INT_MAX - 15, y = (big / 4 - 1) * (big / 4 - 1), c = (big / 8 - 1) * (big / 8 - 1);
        const int64_t t[8] = {0, 0, 0, 0, 0, 0, y, c};
        expect(HOST, "the largest frame", args::quality_from_totals(t, (int)big, (int)big, psnr, ssim), false);
    }
}

int main()
{
    std::printf("%s:", CALL);
    for (int f = 0; f < N_FIELDS; ++f)
        std::printf("%s %s %u %s%s", f ? "," : "", FIELDS[f].name, FIELDS[f].align, FIELDS[f].optional ? "opt " : "", FIELDS[f].output ? "out" : "in");
    std::printf("\n");
    ++g_checks;
    if (!args::quality_stats(nullptr)) ++g_failures, std::printf("FAIL a NULL parameter struct is accepted\n");
    for (auto wh : {std::pair<int, int>{16, 16}, {144, 80}, {64, 64}, {1920, 1088}}) {
        const Tuple b = placed(wh.first, wh.second);
        const std::string label = std::to_string(wh.first) + "x" + std::to_string(wh.second) + " ";
        for (bool with_total : {true, false}) {
            walk(b, with_total, label);
            Tuple t = b;
            if (!with_total) t.p[TOTAL] = 0;
            sizes_and_flags(t);
            t.p[DEC] = t.p[SRC];                                            // the two inputs may be the same frame
            expect(CALL, label + "d_dec == d_src", rule(t), false);
            t.p[DEC] = t.p[SRC] + 512;                                      // ... or overlap in any other way
            expect(CALL, label + "d_dec a tile into d_src", rule(t), false);
        }
    }
    from_totals();
    std::printf("checks x266_quality_t %d\n", g_checks);
    if (g_failures) {
        std::printf("%d of %d checks FAILED\n", g_failures, g_checks);
        return 1;
    }
    std::printf("the argument rules hold (%d checks)\n", g_checks);
    return 0;
}
