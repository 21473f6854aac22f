// CPU check of the argument rules of the calls that take their device pointers in a host-read struct (x266_amd/csrc/x266_args.hpp:
// levels_pack, levels_unpack, aq_stats, aq_decide, the five la_*, seeded_search, mixed_code_frame, rdoq_regions, levels_bits) and of the
// two host-pointer calls beside them (weights_from_totals, scene_cut_from_totals).  tests/cpp/arg_rules_check.cpp holds the calls with
// flat arguments; this driver holds these, one family per struct.  The rules are integer arithmetic on addresses and sizes: the addresses
// are made-up integers, nothing is dereferenced, no device is needed.
//
// A Family is the contract written down once more by hand from include/x266hip.h: the struct's pointer fields in struct order with their
// alignments, per call each field's flags (not looked at / read / written, may be NULL) and the one input an output may exactly be, the
// fields' extents, the struct from a tuple, and the base tuple(s).  One walk perturbs a base tuple one field at a time, with and without
// the optional buffers, for every call of every family; one helper walks the frame sizes and one the scalar ranges, from per-family
// lists; the rules that are a family's own follow its description.  The expected verdict of every check follows from these tables and
// from literals, never from the functions under test.  A new struct call adds a row to its family, a new struct a family.
// Test infrastructure; built and run by tests/test_struct_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <climits>
#include <string>
#include <utility>
#include <vector>

#include "rules_expect.hpp"
#include "x266_args.hpp"

using namespace x266;

enum { IN = 0, OPT = 1, OUT = 2, UNUSED = 4 };
enum { MAX_FIELDS = 14 };
struct Tuple {
    U p[MAX_FIELDS];
    size_t n;                       // count families: regions
    uint64_t cap;
    int w, h;                       // frame families
    int s[4];                       // the family's scalars, in struct order
};
struct Field {
    const char *name;
    unsigned align;
};
struct Call {
    const char *name;
    const char *(*rule)(const Tuple *);             // nullptr: the call with p == NULL
    std::vector<int> flags;                         // per field
    int high = 0;                                   // the largest frame: with this field ...
    U high_at = 0;                                  // ... up here, its span does not fit
    std::vector<std::pair<int, int>> may_be = {};   // an output and the one input it may be (the very same address)
    unsigned one_of = 0;                            // a bit per field: not all of these may be NULL ...
    const char *one_of_why = nullptr;               // ... or the call is refused for this
};
struct Scalar {
    const char *name;
    int at;                         // index into Tuple::s
    int lo, hi;
    unsigned calls;                 // a bit per call that reads it; the others accept any value
    const char *why;
    int without;                    // this pointer NULL while the scalar is walked, or -1
};
struct Family {
    const char *name;
    std::vector<Field> fields;
    std::vector<Call> calls;
    size_t (*extent)(int f, const Tuple &);
    std::vector<Tuple> bases;
    int granule;                    // 0: a count family
    std::vector<int> bad;           // sides that are refused
    std::vector<std::pair<int, int>> good;
    std::vector<Scalar> scalars;
    void (*own)(const Family &, int c, const Tuple &b);    // the family's own rules, per call and base
    void (*once)();                 // ... and what it holds beside its struct calls
};

template <class S, S (*Make)(const Tuple &), const char *(*Rule)(const S *)> static const char *apply(const Tuple *t)
{
    if (!t) return Rule(nullptr);
    const S s = Make(*t);
    return Rule(&s);
}
// every pointer in a region of its own, at exactly its alignment times an odd number
static Tuple placed(const std::vector<Field> &fields)
{
    Tuple t = {};
    for (size_t i = 0; i < fields.size(); ++i) t.p[i] = ((U)(i + 1) << 44) + (U)fields[i].align * (2 * i + 1);
    return t;
}
static const char *size_reason(int granule)
{
    return granule == 16 ? "width/height must be positive multiples of 16" : granule == 32 ? "width/height must be positive multiples of 32"
                                                                                            : "width/height must be positive multiples of 64";
}
static bool pair(const Call &c, int f, int g)
{
    for (const auto &m : c.may_be)
        if ((m.first == f && m.second == g) || (m.first == g && m.second == f)) return true;
    return false;
}

// ---- the one walk ------------------------------------------------------------------------------------------------------------------
// `without`: a bit per optional field that is NULL in this walk's base
static void walk(const Family &F, const Call &c, const Tuple &base, unsigned without, const std::string &label)
{
    const int n = (int)F.fields.size();
    const char *call = c.name;
    auto used = [&](int f) { return !(c.flags[f] & UNUSED); };
    auto out = [&](int f) { return (c.flags[f] & OUT) != 0; };
    Tuple b = base;
    std::string at = label + "without";
    for (int f = 0; f < n; ++f)
        if ((without >> f) & 1u) {
            b.p[f] = 0;
            at += std::string(" ") + F.fields[f].name;
        }
    at += ": ";
    expect(call, at + "base", c.rule(&b), false);
    for (int f = 0; f < n; ++f) {
        if (!b.p[f]) continue;
        const unsigned align = F.fields[f].align;
        const std::string name = at + F.fields[f].name;
        bool last = (c.one_of >> f) & 1u;                                       // the last one given of a group that needs one
        for (int g = 0; g < n; ++g)
            if (g != f && ((c.one_of >> g) & 1u) && b.p[g]) last = false;
        Tuple t = b;
        t.p[f] = 0;
        if (used(f) && !(c.flags[f] & OPT)) expect(call, name + " NULL", c.rule(&t), true, args::kNull);
        else expect(call, name + " NULL", c.rule(&t), last, c.one_of_why);
        if (align > 1) {
            t = b;
            t.p[f] += align / 2;
            expect(call, name + " at half its alignment", c.rule(&t), used(f), args::kMisaligned);
        }
        t = b;
        t.p[f] += align;                                                        // aligned to exactly that, and to twice it (or odd): both fine
        expect(call, name + " one alignment further", c.rule(&t), false);
        // the span's end against the end of the address space
        const size_t bytes = F.extent(f, b);
        if (bytes <= align) ++g_failures, std::printf("FAIL the driver's own extent of %s\n", name.c_str());
        t = b;
        t.p[f] = (U)0 - align;                                                  // the last aligned address: every extent here is larger and wraps
        expect(call, name + " running past the top of the address space", c.rule(&t), used(f), args::kNoFit);
        t = b;
        t.p[f] = down((U)0 - 2 * bytes, align);                                 // high up, with room to spare
        expect(call, name + " near the top of the address space", c.rule(&t), false);
        t.p[f] = down((U)0 - bytes - align, align);                             // the span ends just below the top
        expect(call, name + " ending just below the top", c.rule(&t), false);
        t.p[f] += 2 * align;
        expect(call, name + " two alignments further", c.rule(&t), used(f), args::kNoFit);
        // overlap: field g moved onto the first byte, onto the last byte and right behind field f; refused when the call looks at both and
        // either is an output -- except the very same address of an output and the one input it may be
        for (int g = 0; g < n; ++g) {
            if (g == f || !b.p[g]) continue;
            const unsigned ga = F.fields[g].align;
            const bool clash = used(f) && used(g) && (out(f) || out(g));
            const std::string gname = F.fields[g].name;
            t = b;
            t.p[g] = down(t.p[f], ga);                                          // g starts at or just before f's first byte, and is longer than that step
            if (F.extent(g, b) <= t.p[f] - t.p[g]) ++g_failures, std::printf("FAIL the driver's own overlap case %s / %s\n", gname.c_str(), name.c_str());
            expect(call, gname + " over the start of " + name, c.rule(&t), clash && !(pair(c, f, g) && t.p[g] == t.p[f]), args::kOverlap);
            t = b;
            t.p[g] = down(t.p[f] + bytes - 1, ga);                              // g's first byte among f's last
            expect(call, gname + " over the end of " + name, c.rule(&t), clash && !(pair(c, f, g) && t.p[g] == t.p[f]), args::kOverlap);
            t = b;
            t.p[g] = down(t.p[f] + bytes + ga - 1, ga);                         // right behind f
            expect(call, gname + " right behind " + name, c.rule(&t), false);
            if (pair(c, f, g)) {                                                // one step off the allowed address is an overlap like any other
                t = b;
                t.p[g] = t.p[f] + ga;
                expect(call, gname + " one alignment into " + name, c.rule(&t), true, args::kOverlap);
            }
        }
    }
}
// the very same address twice, for every pair of fields, at an address of its own and at the first one's: accepted for two inputs, for
// a field the call does not look at, and for the pairs of the header
static void same_address(const Family &F, const Call &c, const Tuple &b, const std::string &label)
{
    const int n = (int)F.fields.size();
    for (int f = 0; f < n; ++f)
        for (int g = 0; g < n; ++g) {
            if (g == f) continue;
            const bool both = !(c.flags[f] & UNUSED) && !(c.flags[g] & UNUSED), any_out = ((c.flags[f] | c.flags[g]) & OUT) != 0;
            const std::string what = label + F.fields[g].name + " == " + F.fields[f].name;
            Tuple t = b;
            t.p[g] = t.p[f] = ((U)1 << 50) + 4096;                              // aligned for every field
            expect(c.name, what, c.rule(&t), both && any_out && !pair(c, f, g), args::kOverlap);
            if (b.p[f] % F.fields[g].align) continue;
            t = b;
            t.p[g] = t.p[f];
            expect(c.name, what + ", where it is", c.rule(&t), both && any_out && !pair(c, f, g), args::kOverlap);
        }
}
static void frame_sizes(const Family &F, const Call &c, const Tuple &b, const std::string &label)
{
    for (int v : F.bad) {
        Tuple t = b;
        t.w = v;
        expect(c.name, label + "width " + std::to_string(v), c.rule(&t), true, size_reason(F.granule));
        t = b;
        t.h = v;
        expect(c.name, label + "height " + std::to_string(v), c.rule(&t), true, size_reason(F.granule));
    }
    for (const auto &g : F.good) {
        Tuple t = b;
        t.w = g.first;
        t.h = g.second;
        expect(c.name, label + "frame " + std::to_string(g.first) + "x" + std::to_string(g.second), c.rule(&t), false);
    }
    // the largest frame an int describes: its spans fit behind addresses of 2^44 and cover every buffer above them; high up they do not fit
    const int side = INT_MAX - INT_MAX % F.granule;
    Tuple t = b;
    t.w = t.h = side;
    expect(c.name, label + "the largest frame", c.rule(&t), true, args::kOverlap);
    t.p[c.high] = c.high_at;
    expect(c.name, label + "the largest frame, high up", c.rule(&t), true, args::kNoFit);
}
// the call that reads a scalar holds it to its range, the others read none of them
static void scalar_ranges(const Family &F, int ci, const Tuple &b, const std::string &label)
{
    const Call &c = F.calls[ci];
    for (const Scalar &s : F.scalars) {
        const int values[] = {s.lo, s.hi, s.lo + 1, s.hi - 1, s.lo - 1, s.hi + 1, INT_MIN, INT_MAX};
        for (int v : values) {
            Tuple t = b;
            if (s.without >= 0) t.p[s.without] = 0;
            t.s[s.at] = v;
            expect(c.name, label + s.name + " " + std::to_string(v), c.rule(&t), ((s.calls >> ci) & 1u) && (v < s.lo || v > s.hi), s.why);
        }
    }
}

static void run(const Family &F)
{
    const int n = (int)F.fields.size();
    for (size_t ci = 0; ci < F.calls.size(); ++ci) {
        const Call &c = F.calls[ci];
        expect(c.name, "NULL p", c.rule(nullptr), true, "NULL parameter struct");
        // the bases: everything given, each optional field alone NULL, all of them NULL (but one of a group that needs one)
        unsigned all = 0;
        std::vector<unsigned> masks = {0u};
        auto add = [&](unsigned m) {
            for (unsigned d : masks)
                if (d == m) return;
            masks.push_back(m);
        };
        for (int f = 0; f < n; ++f)
            if (!(c.flags[f] & UNUSED) && (c.flags[f] & OPT)) all |= 1u << f, add(1u << f);
        if (!c.one_of) add(all);
        for (int f = 0; f < n; ++f)
            if ((c.one_of >> f) & 1u) add(all & ~(1u << f));
        for (size_t bi = 0; bi < F.bases.size(); ++bi) {
            const std::string label = F.bases.size() > 1 ? "base " + std::to_string(bi) + ": " : "";
            for (unsigned m : masks) walk(F, c, F.bases[bi], m, label);
            same_address(F, c, F.bases[bi], label);
            if (F.granule) frame_sizes(F, c, F.bases[bi], label);
            scalar_ranges(F, (int)ci, F.bases[bi], label);
            if (F.own) F.own(F, (int)ci, F.bases[bi]);
        }
        std::printf("%s:", c.name);
        const char *sep = " ";
        for (int f = 0; f < n; ++f) {
            if (c.flags[f] & UNUSED) continue;
            std::printf("%s%s %u %s%s", sep, F.fields[f].name, F.fields[f].align, (c.flags[f] & OPT) ? "opt " : "", (c.flags[f] & OUT) ? "out" : "in");
            sep = ", ";
        }
        std::printf("\n");
    }
    if (F.once) F.once();
}

// ---- the compact level stream: xLevelsPackGpu, xLevelsUnpackGpu ----------------------------------------------------------------------
namespace levels {
enum { LEVEL, CLASS, NNZ, REGION, STREAM, TOTAL };
enum { PACK, UNPACK };
static size_t extent(int f, const Tuple &t)
{
    switch (f) {
    case LEVEL: return t.n * 2048;
    case CLASS: return t.n;
    case NNZ: return t.n * 4;
    case REGION: return t.n * 32;
    case STREAM: return (size_t)t.cap * 2;
    default: return 16;
    }
}
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
static void own(const Family &F, int c, const Tuple &b)
{
    const char *call = F.calls[c].name;
    auto rule = F.calls[c].rule;
    const bool unpack = c == UNPACK;
    // n_regions == 0: pack looks at d_total alone, unpack at nothing
    {
        Tuple t = b;
        t.n = 0;
        for (int f = 0; f < TOTAL; ++f) t.p[f] = f % 2 ? 0 : 3;                 // NULL or misaligned: not looked at
        expect(call, "no regions, the other pointers NULL or odd", rule(&t), false);
        t.p[TOTAL] = 0;
        expect(call, "no regions, d_total NULL", rule(&t), !unpack, args::kNull);
        t.p[TOTAL] = b.p[TOTAL] + 4;
        expect(call, "no regions, d_total misaligned", rule(&t), !unpack, args::kMisaligned);
    }
    // cap_words == 0: d_stream may be NULL (pack: the count-only call), and is still held to its alignment when given
    {
        Tuple t = b;
        t.cap = 0;
        expect(call, "no capacity", rule(&t), false);
        t.p[STREAM] = 0;
        expect(call, "no capacity, d_stream NULL", rule(&t), false);
        t.p[STREAM] = b.p[STREAM] + 8;
        expect(call, "no capacity, d_stream misaligned", rule(&t), true, args::kMisaligned);
        t = b;
        t.cap = 1;
        t.p[STREAM] = 0;
        expect(call, "one word of capacity, d_stream NULL", rule(&t), true, args::kNull);
    }
    // extents that saturate: no pointer has room for them
    {
        Tuple t = b;
        t.n = SIZE_MAX / 2048 + 1;                                              // n * 2048 wraps size_t
        expect(call, "n_regions * 2048 wraps", rule(&t), true, args::kNoFit);
        t.n = SIZE_MAX / 32 + 1;                                                // n * 32 wraps too
        expect(call, "n_regions * 32 wraps", rule(&t), true, args::kNoFit);
        t.n = ((size_t)1 << 52);                                                // 2^63 bytes of levels behind an address of 2^44: fits, and covers everything above it
        expect(call, "2^52 regions", rule(&t), true, args::kOverlap);
        t = b;
        t.cap = UINT64_MAX;
        expect(call, "cap_words * 2 wraps", rule(&t), true, args::kNoFit);
        t.cap = (uint64_t)1 << 63;
        expect(call, "cap_words = 2^63", rule(&t), true, args::kNoFit);
    }
}
static Family family()
{
    Family F = {};
    F.name = "x266_levels_t";
    F.fields = {{"d_level", 16}, {"d_class", 1}, {"d_nnz", 4}, {"d_region", 8}, {"d_stream", 16}, {"d_total", 8}};
    F.calls = {{"xLevelsPackGpu", apply<x266_levels_t, make, args::levels_pack>, {IN, OPT, OPT, OUT, OUT, OUT}},
               {"xLevelsUnpackGpu", apply<x266_levels_t, make, args::levels_unpack>, {OUT, OPT, OPT | OUT, IN, IN, UNUSED}}};
    F.extent = extent;
    Tuple b = placed(F.fields);
    b.n = 7;
    b.cap = 5000;
    F.bases = {b};
    F.own = own;
    return F;
}
}  // namespace levels

// ---- RDOQ and the level rate estimate: xRdoQuantRegionsGpu, xLevelsBitsGpu -------------------------------------------------------------
namespace rdoq {
enum { COEF, LEVEL, CLASS, QP, NNZ, STAT };
enum { RDOQ, BITS };
enum { S_QP, S_LAMBDA };
static size_t extent(int f, const Tuple &t)
{
    switch (f) {
    case COEF:
    case LEVEL: return t.n * 2048;
    case CLASS:
    case QP: return t.n;
    case NNZ: return t.n * 4;
    default: return t.n * 16;
    }
}
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
    s.qp = t.s[S_QP];
    s.lambda = t.s[S_LAMBDA];
    return s;
}
static void own(const Family &F, int c, const Tuple &b)
{
    const char *call = F.calls[c].name;
    auto rule = F.calls[c].rule;
    const bool bits = c == BITS;
    // in place: d_level == d_coef is accepted by the optimisation, one chunk apart is not; the estimate does not look at d_coef
    {
        Tuple t = b;
        t.p[LEVEL] = t.p[COEF];
        expect(call, "d_level == d_coef", rule(&t), false);
        t.p[LEVEL] = t.p[COEF] + 16;
        expect(call, "d_level one chunk into d_coef", rule(&t), !bits, args::kOverlap);
        t.p[LEVEL] = t.p[COEF] - 16;
        expect(call, "d_level one chunk before d_coef", rule(&t), !bits, args::kOverlap);
    }
    // beside d_qp the scalar qp is not looked at
    for (int q : {-1, 0, 51, 52}) {
        Tuple t = b;
        t.s[S_QP] = q;
        expect(call, "qp " + std::to_string(q) + " beside d_qp", rule(&t), false);
    }
    // n_regions == 0: nothing is looked at
    {
        Tuple t = b;
        t.n = 0;
        t.s[S_QP] = 99;
        t.s[S_LAMBDA] = -1;
        for (int f = 0; f <= STAT; ++f) t.p[f] = f % 2 ? 0 : 3;                 // NULL or misaligned
        expect(call, "no regions, the pointers NULL or odd, the scalars out of range", rule(&t), false);
    }
    // extents that saturate: no pointer has room for them
    {
        Tuple t = b;
        t.n = SIZE_MAX / 2048 + 1;                                              // n * 2048 wraps size_t
        expect(call, "n_regions * 2048 wraps", rule(&t), true, args::kNoFit);
        t.n = SIZE_MAX / 16 + 1;                                                // n * 16 wraps too
        expect(call, "n_regions * 16 wraps", rule(&t), true, args::kNoFit);
        t.n = ((size_t)1 << 52);                                                // 2^63 bytes of levels behind an address of 2^45: fits, and covers everything above it
        expect(call, "2^52 regions", rule(&t), true, args::kOverlap);
    }
}
static Family family()
{
    Family F = {};
    F.name = "x266_rdoq_t";
    F.fields = {{"d_coef", 16}, {"d_level", 16}, {"d_class", 1}, {"d_qp", 1}, {"d_nnz", 4}, {"d_stat", 8}};
    F.calls = {{"xRdoQuantRegionsGpu", apply<x266_rdoq_t, make, args::rdoq_regions>, {IN, OUT, OPT, OPT, OPT | OUT, OPT | OUT}, 0, 0, {{LEVEL, COEF}}},
               {"xLevelsBitsGpu", apply<x266_rdoq_t, make, args::levels_bits>, {UNUSED, IN, OPT, UNUSED, OPT, OUT}}};
    F.extent = extent;
    Tuple b = placed(F.fields);
    b.n = 7;
    b.s[S_QP] = 30;
    b.s[S_LAMBDA] = 368;
    F.bases = {b};
    F.scalars = {{"lambda", S_LAMBDA, 0, 8192, 1u << RDOQ, args::kRdoqScalars, -1}, {"qp without d_qp", S_QP, 0, 51, 1u << RDOQ, args::kRdoqScalars, QP}};
    F.own = own;
    return F;
}
}  // namespace rdoq

// ---- source analysis: xAqStatsGpu, xAqDecideGpu, xWeightsFromTotals --------------------------------------------------------------------
namespace aq {
enum { SRC, TILE, TOTAL, OFFSET, QP };
enum { STATS, DECIDE };
enum { S_MODE, S_STRENGTH, S_QP, S_CHROMA };
static size_t extent(int f, const Tuple &t)
{
    const size_t n_tiles = (size_t)(t.w / 16) * (size_t)(t.h / 16), n_ctu = (size_t)((t.w + 63) / 64) * (size_t)((t.h + 63) / 64);
    switch (f) {
    case SRC: return n_tiles * 512;
    case TILE: return n_tiles * 32;
    case TOTAL: return 64;
    case OFFSET: return n_tiles * 2;
    default: return n_ctu * 6;
    }
}
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
    s.mode = t.s[S_MODE];
    s.strength_q8 = t.s[S_STRENGTH];
    s.qp = t.s[S_QP];
    s.chroma_qp_offset = t.s[S_CHROMA];
    return s;
}
// the two outputs of decide: either alone is enough, none is refused; stats looks at neither
static void own(const Family &F, int c, const Tuple &b)
{
    const char *call = F.calls[c].name;
    auto rule = F.calls[c].rule;
    const bool decide = c == DECIDE;
    Tuple t = b;
    t.p[OFFSET] = t.p[QP] = 0;
    expect(call, "d_offset and d_qp both NULL", rule(&t), decide, "d_offset and d_qp are both NULL");
    t.p[OFFSET] = 3;
    t.p[QP] = (U)0 - 1;
    expect(call, "d_offset odd and d_qp at the last byte", rule(&t), decide);
    t = b;
    t.p[SRC] = 8;
    expect(call, "d_src misaligned", rule(&t), !decide, args::kMisaligned);
}
// xWeightsFromTotals (host pointers): every refusal of the header, and the ends of what it accepts
static void weights()
{
    const char *call = "xWeightsFromTotals";
    const int64_t good[8] = {5000000, 120000000000, 600000, 80000000, 610000, 81000000, 123456, 45};
    const x266_wp_t wp = {{{0, 0, 0}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}, {7, 0}};
    expect(call, "base", args::weights_from_totals(good, good, 0, &wp), false);
    expect(call, "NULL cur", args::weights_from_totals(nullptr, good, 0, &wp), true, args::kNull);
    expect(call, "NULL ref", args::weights_from_totals(good, nullptr, 0, &wp), true, args::kNull);
    expect(call, "NULL wp", args::weights_from_totals(good, good, 0, nullptr), true, args::kNull);
    range(call, "list", 0, 1, [&](int v) { return args::weights_from_totals(good, good, v, &wp); }, "list must be 0 or 1");
    for (int k = 0; k < 2; ++k)
        for (int v : {0, 7, 8, 255}) {
            x266_wp_t w = wp;
            w.log2_denom[k] = (uint8_t)v;
            expect(call, "log2_denom " + std::to_string(v), args::weights_from_totals(good, good, 1, &w), v > 7, "log2_denom must be 0..7");
        }
    for (int64_t v : {(int64_t)1, (int64_t)1 << 24, (int64_t)0, ((int64_t)1 << 24) + 1, (int64_t)-1, INT64_MAX}) {
        int64_t t[8];
        std::memcpy(t, good, sizeof t);
        t[7] = v;
        expect(call, "both tile counts " + std::to_string(v), args::weights_from_totals(t, t, 0, &wp), v < 1 || v > ((int64_t)1 << 24), "the tile count must be 1..2^24");
        expect(call, "cur's tile count " + std::to_string(v), args::weights_from_totals(t, good, 0, &wp), true, "the two frames differ in size");
        expect(call, "ref's tile count " + std::to_string(v), args::weights_from_totals(good, t, 0, &wp), true, "the two frames differ in size");
    }
    for (int i = 0; i < 7; ++i) {
        int64_t t[8];
        std::memcpy(t, good, sizeof t);
        t[i] = -1;
        expect(call, "cur[" + std::to_string(i) + "] negative", args::weights_from_totals(t, good, 0, &wp), true, "a total is negative");
        expect(call, "ref[" + std::to_string(i) + "] negative", args::weights_from_totals(good, t, 0, &wp), true, "a total is negative");
        t[i] = 0;
        expect(call, "cur[" + std::to_string(i) + "] 0", args::weights_from_totals(t, good, 0, &wp), false);
    }
}
static Family family()
{
    Family F = {};
    F.name = "x266_aq_t";
    F.fields = {{"d_src", 16}, {"d_tile", 16}, {"d_total", 8}, {"d_offset", 2}, {"d_qp", 1}};
    F.calls = {{"xAqStatsGpu", apply<x266_aq_t, make, args::aq_stats>, {IN, OUT, OUT, UNUSED, UNUSED}, SRC, ((U)1 << 63) + ((U)1 << 40)},
               {"xAqDecideGpu", apply<x266_aq_t, make, args::aq_decide>, {UNUSED, IN, IN, OPT | OUT, OPT | OUT}, TILE, (U)0 - ((U)1 << 58), {},
                (1u << OFFSET) | (1u << QP), "d_offset and d_qp are both NULL"}};
    F.extent = extent;
    Tuple b = placed(F.fields);                                                 // a frame of 9 x 5 tiles, 3 x 2 CTUs
    b.w = 144;
    b.h = 80;
    b.s[S_MODE] = 2;
    b.s[S_STRENGTH] = 256;
    b.s[S_QP] = 30;
    b.s[S_CHROMA] = -2;
    F.bases = {b};
    F.granule = 16;
    F.bad = {0, -16, 8, 24, 143, 145, INT_MIN, INT_MAX};
    F.good = {{16, 16}, {48, 80}, {64, 64}, {16, 16400}, {3840, 2176}, {7680, 4320}};
    F.scalars = {{"mode", S_MODE, 1, 2, 1u << DECIDE, args::kAqScalars, -1}, {"strength_q8", S_STRENGTH, 0, 1024, 1u << DECIDE, args::kAqScalars, -1},
                 {"qp", S_QP, 0, 51, 1u << DECIDE, args::kAqScalars, -1}, {"chroma_qp_offset", S_CHROMA, -12, 12, 1u << DECIDE, args::kAqScalars, -1}};
    F.own = own;
    F.once = weights;
    return F;
}
}  // namespace aq

// ---- lookahead: the five xLa...Gpu calls, xSceneCutFromTotals --------------------------------------------------------------------------
namespace la {
enum { SRC, LOW, INTRA, MODE, INTER0, INTER1, BLOCK, TOTAL, PROP, REF0, REF1, AQ, OFFSET, QP };
enum { DOWNSCALE, INTRA_COSTS, FRAME_COST, PROPAGATE, TREE_QP };
enum { S_PENALTY, S_STRENGTH, S_QP, S_CHROMA };
static size_t extent(int f, const Tuple &t)
{
    const size_t n = (size_t)(t.w / 16) * (size_t)(t.h / 16), n_ctu = (size_t)((t.w + 63) / 64) * (size_t)((t.h + 63) / 64);
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
    s.intra_penalty = t.s[S_PENALTY];
    s.strength_q8 = t.s[S_STRENGTH];
    s.qp = t.s[S_QP];
    s.chroma_qp_offset = t.s[S_CHROMA];
    return s;
}
// tree qp needs one of its two outputs, whatever else is NULL, and its qp map's extent is the CTUs'; the other calls look at neither.
// (The accumulators of propagate alias nothing -- each other, what the frame received -- and two lists may be one array: the walk's pairs.)
static void own(const Family &F, int c, const Tuple &b)
{
    const char *call = F.calls[c].name;
    auto rule = F.calls[c].rule;
    Tuple t = b;
    for (int f = 0; f <= QP; ++f)
        if ((F.calls[c].flags[f] & OPT) && f != QP) t.p[f] = 0;
    t.p[QP] = 0;
    expect(call, "d_offset and d_qp both NULL", rule(&t), c == TREE_QP, "d_offset and d_qp are both NULL");
    t = b;
    t.p[OFFSET] = 0;
    t.p[QP] = (U)0 - 37;                                                        // 6 CTUs, 36 bytes: the span ends one byte below the top
    expect(call, "d_qp ending just below the top", rule(&t), false);
    t.p[QP] = (U)0 - 35;
    expect(call, "d_qp one byte too far", rule(&t), c == TREE_QP, args::kNoFit);
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
static Family family()
{
    const int _ = UNUSED;
    const U high = (U)0 - ((U)1 << 40);
    Family F = {};
    F.name = "x266_la_t";
    F.fields = {{"d_src", 16},  {"d_low", 16},      {"d_intra", 4},     {"d_mode", 1},      {"d_inter0", 8},   {"d_inter1", 8}, {"d_block", 16},
                {"d_total", 8}, {"d_prop", 8},      {"d_prop_ref0", 8}, {"d_prop_ref1", 8}, {"d_aq_offset", 2}, {"d_offset", 2}, {"d_qp", 1}};
    //                                                 src low  intra mode       inter0 inter1 block total prop ref0       ref1       aq   offset     qp
    F.calls = {{"xLaDownscaleGpu", apply<x266_la_t, make, args::la_downscale>, {IN, OUT, _, _, _, _, _, _, _, _, _, _, _, _}, SRC, high},
               {"xLaIntraCostsGpu", apply<x266_la_t, make, args::la_intra_costs>, {_, IN, OUT, OPT | OUT, _, _, _, _, _, _, _, _, _, _}, LOW, high},
               {"xLaFrameCostGpu", apply<x266_la_t, make, args::la_frame_cost>, {_, _, IN, OPT, OPT, OPT, OUT, OUT, _, _, _, _, _, _}, INTRA, high},
               // an accumulator added into counts as an output
               {"xLaPropagateGpu", apply<x266_la_t, make, args::la_propagate>, {_, _, _, _, _, _, IN, _, OPT, OPT | OUT, OPT | OUT, _, _, _}, BLOCK, high},
               {"xLaTreeQpGpu", apply<x266_la_t, make, args::la_tree_qp>, {_, _, _, _, _, _, IN, _, OPT, _, _, OPT, OPT | OUT, OPT | OUT}, BLOCK, high, {},
                (1u << OFFSET) | (1u << QP), "d_offset and d_qp are both NULL"}};
    F.extent = extent;
    Tuple b = placed(F.fields);                                                 // a frame of 10 x 6 tiles, 3 x 2 CTUs
    b.w = 160;
    b.h = 96;
    b.s[S_PENALTY] = 300;
    b.s[S_STRENGTH] = 256;
    b.s[S_QP] = 30;
    b.s[S_CHROMA] = -2;
    F.bases = {b};
    F.granule = 32;
    F.bad = {0, -32, 8, 16, 48, 144, 159, 161, INT_MIN, INT_MAX};
    F.good = {{32, 32}, {64, 32}, {32, 64}, {96, 160}, {160, 96}, {32, 32800}, {3840, 2176}, {7680, 4320}};
    F.scalars = {{"intra_penalty", S_PENALTY, 0, 65535, 1u << FRAME_COST, args::kLaPenalty, -1}, {"strength_q8", S_STRENGTH, 0, 1024, 1u << TREE_QP, args::kLaScalars, -1},
                 {"qp", S_QP, 0, 51, 1u << TREE_QP, args::kLaScalars, -1}, {"chroma_qp_offset", S_CHROMA, -12, 12, 1u << TREE_QP, args::kLaScalars, -1}};
    F.own = own;
    F.once = scene_cut;
    return F;
}
}  // namespace la

// ---- the seeded search: xSatd8x8SeededSearchGpu, at both seed scales -------------------------------------------------------------------
namespace seed {
enum { CUR, REF, SEED, BEST, J };
enum { S_SCALE, S_CENTRES, S_RANGE, S_LAMBDA };
static size_t extent(int f, const Tuple &t)
{
    const size_t tiles = (size_t)(t.w / 16) * (size_t)(t.h / 16), blocks = (size_t)(t.w / 8) * (size_t)(t.h / 8);
    switch (f) {
    case CUR:
    case REF: return tiles * 512;
    case SEED: return (t.s[S_SCALE] ? tiles : blocks) * 8;
    case BEST: return blocks * 8;
    default: return blocks * 4;
    }
}
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
    s.seed_scale = t.s[S_SCALE];
    s.centres = t.s[S_CENTRES];
    s.range = t.s[S_RANGE];
    s.lambda_q4 = t.s[S_LAMBDA];
    return s;
}
static void own(const Family &F, int c, const Tuple &b)
{
    const char *call = F.calls[c].name;
    auto rule = F.calls[c].rule;
    const std::string at = "seed_scale " + std::to_string(b.s[S_SCALE]) + ": ";
    Tuple t = b;
    t.p[J] = 0;
    t.p[REF] = t.p[CUR];
    expect(call, at + "d_j NULL and one frame", rule(&t), false);
    for (int centres = 0; centres < 32; ++centres)
        for (int r = 0; r <= 8; ++r) {
            t = b;
            t.s[S_CENTRES] = centres;
            t.s[S_RANGE] = r;
            expect(call, at + "centres " + std::to_string(centres) + ", range " + std::to_string(r), rule(&t), false);
        }
    // the seeds' extent follows the scale: a d_best right behind the seeds of this scale is fine, one inside them is not
    t = b;
    t.p[BEST] = t.p[SEED] + extent(SEED, b);
    expect(call, at + "d_best right behind the seeds", rule(&t), false);
    t.p[BEST] -= 8;
    expect(call, at + "d_best on the last seed", rule(&t), true, args::kOverlap);
}
static Family family()
{
    Family F = {};
    F.name = "x266_seed_t";
    F.fields = {{"d_cur", 16}, {"d_ref", 16}, {"d_seed", 8}, {"d_best", 8}, {"d_j", 4}};
    // the two frames are read-only and may be one; in place is refused, the seeds included: blocks read their neighbours' seeds
    F.calls = {{"xSatd8x8SeededSearchGpu", apply<x266_seed_t, make, args::seeded_search>, {IN, IN, IN, OUT, OPT | OUT}, CUR, (U)0 - ((U)1 << 40)}};
    F.extent = extent;
    Tuple b = placed(F.fields);                                                 // a frame of 10 x 6 tiles
    b.w = 160;
    b.h = 96;
    b.s[S_CENTRES] = 31;
    b.s[S_RANGE] = 2;
    b.s[S_LAMBDA] = 16;
    F.bases = {b, b};
    F.bases[1].s[S_SCALE] = 1;
    F.granule = 16;
    F.bad = {0, -16, 8, 24, 152, 159, 161, INT_MIN, INT_MAX};
    F.good = {{16, 16}, {32, 16}, {16, 32}, {48, 32}, {96, 80}, {16, 32784}, {3840, 2176}, {7680, 4320}};
    F.scalars = {{"seed_scale", S_SCALE, 0, 1, 1u, args::kSeedScalars, -1}, {"centres", S_CENTRES, 0, 31, 1u, args::kSeedScalars, -1},
                 {"range", S_RANGE, 0, 8, 1u, args::kSeedScalars, -1}, {"lambda_q4", S_LAMBDA, 0, 65535, 1u, args::kSeedScalars, -1}};
    F.own = own;
    return F;
}
}  // namespace seed

// ---- mixed inter / intra coding of a frame: xDct32CodeMixedFrameGpu --------------------------------------------------------------------
namespace mixed {
enum { CUR, PRED, QP, KIND_IN, MODE_IN, LEVEL, NNZ, KIND, MODE, COST, RECON };
enum { S_QP, S_ROUNDING, S_PENALTY };
static size_t extent(int f, const Tuple &t)
{
    const size_t tiles = (size_t)(t.w / 16) * (size_t)(t.h / 16), regions = (size_t)(t.w / 64) * (size_t)(t.h / 64) * 6;
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
    s.qp = t.s[S_QP];
    s.rounding = t.s[S_ROUNDING];
    s.intra_penalty = t.s[S_PENALTY];
    return s;
}
static void own(const Family &F, int c, const Tuple &b)
{
    const char *call = F.calls[c].name;
    auto rule = F.calls[c].rule;
    Tuple t = b;                                                                // the encoder's form: all three at once, the optional outputs NULL
    t.p[RECON] = t.p[PRED];
    t.p[KIND] = t.p[KIND_IN];
    t.p[MODE] = t.p[MODE_IN];
    expect(call, "all three allowed overlaps", rule(&t), false);
    t.p[NNZ] = t.p[COST] = 0;
    expect(call, "all three allowed overlaps, d_nnz and d_cost NULL", rule(&t), false);
    t.p[CUR] = t.p[PRED];                                                       // ... but then the source is the reconstruction
    expect(call, "d_recon == d_pred == d_cur", rule(&t), true, args::kOverlap);
    t = b;
    t.p[PRED] = t.p[CUR];
    expect(call, "d_pred == d_cur", rule(&t), false);
    t = b;
    t.p[KIND] = t.p[MODE_IN];
    expect(call, "d_kind == d_mode_in", rule(&t), true, args::kOverlap);
    t = b;
    t.p[MODE] = t.p[KIND_IN];
    expect(call, "d_mode == d_kind_in", rule(&t), true, args::kOverlap);
    t = b;
    t.p[RECON] = t.p[CUR];
    expect(call, "d_recon == d_cur", rule(&t), true, args::kOverlap);
    for (int qp = 0; qp <= 51; ++qp) {
        t = b;
        t.p[QP] = 0;
        t.s[S_QP] = qp;
        expect(call, "qp " + std::to_string(qp), rule(&t), false);
    }
    for (int v : {-1, 52, 99, INT_MIN, INT_MAX}) {                              // with d_qp the scalar qp is not looked at; the rounding still is
        t = b;
        t.s[S_QP] = v;
        expect(call, "qp " + std::to_string(v) + " under d_qp", rule(&t), false);
        t.s[S_ROUNDING] = 512;
        expect(call, "qp " + std::to_string(v) + " under d_qp, rounding 512", rule(&t), true, args::kQuantScalars);
    }
    // the extents follow the frame: a buffer right behind another one of this frame is fine, one byte (alignment) earlier is not
    t = b;
    t.p[COST] = t.p[NNZ] + extent(NNZ, b);
    expect(call, "d_cost right behind d_nnz", rule(&t), false);
    t.p[COST] -= 4;
    expect(call, "d_cost on the last count", rule(&t), true, args::kOverlap);
    t = b;
    t.p[MODE] = t.p[KIND] + extent(KIND, b);
    expect(call, "d_mode right behind d_kind", rule(&t), false);
    t.p[MODE] -= 1;
    expect(call, "d_mode on the last kind", rule(&t), true, args::kOverlap);
    t = b;
    t.p[LEVEL] = t.p[RECON] + extent(RECON, b);
    expect(call, "d_level right behind d_recon", rule(&t), false);
    t.p[LEVEL] -= 16;
    expect(call, "d_level on the last tile", rule(&t), true, args::kOverlap);
}
static Family family()
{
    Family F = {};
    F.name = "x266_mixed_t";
    F.fields = {{"d_cur", 16},  {"d_pred", 16}, {"d_qp", 1},   {"d_kind_in", 1}, {"d_mode_in", 1}, {"d_level", 16},
                {"d_nnz", 4},   {"d_kind", 1},  {"d_mode", 1}, {"d_cost", 4},    {"d_recon", 16}};
    F.calls = {{"xDct32CodeMixedFrameGpu", apply<x266_mixed_t, make, args::mixed_code_frame>,
                {IN, IN, OPT | IN, OPT | IN, OPT | IN, OUT, OPT | OUT, OUT, OUT, OPT | OUT, OUT}, CUR, (U)0 - ((U)1 << 40),
                {{KIND, KIND_IN}, {MODE, MODE_IN}, {RECON, PRED}}}};
    F.extent = extent;
    Tuple b = placed(F.fields);                                                 // a frame of 3 x 2 CTUs
    b.w = 192;
    b.h = 128;
    b.s[S_QP] = 22;
    b.s[S_ROUNDING] = 171;
    b.s[S_PENALTY] = 4096;
    F.bases = {b};
    F.granule = 64;
    F.bad = {0, -64, 8, 16, 32, 96, 191, 193, 200, INT_MIN, INT_MAX};
    F.good = {{64, 64}, {128, 64}, {64, 128}, {192, 128}, {64, 32768}, {1920, 1088}, {3840, 2176}, {7680, 4352}};
    F.scalars = {{"qp", S_QP, 0, 51, 1u, args::kQuantScalars, QP}, {"rounding", S_ROUNDING, 0, 511, 1u, args::kQuantScalars, QP},   // without d_qp the scalar qp counts
                 {"intra_penalty", S_PENALTY, 0, 1 << 24, 1u, args::kMixedPenalty, QP}};
    F.own = own;
    return F;
}
}  // namespace mixed

int main()
{
    const Family families[] = {levels::family(), aq::family(), la::family(), seed::family(), mixed::family(), rdoq::family()};
    bool failed = false;
    for (const Family &F : families) {
        const int checks = g_checks, failures = g_failures;
        run(F);
        std::printf("checks %s %d\n", F.name, g_checks - checks);
        if (g_failures > failures) std::printf("%s: %d checks failed\n", F.name, g_failures - failures), failed = true;
    }
    if (failed) {
        std::printf("%d of %d checks failed\n", g_failures, g_checks);
        return 1;
    }
    std::printf("%zu families, %d checks: the argument rules hold\n", sizeof families / sizeof *families, g_checks);
    return 0;
}
