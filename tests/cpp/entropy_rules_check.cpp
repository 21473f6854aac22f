// CPU check of the argument rules of xEntropyEncodeLevelsGpu and xEntropyDecodeLevelsGpu (x266_amd/csrc/x266_args.hpp: entropy_encode,
// entropy_decode), the calls whose device pointers are the fields of the host-read x266_entropy_t, and of the coder the kernels share with
// the host through x266_amd/csrc/x266_entropy.hpp: the range coder, the syntax of a region and the default table, run here as plain C++
// against bytes and bin counts that tests/_entropy_ref.py gave (python tests/test_entropy_arg_rules.py prints the literals below).  The
// contract is written down once more by hand from include/x266hip.h -- per call the pointer fields in struct order with their alignments,
// which are written, which may be NULL, their extents -- and one walk perturbs a base tuple one field at a time: NULL, half an alignment,
// one alignment further, the top of the address space, every overlap of an output with any other buffer, a NULL d_stream with and without
// capacity, an entry of init at 30 and at 2018.  The addresses are made-up integers, nothing is dereferenced but the host table, no device
// is needed; the expected verdict of every check follows from these tables and from literals, never from the function under test.
// Test infrastructure; built and run by tests/test_entropy_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <climits>
#include <cstddef>
#include <string>
#include <vector>

#include "rules_expect.hpp"
#include "x266_args.hpp"
#include "x266_entropy.hpp"

using namespace x266;

static const char *SHARED = "x266_entropy.hpp";
enum { LEVEL, CLASS, NNZ, REGION, STREAM, TOTAL, N_FIELDS };
struct Field {
    const char *name;
    unsigned align;
    bool used[2], output[2], optional;                                      // per call: encode, decode
};
static const Field FIELDS[N_FIELDS] = {{"d_level", 16, {true, true}, {false, true}, false}, {"d_class", 1, {true, true}, {false, false}, true},
                                       {"d_nnz", 4, {true, true}, {false, true}, true},     {"d_region", 8, {true, true}, {true, false}, false},
                                       {"d_stream", 16, {true, true}, {true, false}, false}, {"d_total", 8, {true, false}, {true, false}, false}};
static const char *CALLS[2] = {"xEntropyEncodeLevelsGpu", "xEntropyDecodeLevelsGpu"};
struct Tuple {
    U p[N_FIELDS];
    const uint16_t *init;
    size_t n;
    uint64_t cap;
};

static size_t extent(int f, const Tuple &t)
{
    if (f == LEVEL) return t.n * 2048;
    if (f == CLASS) return t.n;
    if (f == NNZ) return t.n * 4;
    if (f == REGION) return t.n * 32;
    if (f == STREAM) return t.cap > SIZE_MAX / 2 ? SIZE_MAX : (size_t)t.cap * 2;
    return 16;
}
static const char *rule(int call, const Tuple &t)
{
    x266_entropy_t s = {};
    s.d_level = (int16_t *)t.p[LEVEL];
    s.d_class = (const uint8_t *)t.p[CLASS];
    s.d_nnz = (uint32_t *)t.p[NNZ];
    s.d_region = (x266_entropy_region_t *)t.p[REGION];
    s.d_stream = (uint16_t *)t.p[STREAM];
    s.d_total = (uint64_t *)t.p[TOTAL];
    s.init = t.init;
    s.n_regions = t.n;
    s.cap_words = t.cap;
    return call == 0 ? args::entropy_encode(&s) : args::entropy_decode(&s);
}
// every pointer in a region of its own, at exactly its alignment times an odd number
static Tuple placed(size_t n, uint64_t cap)
{
    Tuple t = {};
    for (int i = 0; i < N_FIELDS; ++i) t.p[i] = ((U)(i + 1) << 44) + (U)FIELDS[i].align * (2 * i + 1);
    t.n = n;
    t.cap = cap;
    return t;
}

static void walk(int call, const Tuple &b, const std::string &label)
{
    const char *CALL = CALLS[call];
    expect(CALL, label + "base", rule(call, b), false);
    for (int f = 0; f < N_FIELDS; ++f) {
        const unsigned align = FIELDS[f].align;
        const std::string name = label + FIELDS[f].name;
        const size_t bytes = extent(f, b);
        Tuple t = b;
        if (!FIELDS[f].used[call]) {                                        // d_total of the decode call: not looked at, whatever it is
            t.p[f] = 0;
            expect(CALL, name + " NULL, not used", rule(call, t), false);
            t.p[f] = 3;
            expect(CALL, name + " misaligned, not used", rule(call, t), false);
            t.p[f] = b.p[LEVEL];
            expect(CALL, name + " on d_level, not used", rule(call, t), false);
            continue;
        }
        t.p[f] = 0;                                                         // d_stream may be NULL exactly when cap_words is 0
        expect(CALL, name + " NULL", rule(call, t), !FIELDS[f].optional && (f != STREAM || b.cap != 0), args::kNull);
        if (align > 1) {
            t = b;
            t.p[f] += align / 2;
            expect(CALL, name + " at half its alignment", rule(call, t), true, args::kMisaligned);
        }
        t = b;
        t.p[f] += align;
        expect(CALL, name + " one alignment further", rule(call, t), false);
        if (bytes > align) {
            t = b;
            t.p[f] = (U)0 - align;                                          // the last aligned address: the extent is larger and wraps
            expect(CALL, name + " running past the top of the address space", rule(call, t), true, args::kNoFit);
        }
        if (bytes) {
            t = b;
            t.p[f] = down((U)0 - bytes - align, align);                     // the span ends just below the top
            expect(CALL, name + " ending just below the top", rule(call, t), false);
            t.p[f] = down((U)0 - bytes + align, align);                     // ... and just above it
            if (t.p[f]) expect(CALL, name + " ending just above the top", rule(call, t), true, args::kNoFit);
        }
        // overlaps: field f placed onto every other buffer g of the call -- refused iff one of the two is an output and both have bytes
        for (int g = 0; g < N_FIELDS; ++g) {
            if (g == f || !FIELDS[g].used[call]) continue;
            const size_t other = extent(g, b);
            if (!bytes || !other) continue;                                 // an empty stream overlaps nothing
            const bool bad = FIELDS[f].output[call] || FIELDS[g].output[call];
            const std::string on = name + " on " + FIELDS[g].name;
            t = b;
            t.p[f] = b.p[g];
            if (t.p[f] % align == 0) expect(CALL, on + ": same address", rule(call, t), bad, args::kOverlap);
            t.p[f] = down(b.p[g] + other - 1, align);                       // onto g's last byte
            expect(CALL, on + ": its last bytes", rule(call, t), bad, args::kOverlap);
            t.p[f] = up(b.p[g] + other, align);                             // right behind g
            expect(CALL, on + ": right behind it", rule(call, t), false);
            t.p[f] = down(b.p[g] - bytes, align);                           // ending where g begins, or before
            expect(CALL, on + ": right in front of it", rule(call, t), false);
            t.p[f] = down(b.p[g] - bytes, align) + align;                   // f's last bytes reach into g ...
            if (t.p[f] + bytes > b.p[g]) expect(CALL, on + ": its last bytes reach in", rule(call, t), bad, args::kOverlap);
        }
    }
}

static void table_and_capacity(int call, const Tuple &b)
{
    const char *CALL = CALLS[call];
    uint16_t table[X266_ENTROPY_CONTEXTS];
    for (unsigned i = 0; i < X266_ENTROPY_CONTEXTS; ++i) table[i] = (uint16_t)(31 + (i * 1986u) / 99u);      // 31 .. 2017, both ends taken
    Tuple t = b;
    t.init = table;
    expect(CALL, "a table over the whole interval", rule(call, t), false);
    for (unsigned at : {0u, 24u, 57u, 99u}) {
        const uint16_t was = table[at];
        for (unsigned bad : {30u, 2018u, 0u, 2048u, 65535u}) {
            table[at] = (uint16_t)bad;
            expect(CALL, "init[" + std::to_string(at) + "] = " + std::to_string(bad), rule(call, t), true, args::kEntropyInit);
        }
        for (unsigned good : {31u, 2017u}) {
            table[at] = (uint16_t)good;
            expect(CALL, "init[" + std::to_string(at) + "] = " + std::to_string(good), rule(call, t), false);
        }
        table[at] = was;
    }
    table[5] = 30;                                                          // the table is looked at even where no region is
    t.n = 0;
    expect(CALL, "a bad table with no regions", rule(call, t), true, args::kEntropyInit);
    t = b;                                                                  // a NULL d_stream with a non-zero capacity, and the count-only form
    t.p[STREAM] = 0;
    t.cap = 1;
    expect(CALL, "d_stream NULL with cap_words 1", rule(call, t), true, args::kNull);
    t.cap = 0;
    expect(CALL, "d_stream NULL with cap_words 0", rule(call, t), false);
    t = b;
    t.cap = 0;
    expect(CALL, "a d_stream with cap_words 0", rule(call, t), false);
    t.p[STREAM] += 8;
    expect(CALL, "... which still is aligned", rule(call, t), true, args::kMisaligned);
    t = b;
    t.cap = UINT64_MAX;                                                     // a capacity whose bytes saturate fits behind no pointer
    expect(CALL, "cap_words 2^64 - 1", rule(call, t), true, args::kNoFit);
    t.cap = (uint64_t)1 << 63;
    expect(CALL, "cap_words 2^63", rule(call, t), true, args::kNoFit);
    t = b;
    t.n = SIZE_MAX / 1024;                                                  // n_regions * 2048 wraps
    expect(CALL, "n_regions whose levels wrap", rule(call, t), true);
    Tuple none = {};                                                        // no regions: encode looks at d_total alone, decode at nothing
    expect(CALL, "no regions, all NULL", rule(call, none), call == 0, args::kNull);
    none.p[TOTAL] = b.p[TOTAL];
    expect(CALL, "no regions, d_total", rule(call, none), false);
    none.p[TOTAL] += 4;
    expect(CALL, "no regions, d_total misaligned", rule(call, none), call == 0, args::kMisaligned);
}

// ---- the coder against what tests/_entropy_ref.py gave ------------------------------------------------------------------------------------------
// CASE: {k, table (0 the default, 1 every entry 2017, 2 entry i = 31 + (i * 1986) / 99), seed of the levels, non-zero levels, context bins,
// bypass bins, n_bytes, row of BYTES}.  The levels of a case: x = seed; per index x = x * 1103515245 + 12345 (mod 2^32); the level is non-zero
// when (x >> 16) % 97 < density, density = seed % 37 + 1, and then ((x >> 8) % 7 == 0 ? (x >> 9) % 65535 - 32767 : (x >> 20) % 9 - 4), 0 -> 1;
// seed 0 is the all-zero region, seed 1 all 1024 levels at +-32767 (negative at every third index).  BYTES: a case's first 24 bytes, and
// the sum of all of them in the last column.
static const int CASE[16][8] = {{3, 0, 0, 0, 1, 0, 0, 0}, {0, 0, 0, 0, 64, 0, 0, 1}, {3, 0, 5, 58, 810, 331, 101, 2}, {2, 0, 6, 78, 954, 538, 143, 3}, {1, 0, 7, 82, 1017, 486, 142, 4}, {0, 0, 8, 101, 1082, 703, 177, 5}, {3, 2, 40, 48, 689, 289, 98, 6}, {2, 2, 77, 45, 736, 262, 89, 7}, {1, 2, 114, 49, 828, 379, 101, 8}, {0, 2, 36, 384, 1976, 2258, 481, 9}, {3, 0, 73, 428, 1837, 2626, 546, 10}, {0, 1, 1, 1024, 3456, 33792, 4329, 11}, {1, 1, 1, 1024, 3264, 33824, 4342, 12}, {2, 1, 1, 1024, 3184, 33808, 4314, 13}, {3, 1, 1, 1024, 3152, 33798, 4289, 14}, {3, 0, 2, 30, 488, 237, 66, 15}};
static const int BYTES[16][25] = {{-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0}, {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0}, {255, 215, 253, 214, 160, 155, 95, 192, 53, 41, 151, 127, 63, 19, 149, 88, 15, 41, 34, 67, 153, 136, 114, 182, 12516}, {255, 63, 131, 142, 196, 241, 65, 190, 96, 230, 152, 152, 181, 38, 35, 150, 153, 147, 234, 74, 158, 46, 248, 171, 18791}, {255, 240, 71, 129, 185, 32, 95, 245, 172, 142, 246, 7, 5, 141, 8, 242, 243, 98, 241, 113, 152, 219, 72, 161, 17906}, {252, 27, 111, 166, 189, 222, 127, 16, 138, 59, 13, 133, 143, 71, 4, 215, 137, 15, 139, 227, 29, 116, 205, 199, 21110}, {255, 255, 255, 186, 81, 120, 254, 147, 248, 235, 234, 102, 218, 68, 58, 235, 157, 20, 217, 99, 74, 109, 90, 98, 12578}, {254, 246, 104, 52, 141, 31, 219, 57, 255, 30, 50, 54, 219, 225, 219, 88, 129, 181, 90, 129, 175, 50, 16, 75, 11217}, {220, 169, 203, 57, 98, 122, 171, 209, 90, 104, 164, 182, 57, 94, 242, 154, 135, 230, 241, 50, 150, 223, 169, 191, 14741}, {79, 117, 167, 45, 58, 50, 76, 4, 71, 178, 251, 134, 62, 35, 62, 155, 216, 215, 87, 154, 45, 137, 251, 6, 60338}, {255, 255, 255, 151, 110, 118, 184, 133, 47, 105, 178, 152, 254, 129, 110, 80, 249, 0, 213, 58, 12, 64, 172, 197, 66411}, {255, 255, 255, 254, 255, 255, 255, 255, 255, 253, 19, 173, 14, 21, 255, 252, 241, 170, 202, 115, 255, 229, 170, 201, 566483}, {255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 90, 47, 172, 188, 127, 255, 80, 213, 160, 164, 249, 564659}, {255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 219, 134, 165, 125, 230, 255, 217, 223, 551991}, {255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 247, 239, 172, 198, 23, 547470}, {255, 255, 249, 254, 210, 251, 113, 92, 107, 8, 71, 77, 85, 59, 164, 127, 129, 217, 149, 156, 79, 182, 137, 62, 9102}};

static void truth(const std::string &what, bool ok) { expect(SHARED, what, ok ? nullptr : "differs from the reference's value", false); }

static void case_levels(unsigned seed, int16_t *level)
{
    uint32_t x = seed;
    const unsigned density = seed % 37 + 1;
    for (unsigned i = 0; i < 1024; ++i) {
        x = x * 1103515245u + 12345u;
        int l = 0;
        if (seed == 1) {
            l = i % 3 == 0 ? -32767 : 32767;
        } else if (seed != 0 && (x >> 16) % 97 < density) {
            l = (x >> 8) % 7 == 0 ? (int)((x >> 9) % 65535) - 32767 : (int)((x >> 20) % 9) - 4;
            if (l == 0) l = 1;
        }
        level[i] = (int16_t)l;
    }
}

static void case_table(int kind, unsigned k, uint16_t *ctx)
{
    for (unsigned i = 0; i < kEntropyCtxPerSize; ++i) {
        const unsigned at = k * kEntropyCtxPerSize + i;
        ctx[i] = kind == 0 ? kEntropyDefault.p[at] : kind == 1 ? (uint16_t)2017 : (uint16_t)(31 + (at * 1986u) / 99u);
    }
}

static void shared_coder()
{
    const int n_cases = (int)(sizeof(CASE) / sizeof(CASE[0]));
    std::vector<uint8_t> out(kEntropyMaxBytes);
    int16_t level[1024], back[1024];
    for (int c = 0; c < n_cases; ++c) {
        const unsigned k = (unsigned)CASE[c][0];
        const std::string what = "case " + std::to_string(c);
        case_levels((unsigned)CASE[c][2], level);
        unsigned nz = 0;
        for (int i = 0; i < 1024; ++i) nz += level[i] != 0;
        truth(what + ": the levels", nz == (unsigned)CASE[c][3]);
        uint16_t ctx[kEntropyCtxPerSize];
        case_table(CASE[c][1], k, ctx);
        EntropyEnc e;
        entropy_enc_start(e, out.data(), (uint32_t)out.size());
        entropy_encode_region(e, level, k, entropy_cg_mask(level, k), ctx);
        const uint32_t n_bytes = entropy_enc_finish(e);
        truth(what + ": bins", e.ctx_bins == (uint32_t)CASE[c][4] && e.bypass_bins == (uint32_t)CASE[c][5]);
        truth(what + ": n_bytes", n_bytes == (uint32_t)CASE[c][6] && n_bytes <= kEntropyMaxBytes);
        long sum = 0;
        bool head = true;
        for (uint32_t i = 0; i < n_bytes && i < out.size(); ++i) {
            sum += out[i];
            if (i < 24) head = head && out[i] == BYTES[CASE[c][7]][i];
        }
        for (uint32_t i = n_bytes; i < 24; ++i) head = head && BYTES[CASE[c][7]][i] == -1;
        truth(what + ": bytes", head && sum == BYTES[CASE[c][7]][24]);
        // the sink stores nothing at or beyond its capacity, and counts all the same
        if (n_bytes > 2) {
            std::vector<uint8_t> tight(n_bytes / 2);                        // the sanitizers watch the byte behind it
            case_table(CASE[c][1], k, ctx);
            entropy_enc_start(e, tight.data(), (uint32_t)tight.size());
            entropy_encode_region(e, level, k, entropy_cg_mask(level, k), ctx);
            truth(what + ": a tight sink", entropy_enc_finish(e) == n_bytes && !std::memcmp(tight.data(), out.data(), tight.size()));
        }
        case_table(CASE[c][1], k, ctx);
        entropy_enc_start(e, nullptr, 0);
        entropy_encode_region(e, level, k, entropy_cg_mask(level, k), ctx);
        truth(what + ": no sink", entropy_enc_finish(e) == n_bytes);
        // and back: a buffer of exactly n_bytes, so that a read beyond the end is a finding
        std::vector<uint8_t> exact(out.begin(), out.begin() + n_bytes);
        case_table(CASE[c][1], k, ctx);
        for (int i = 0; i < 1024; ++i) back[i] = 0;
        EntropyDec d;
        entropy_dec_start(d, exact.data(), n_bytes);
        uint32_t count = 0;
        const bool good = entropy_decode_region(d, back, k, ctx, &count);
        truth(what + ": the round trip", good && count == nz && !std::memcmp(back, level, sizeof level));
    }
    // garbage terminates, inside its buffer, and is malformed where every bin is a one
    std::vector<uint8_t> ones(64, 0xFF);
    for (unsigned k = 0; k < 4; ++k) {
        uint16_t ctx[kEntropyCtxPerSize];
        case_table(0, k, ctx);
        for (int i = 0; i < 1024; ++i) back[i] = 0;
        EntropyDec d;
        entropy_dec_start(d, ones.data(), (uint32_t)ones.size());
        uint32_t count = 0;
        truth("0xFF bytes are malformed at size " + std::to_string(4 << k), !entropy_decode_region(d, back, k, ctx, &count));
    }
    truth("the default table", kEntropyDefault.p[0] == 1024 && kEntropyDefault.p[18] == 1024 && kEntropyDefault.p[19] == 1385 && kEntropyDefault.p[20] == 723 &&
                                   kEntropyDefault.p[21] == 1242 && kEntropyDefault.p[22] == 1609 && kEntropyDefault.p[23] == 1325 && kEntropyDefault.p[24] == 1263 &&
                                   kEntropyDefault.p[99] == 1263 && kEntropyDefault.p[75] == 1024);
    truth("groups", entropy_last_group(0) == 0 && entropy_last_group(3) == 3 && entropy_last_group(4) == 4 && entropy_last_group(6) == 5 && entropy_last_group(8) == 6 &&
                        entropy_last_group(31) == 9 && entropy_last_group(16) == 8 && entropy_last_group(24) == 9);
    truth("inverse scans", entropy_cg_scan(3, 0, 0) == 0 && entropy_cg_scan(3, 7, 7) == 63 && entropy_cg_scan(1, 1, 0) == 2 && entropy_cg_scan(1, 0, 1) == 1 &&
                               entropy_pos4(0, 1) == 1 && entropy_pos4(1, 0) == 2 && entropy_pos4(3, 3) == 15);
}

int main()
{
    for (int call = 0; call < 2; ++call) {
        std::printf("%s:", CALLS[call]);
        bool first = true;
        for (int f = 0; f < N_FIELDS; ++f)
            if (FIELDS[f].used[call]) {
                std::printf("%s %s %u %s%s", first ? "" : ",", FIELDS[f].name, FIELDS[f].align, FIELDS[f].optional ? "opt " : "", FIELDS[f].output[call] ? "out" : "in");
                first = false;
            }
        std::printf("\n");
    }
    static_assert(sizeof(x266_entropy_region_t) == 32 && offsetof(x266_entropy_region_t, ctx_bins) == 0 && offsetof(x266_entropy_region_t, bypass_bins) == 4 &&
                      offsetof(x266_entropy_region_t, offset) == 8 && offsetof(x266_entropy_region_t, n_words) == 16 && offsetof(x266_entropy_region_t, n_bytes) == 20 &&
                      offsetof(x266_entropy_region_t, n_nz) == 24 && offsetof(x266_entropy_region_t, reserved) == 28,
                  "the record of the header");
    static_assert(offsetof(x266_level_region_t, offset) == 8 && offsetof(x266_level_region_t, n_words) == 16, "the first 20 bytes are the level record's");
    static_assert(offsetof(x266_entropy_t, init) == 48 && offsetof(x266_entropy_t, n_regions) == 56 && offsetof(x266_entropy_t, cap_words) == 64, "the struct of the header");
    static_assert(X266_ENTROPY_CONTEXTS == 100 && X266_ENTROPY_MAX_BYTES == 6848, "the header's constants");
    std::printf("sizeof(x266_entropy_region_t) %zu\nsizeof(x266_entropy_t) %zu\n", sizeof(x266_entropy_region_t), sizeof(x266_entropy_t));
    for (int call = 0; call < 2; ++call) {
        ++g_checks;
        if (!(call == 0 ? args::entropy_encode(nullptr) : args::entropy_decode(nullptr)))
            ++g_failures, std::printf("FAIL a NULL parameter struct is accepted\n");
        for (size_t n : {(size_t)1, (size_t)5, (size_t)1025, (size_t)12240})
            for (uint64_t cap : {(uint64_t)4096, (uint64_t)0, (uint64_t)3}) {
                const Tuple b = placed(n, cap);
                walk(call, b, std::to_string(n) + " regions cap " + std::to_string(cap) + " ");
                if (cap == 4096 && n == 5) table_and_capacity(call, b);
            }
    }
    shared_coder();
    std::printf("checks x266_entropy_t %d\n", g_checks);
    if (g_failures) {
        std::printf("%d of %d checks FAILED\n", g_failures, g_checks);
        return 1;
    }
    std::printf("the argument rules hold (%d checks)\n", g_checks);
    return 0;
}
