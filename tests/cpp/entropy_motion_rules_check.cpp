// CPU check of the argument rules of xEntropyEncodeMvGpu, xEntropyDecodeMvGpu and xMotionReconstructGpu (x266_amd/csrc/x266_args.hpp:
// entropy_motion_encode, entropy_motion_decode, motion_reconstruct), the calls whose device pointers are the fields of the host-read
// x266_entropy_motion_t and x266_motion_t, and of the syntax the kernels share with the host through x266_amd/csrc/x266_entropy_motion.hpp,
// run here as plain C++ against the worked values of include/x266hip.h (tests/test_entropy_motion_ref.py holds the same values against
// tests/_entropy_motion_ref.py).  The contract is written down once more by hand from the header -- per call the pointer fields in struct
// order with their alignments, which are written, which may be NULL, their extents -- and one walk perturbs a base tuple one field at a
// time: NULL, half an alignment, one alignment further, the top of the address space, every overlap of an output with any other buffer, a
// NULL d_stream and a NULL d_words with and without their counts, an entry of init at 30 and at 2018, sides that are no multiple of 16.
// The addresses are made-up integers, nothing is dereferenced but the host table, no device is needed; the expected verdict of every
// check follows from these tables and from literals, never from the function under test.
// Test infrastructure; built and run by tests/test_entropy_motion_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <climits>
#include <cstddef>
#include <string>
#include <vector>

#include "rules_expect.hpp"
#include "x266_args.hpp"
#include "x266_entropy_motion.hpp"

using namespace x266;

static const char *SHARED = "x266_entropy_motion.hpp";
enum { CTU, WORDS, CODED, STREAM, TOTAL, STATUS, N_FIELDS };
struct Field {
    const char *name;
    unsigned align;
    bool used[2], output[2], optional;                                      // per call: encode, decode
};
static const Field FIELDS[N_FIELDS] = {{"d_ctu", 8, {true, true}, {false, true}, false},    {"d_words", 16, {true, true}, {false, true}, false},
                                       {"d_coded", 8, {true, true}, {true, false}, false},  {"d_stream", 16, {true, true}, {true, false}, false},
                                       {"d_total", 8, {true, false}, {true, false}, false}, {"d_status", 1, {false, true}, {false, true}, true}};
static const char *CALLS[2] = {"xEntropyEncodeMvGpu", "xEntropyDecodeMvGpu"};
static const char *RECON = "xMotionReconstructGpu";
struct Tuple {
    U p[N_FIELDS];
    const uint16_t *init;
    int w, h;
    uint64_t in, cap;
};

static size_t n_ctus(const Tuple &t) { return (size_t)((t.w + 63) / 64) * (size_t)((t.h + 63) / 64); }
static size_t words2(uint64_t n) { return n > SIZE_MAX / 2 ? SIZE_MAX : (size_t)n * 2; }
static size_t extent(int call, int f, const Tuple &t)
{
    if (f == CTU || f == CODED) return n_ctus(t) * 32;
    if (f == WORDS) return call == 0 ? words2(t.in) : n_ctus(t) * 512;
    if (f == STREAM) return words2(t.cap);
    if (f == TOTAL) return 16;
    return n_ctus(t);
}
static const char *rule(int call, const Tuple &t)
{
    x266_entropy_motion_t s = {};
    s.d_ctu = (x266_motion_ctu_t *)t.p[CTU];
    s.d_words = (uint16_t *)t.p[WORDS];
    s.d_coded = (x266_entropy_motion_ctu_t *)t.p[CODED];
    s.d_stream = (uint16_t *)t.p[STREAM];
    s.d_total = (uint64_t *)t.p[TOTAL];
    s.d_status = (uint8_t *)t.p[STATUS];
    s.init = t.init;
    s.width = t.w;
    s.height = t.h;
    s.in_words = t.in;
    s.cap_words = t.cap;
    return call == 0 ? args::entropy_motion_encode(&s) : args::entropy_motion_decode(&s);
}
// every pointer in a region of its own, at exactly its alignment times an odd number
static Tuple placed(int w, int h, uint64_t in, uint64_t cap)
{
    Tuple t = {};
    for (int i = 0; i < N_FIELDS; ++i) t.p[i] = ((U)(i + 1) << 44) + (U)FIELDS[i].align * (2 * i + 1);
    t.w = w;
    t.h = h;
    t.in = in;
    t.cap = cap;
    return t;
}
static bool may_be_null(int call, int f, const Tuple &b)
{
    if (FIELDS[f].optional) return true;
    if (f == STREAM) return b.cap == 0;
    return f == WORDS && call == 0 && b.in == 0;
}

// do [x, x + n) and [y, y + m) share a byte
static bool meet(U x, size_t n, U y, size_t m) { return x < y + m && y < x + n; }

static void walk(int call, const Tuple &b, const std::string &label)
{
    const char *CALL = CALLS[call];
    expect(CALL, label + "base", rule(call, b), false);
    for (int f = 0; f < N_FIELDS; ++f) {
        const unsigned align = FIELDS[f].align;
        const std::string name = label + FIELDS[f].name;
        const size_t bytes = extent(call, f, b);
        Tuple t = b;
        if (!FIELDS[f].used[call]) {                                        // d_total of decode, d_status of encode: not looked at
            t.p[f] = 0;
            expect(CALL, name + " NULL, not used", rule(call, t), false);
            t.p[f] = 3;
            expect(CALL, name + " misaligned, not used", rule(call, t), false);
            t.p[f] = b.p[CODED];
            expect(CALL, name + " on d_coded, not used", rule(call, t), false);
            continue;
        }
        t.p[f] = 0;
        expect(CALL, name + " NULL", rule(call, t), !may_be_null(call, f, b), args::kNull);
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
            const size_t other = extent(call, g, b);
            if (!bytes || !other) continue;                                 // an empty stream overlaps nothing
            const bool bad = FIELDS[f].output[call] || FIELDS[g].output[call];
            const std::string on = name + " on " + FIELDS[g].name;
            t = b;
            t.p[f] = b.p[g];
            if (t.p[f] % align == 0) expect(CALL, on + ": same address", rule(call, t), bad, args::kOverlap);
            t.p[f] = down(b.p[g] + other - 1, align);                       // onto g's last byte, if rounding down leaves f long enough to reach it
            expect(CALL, on + ": its last bytes", rule(call, t), bad && meet(t.p[f], bytes, b.p[g], other), args::kOverlap);
            t.p[f] = up(b.p[g] + other, align);                             // right behind g
            expect(CALL, on + ": right behind it", rule(call, t), false);
            t.p[f] = down(b.p[g] - bytes, align);                           // ending where g begins, or before
            expect(CALL, on + ": right in front of it", rule(call, t), false);
            t.p[f] = down(b.p[g] - bytes, align) + align;                   // f's last bytes reach into g ...
            if (t.p[f] + bytes > b.p[g]) expect(CALL, on + ": its last bytes reach in", rule(call, t), bad && meet(t.p[f], bytes, b.p[g], other), args::kOverlap);
        }
    }
}

static void table_sides_and_counts(int call, const Tuple &b)
{
    const char *CALL = CALLS[call];
    uint16_t table[X266_ENTROPY_MOTION_CONTEXTS];
    for (unsigned i = 0; i < X266_ENTROPY_MOTION_CONTEXTS; ++i) table[i] = (uint16_t)(31 + i * 331u);       // 31 .. 2017, both ends taken
    Tuple t = b;
    t.init = table;
    expect(CALL, "a table over the whole interval", rule(call, t), false);
    for (unsigned at : {0u, 2u, 3u, 6u}) {
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
    for (int side = 0; side < 2; ++side)
        for (int v : {0, -16, 8, 24, 1, INT_MIN, INT_MAX}) {
            t = b;
            (side ? t.h : t.w) = v;
            expect(CALL, std::string(side ? "height " : "width ") + std::to_string(v), rule(call, t), true);
        }
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
    t = b;                                                                  // in_words: the extent of d_words on encode, ignored on decode
    t.in = UINT64_MAX;
    expect(CALL, "in_words 2^64 - 1", rule(call, t), call == 0, args::kNoFit);
    t.in = (uint64_t)1 << 63;
    expect(CALL, "in_words 2^63", rule(call, t), call == 0, args::kNoFit);
    t = b;
    t.p[WORDS] = 0;
    t.in = 0;
    expect(CALL, "d_words NULL with in_words 0", rule(call, t), call == 1, args::kNull);
    t.in = 4;
    expect(CALL, "d_words NULL with in_words 4", rule(call, t), true, args::kNull);
}

// xMotionReconstructGpu: the rules of xMotionUnpackGpu, which tests/cpp/motion_rules_check.cpp walks; here that it is those rules
static void reconstruct_rules()
{
    x266_motion_t base = {};
    base.d_mv = (x266_me_result_t *)(((U)1 << 44) + 8);
    base.d_level = (uint8_t *)(((U)2 << 44) + 3);
    base.d_ctu = (x266_motion_ctu_t *)(((U)3 << 44) + 40);
    base.d_stream = (uint16_t *)(((U)4 << 44) + 112);
    base.width = 144;
    base.height = 112;
    base.cap_words = 4096;
    expect(RECON, "base", args::motion_reconstruct(&base), false);
    expect(RECON, "NULL p", args::motion_reconstruct(nullptr), true);
    x266_motion_t t = base;
    t.d_total = (uint64_t *)3;
    expect(RECON, "d_total is not looked at", args::motion_reconstruct(&t), false);
    t = base;
    t.d_mv = nullptr;
    expect(RECON, "d_mv NULL", args::motion_reconstruct(&t), true, args::kNull);
    t = base;
    t.d_level = nullptr;
    expect(RECON, "d_level NULL", args::motion_reconstruct(&t), true, args::kNull);
    t = base;
    t.d_ctu = (x266_motion_ctu_t *)((U)base.d_ctu + 4);
    expect(RECON, "d_ctu at half its alignment", args::motion_reconstruct(&t), true, args::kMisaligned);
    t = base;
    t.d_stream = nullptr;
    expect(RECON, "d_stream NULL with a capacity", args::motion_reconstruct(&t), true, args::kNull);
    t.cap_words = 0;
    expect(RECON, "d_stream NULL without", args::motion_reconstruct(&t), false);
    t = base;
    t.d_level = (uint8_t *)base.d_ctu;
    expect(RECON, "d_level on d_ctu", args::motion_reconstruct(&t), true, args::kOverlap);
    t = base;
    t.d_mv = (x266_me_result_t *)base.d_stream;
    expect(RECON, "d_mv on d_stream", args::motion_reconstruct(&t), true, args::kOverlap);
    t = base;
    t.width = 152;
    expect(RECON, "width 152", args::motion_reconstruct(&t), true);
    t = base;
    t.cap_words = (uint64_t)1 << 63;
    expect(RECON, "cap_words 2^63", args::motion_reconstruct(&t), true, args::kNoFit);
    for (int w : {16, 64, 80, 65664})
        for (int h : {16, 48, 1104}) {
            t = base;
            t.width = w;
            t.height = h;
            expect(RECON, "sizes agree with unpack", args::motion_reconstruct(&t), args::motion_unpack(&t) != nullptr);
        }
}

// ---- the syntax against the header's worked values ------------------------------------------------------------------------------------------
struct Worked {
    int w, h;
    uint64_t mask;
    int parts, d[4][2], n_bytes, bytes[9];
    unsigned ctx_bins, bypass_bins;
};
static const Worked WORKED[7] = {
    {64, 64, 1, 1, {{0, 0}}, 0, {}, 3, 0},
    {64, 64, 1, 1, {{1, 0}}, 1, {0x40}, 4, 1},
    {64, 64, 1, 1, {{-2, 5}}, 2, {0x67, 0x90}, 5, 8},
    {64, 64, 1, 1, {{-65535, 65535}}, 9, {0x7f, 0xff, 0xbb, 0xff, 0xff, 0xff, 0xdf, 0xff, 0xc0}, 5, 62},
    {32, 32, 0x1111, 4, {{4, -8}, {0, 0}, {-1, 1}, {0, 3}}, 5, {0xb8, 0x78, 0x3e, 0xd0, 0xc2}, 18, 17},
    {16, 16, 0xF, 4, {{0, 0}, {0, 0}, {0, 0}, {0, 0}}, 1, {0x80}, 9, 0},
    {16, 16, 1, 1, {{0, 0}}, 0, {}, 3, 0},
};

static void truth(const std::string &what, bool ok) { expect(SHARED, what, ok ? nullptr : "differs from the header's value", false); }

// pack-form words of a true difference: q = d with P = 0 where d fits int16, otherwise q at the end of int16 on d's side
static void words_of(int d, uint16_t *q, uint16_t *low)
{
    const int v = d > 32767 ? 32767 : d < -32768 ? -32768 : d;
    *q = (uint16_t)v;
    *low = (uint16_t)d;
}

static void fresh(uint16_t *ctx, uint16_t p = 1024)
{
    for (unsigned i = 0; i < kEntropyMotionContexts; ++i) ctx[i] = p;
}

static void shared_syntax()
{
    uint16_t ctx[kEntropyMotionContexts];
    for (int c = 0; c < 7; ++c) {
        const Worked &v = WORKED[c];
        const std::string what = "worked value " + std::to_string(c);
        const MotionCtu g = motion_ctu(v.w / 8, v.h / 8, 0);
        truth(what + ": the mask is well formed", motion_mask_well_formed(g, v.mask));
        std::vector<uint16_t> words(4 * v.parts);
        for (int j = 0; j < v.parts; ++j) {
            words_of(v.d[j][0], &words[4 * j], &words[4 * j + 2]);
            words_of(v.d[j][1], &words[4 * j + 1], &words[4 * j + 3]);
            truth(what + ": the true difference", entropy_motion_true_diff(words[4 * j], words[4 * j + 2]) == v.d[j][0] &&
                                                      entropy_motion_true_diff(words[4 * j + 1], words[4 * j + 3]) == v.d[j][1]);
        }
        std::vector<uint8_t> out(kEntropyMotionMaxBytes);
        EntropyEnc e;
        fresh(ctx);
        entropy_enc_start(e, out.data(), (uint32_t)out.size());
        entropy_motion_encode_ctu(e, g, v.mask, words.data(), ctx);
        const uint32_t n_bytes = entropy_enc_finish(e);
        truth(what + ": bins", e.ctx_bins == v.ctx_bins && e.bypass_bins == v.bypass_bins);
        bool same = n_bytes == (uint32_t)v.n_bytes;
        for (int i = 0; same && i < v.n_bytes; ++i) same = out[i] == v.bytes[i];
        truth(what + ": bytes", same);
        fresh(ctx);
        entropy_enc_start(e, nullptr, 0);                                   // no sink: counted all the same
        entropy_motion_encode_ctu(e, g, v.mask, words.data(), ctx);
        truth(what + ": no sink", entropy_enc_finish(e) == n_bytes);
        // and back: a buffer of exactly n_bytes and exactly 4 * parts words, so that an access beyond either is a finding
        std::vector<uint8_t> exact(out.begin(), out.begin() + n_bytes);
        std::vector<uint16_t> back(4 * v.parts, 0xAAAA);
        EntropyDec d;
        EntropyMotionCtu r;
        fresh(ctx);
        entropy_dec_start(d, exact.data(), n_bytes);
        bool good = entropy_motion_decode_ctu(d, g, ctx, back.data(), &r);
        good = good && r.mask == v.mask && r.parts == (uint32_t)v.parts && r.bits == v.ctx_bins + v.bypass_bins;
        for (int j = 0; good && j < v.parts; ++j)
            good = back[4 * j] == 0 && back[4 * j + 1] == 0 && back[4 * j + 2] == (uint16_t)v.d[j][0] && back[4 * j + 3] == (uint16_t)v.d[j][1];
        truth(what + ": the round trip, and bins == bits", good);
    }
    // the worst CTU: 64 level-0 partitions, every |d| = 65535 -- the header's 511 bytes, and under the bound for the two extreme tables
    std::vector<uint16_t> words(256);
    for (int j = 0; j < 64; ++j) {
        words_of(j % 3 ? 65535 : -65535, &words[4 * j], &words[4 * j + 2]);
        words_of(j % 2 ? 65535 : -65535, &words[4 * j + 1], &words[4 * j + 3]);
    }
    const MotionCtu g = motion_ctu(8, 8, 0);
    for (uint16_t p : {(uint16_t)1024, (uint16_t)31, (uint16_t)2017}) {
        std::vector<uint8_t> out(kEntropyMotionMaxBytes);
        EntropyEnc e;
        fresh(ctx, p);
        entropy_enc_start(e, out.data(), (uint32_t)out.size());
        entropy_motion_encode_ctu(e, g, ~(uint64_t)0, words.data(), ctx);
        const uint32_t n_bytes = entropy_enc_finish(e);
        truth("the worst CTU under " + std::to_string(p), e.ctx_bins == 277 && e.bypass_bins == 3968 && n_bytes <= kEntropyMotionMaxBytes && (p != 1024 || n_bytes == 511));
        std::vector<uint8_t> exact(out.begin(), out.begin() + n_bytes);
        std::vector<uint16_t> back(256);
        EntropyDec d;
        EntropyMotionCtu r;
        fresh(ctx, p);
        entropy_dec_start(d, exact.data(), n_bytes);
        bool good = entropy_motion_decode_ctu(d, g, ctx, back.data(), &r) && r.parts == 64 && r.max_abs == 65535 && r.bits == 64 * 66 + 21;
        for (int j = 0; good && j < 64; ++j) good = back[4 * j + 2] == words[4 * j + 2] && back[4 * j + 3] == words[4 * j + 3];
        truth("the worst CTU and back under " + std::to_string(p), good);
    }
    // garbage terminates inside its buffers; where every bin is a one it is malformed; no bytes are the flat CTU
    std::vector<uint8_t> ones(64, 0xFF);
    for (int w : {64, 80, 16}) {
        const MotionCtu c = motion_ctu(w / 8, 6, 0);
        std::vector<uint16_t> back(256);
        EntropyDec d;
        EntropyMotionCtu r, flat;
        fresh(ctx);
        entropy_dec_start(d, ones.data(), (uint32_t)ones.size());
        truth("0xFF bytes are malformed at width " + std::to_string(w), !entropy_motion_decode_ctu(d, c, ctx, back.data(), &r));
        entropy_motion_flat_ctu(c, ctx, back.data(), &flat);
        bool zero = motion_mask_well_formed(c, flat.mask) && flat.max_abs == 0;
        for (unsigned i = 0; zero && i < 4 * flat.parts; ++i) zero = back[i] == 0;
        std::vector<uint16_t> none(4 * flat.parts, 0);
        EntropyEnc e;
        fresh(ctx, 777);
        entropy_enc_start(e, nullptr, 0);
        entropy_motion_encode_ctu(e, c, flat.mask, none.data(), ctx);
        truth("the flat CTU is no bytes at width " + std::to_string(w), zero && entropy_enc_finish(e) == 0 && e.bypass_bins == 0 && e.ctx_bins == flat.bits);
    }
    truth("the default table", kEntropyMotionDefault.p[0] == 1024 && kEntropyMotionDefault.p[6] == 1024);
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
    static_assert(sizeof(x266_entropy_motion_ctu_t) == 32 && offsetof(x266_entropy_motion_ctu_t, ctx_bins) == 0 && offsetof(x266_entropy_motion_ctu_t, bypass_bins) == 4 &&
                      offsetof(x266_entropy_motion_ctu_t, offset) == 8 && offsetof(x266_entropy_motion_ctu_t, n_words) == 16 &&
                      offsetof(x266_entropy_motion_ctu_t, n_bytes) == 20 && offsetof(x266_entropy_motion_ctu_t, parts) == 24 &&
                      offsetof(x266_entropy_motion_ctu_t, unreadable) == 28,
                  "the record of the header");
    static_assert(offsetof(x266_level_region_t, offset) == 8 && offsetof(x266_level_region_t, n_words) == 16, "the first 20 bytes are the level record's");
    static_assert(offsetof(x266_entropy_motion_t, init) == 48 && offsetof(x266_entropy_motion_t, width) == 56 && offsetof(x266_entropy_motion_t, in_words) == 64 &&
                      offsetof(x266_entropy_motion_t, cap_words) == 72,
                  "the struct of the header");
    static_assert(X266_ENTROPY_MOTION_CONTEXTS == 7 && X266_ENTROPY_MOTION_MAX_BYTES == 720, "the header's constants");
    std::printf("sizeof(x266_entropy_motion_ctu_t) %zu\nsizeof(x266_entropy_motion_t) %zu\n", sizeof(x266_entropy_motion_ctu_t), sizeof(x266_entropy_motion_t));
    for (int call = 0; call < 2; ++call) {
        ++g_checks;
        if (!(call == 0 ? args::entropy_motion_encode(nullptr) : args::entropy_motion_decode(nullptr)))
            ++g_failures, std::printf("FAIL a NULL parameter struct is accepted\n");
        const int sizes[4][2] = {{16, 16}, {144, 112}, {3840, 2176}, {65664, 16}};
        for (const auto &wh : sizes)
            for (uint64_t cap : {(uint64_t)4096, (uint64_t)0, (uint64_t)3})
                for (uint64_t in : {(uint64_t)1024, (uint64_t)0}) {
                    const Tuple b = placed(wh[0], wh[1], in, cap);
                    walk(call, b, std::to_string(wh[0]) + " x " + std::to_string(wh[1]) + " in " + std::to_string(in) + " cap " + std::to_string(cap) + " ");
                    if (cap == 4096 && in == 1024 && wh[0] == 144) table_sides_and_counts(call, b);
                }
    }
    reconstruct_rules();
    shared_syntax();
    std::printf("checks x266_entropy_motion_t %d\n", g_checks);
    if (g_failures) {
        std::printf("%d of %d checks FAILED\n", g_failures, g_checks);
        return 1;
    }
    std::printf("the argument rules hold (%d checks)\n", g_checks);
    return 0;
}
