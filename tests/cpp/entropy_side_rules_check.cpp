// CPU check of the argument rules of xEntropyEncodeSideGpu and xEntropyDecodeSideGpu (x266_amd/csrc/x266_args.hpp: entropy_side_encode,
// entropy_side_decode), the calls whose device pointers are the fields of the host-read x266_entropy_side_t, and of the syntax the kernels
// share with the host through x266_amd/csrc/x266_entropy_side.hpp, run here as plain C++ against the worked values of include/x266hip.h
// (tests/test_entropy_side_ref.py holds the same values against tests/_entropy_side_ref.py).  The contract is written down once more by hand
// from the header -- per call the pointer fields in struct order with their alignments, which are written, which may be NULL, their
// extents -- and one walk perturbs a base tuple one field at a time: NULL, half an alignment, one alignment further, the top of the address
// space, every overlap of an output with any other buffer, a NULL d_stream with and without a capacity, d_kind without d_mode, an entry of
// init at 30 and at 2018, qp at -1 and 52, chroma_qp_offset at -13 and 13.
// The addresses are made-up integers, nothing is dereferenced but the host table, no device is needed; the expected verdict of every
// check follows from these tables and from literals, never from the function under test.
// Test infrastructure; built and run by tests/test_entropy_side_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <climits>
#include <cstddef>
#include <string>
#include <vector>

#include "rules_expect.hpp"
#include "x266_args.hpp"
#include "x266_entropy_side.hpp"

using namespace x266;

static const char *SHARED = "x266_entropy_side.hpp";
enum { KIND, MODE, CLASS, QP, NNZ, CODED, STREAM, TOTAL, STATUS, N_FIELDS };
struct Field {
    const char *name;
    unsigned align;
    bool used[2], output[2], optional;                                      // per call: encode, decode
};
static const Field FIELDS[N_FIELDS] = {{"d_kind", 1, {true, true}, {false, true}, true},     {"d_mode", 1, {true, true}, {false, true}, true},
                                       {"d_class", 1, {true, true}, {false, true}, true},    {"d_qp", 1, {true, true}, {false, true}, true},
                                       {"d_nnz", 4, {true, true}, {false, true}, true},      {"d_coded", 8, {true, true}, {true, false}, false},
                                       {"d_stream", 16, {true, true}, {true, false}, false}, {"d_total", 8, {true, false}, {true, false}, false},
                                       {"d_status", 1, {false, true}, {false, true}, true}};
static const char *CALLS[2] = {"xEntropyEncodeSideGpu", "xEntropyDecodeSideGpu"};
struct Tuple {
    U p[N_FIELDS];
    const uint16_t *init;
    size_t n;
    uint64_t cap;
    int qp, off;
};

static size_t words2(uint64_t n) { return n > SIZE_MAX / 2 ? SIZE_MAX : (size_t)n * 2; }
static size_t extent(int f, const Tuple &t)
{
    if (f <= QP) return t.n * 6;
    if (f == NNZ) return t.n * 24;
    if (f == CODED) return t.n * 32;
    if (f == STREAM) return words2(t.cap);
    if (f == TOTAL) return 16;
    return t.n;
}
static const char *rule(int call, const Tuple &t)
{
    x266_entropy_side_t s = {};
    s.d_kind = (uint8_t *)t.p[KIND];
    s.d_mode = (uint8_t *)t.p[MODE];
    s.d_class = (uint8_t *)t.p[CLASS];
    s.d_qp = (uint8_t *)t.p[QP];
    s.d_nnz = (uint32_t *)t.p[NNZ];
    s.d_coded = (x266_entropy_side_ctu_t *)t.p[CODED];
    s.d_stream = (uint16_t *)t.p[STREAM];
    s.d_total = (uint64_t *)t.p[TOTAL];
    s.d_status = (uint8_t *)t.p[STATUS];
    s.init = t.init;
    s.n_ctu = t.n;
    s.cap_words = t.cap;
    s.qp = t.qp;
    s.chroma_qp_offset = t.off;
    return call == 0 ? args::entropy_side_encode(&s) : args::entropy_side_decode(&s);
}
// every pointer in a region of its own, at exactly its alignment times an odd number
static Tuple placed(size_t n, uint64_t cap)
{
    Tuple t = {};
    for (int i = 0; i < N_FIELDS; ++i) t.p[i] = ((U)(i + 1) << 44) + (U)FIELDS[i].align * (2 * i + 1);
    t.n = n;
    t.cap = cap;
    t.qp = 32;
    t.off = -3;
    return t;
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
        const size_t bytes = extent(f, b);
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
        if (f == MODE && call == 0) expect(CALL, name + " NULL with d_kind present", rule(call, t), true, args::kEntropySideModes);
        else expect(CALL, name + " NULL", rule(call, t), !(FIELDS[f].optional || (f == STREAM && b.cap == 0)), args::kNull);
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

static void table_scalars_and_counts(int call, const Tuple &b)
{
    const char *CALL = CALLS[call];
    uint16_t table[X266_ENTROPY_SIDE_CONTEXTS];
    for (unsigned i = 0; i < X266_ENTROPY_SIDE_CONTEXTS; ++i) table[i] = (uint16_t)(31 + (i * 1986u) / 15u);       // 31 .. 2017, both ends taken
    Tuple t = b;
    t.init = table;
    expect(CALL, "a table over the whole interval", rule(call, t), table[15] != 2017, args::kEntropyInit);
    for (unsigned at : {0u, 3u, 9u, 15u}) {
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
    range(CALL, "qp", 0, 51, [&](int v) {
        Tuple u = b;
        u.qp = v;
        return rule(call, u);
    }, args::kEntropySideScalars);
    range(CALL, "chroma_qp_offset", -12, 12, [&](int v) {
        Tuple u = b;
        u.off = v;
        return rule(call, u);
    }, args::kEntropySideScalars);
    for (int v : {INT_MIN, INT_MAX}) {
        t = b;
        t.qp = v;
        expect(CALL, "qp " + std::to_string(v), rule(call, t), true, args::kEntropySideScalars);
        t = b;
        t.off = v;
        expect(CALL, "chroma_qp_offset " + std::to_string(v), rule(call, t), true, args::kEntropySideScalars);
    }
    t = b;                                                                  // kinds need modes, on encode only; modes alone are fine
    t.p[MODE] = 0;
    expect(CALL, "d_mode NULL with d_kind present", rule(call, t), call == 0, args::kEntropySideModes);
    t.p[KIND] = 0;
    expect(CALL, "d_mode and d_kind NULL", rule(call, t), false);
    t = b;
    t.p[KIND] = 0;
    expect(CALL, "d_kind NULL with d_mode present", rule(call, t), false);
    t = b;                                                                  // every array NULL
    for (int f = KIND; f <= NNZ; ++f) t.p[f] = 0;
    t.p[STATUS] = 0;
    expect(CALL, "every optional array NULL", rule(call, t), false);
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
    t.n = SIZE_MAX / 4;                                                     // 6, 24 and 32 bytes per CTU all saturate
    expect(CALL, "n_ctu 2^62 - 1", rule(call, t), true, args::kNoFit);
    t = b;                                                                  // no CTU: only the scalars, the table and d_total of encode
    t.n = 0;
    for (int f = 0; f < N_FIELDS; ++f)
        if (f != TOTAL) t.p[f] = 0;
    expect(CALL, "n_ctu 0 with every buffer NULL", rule(call, t), false);
    t.p[TOTAL] = 0;
    expect(CALL, "n_ctu 0 without d_total", rule(call, t), call == 0, args::kNull);
    t = b;
    t.n = 0;
    t.qp = 52;
    expect(CALL, "n_ctu 0 with qp 52", rule(call, t), true, args::kEntropySideScalars);
}

// ---- the syntax against the header's worked values ------------------------------------------------------------------------------------------
struct Worked {
    bool kinds, classes, qps, flags;                                        // which arrays are given
    uint8_t kind[6], mode[6], cls[6], qp_in[6];
    uint32_t nnz[6];
    int qp, n_bytes, bytes[3];
    unsigned ctx_bins, bypass_bins;
};
static const Worked WORKED[8] = {
    {true, false, false, true, {0, 0, 0, 0, 0, 0}, {9, 9, 9, 9, 9, 9}, {}, {}, {0, 0, 0, 0, 0, 0}, 32, 0, {}, 11, 0},
    {true, false, false, true, {1, 0, 0, 0, 0, 0}, {26, 26, 26, 26, 26, 26}, {}, {}, {0, 0, 0, 0, 0, 0}, 32, 1, {0xf0}, 12, 2},
    {true, false, false, true, {1, 0, 0, 0, 0, 0}, {10, 10, 10, 10, 10, 10}, {}, {}, {0, 0, 0, 0, 0, 0}, 32, 3, {0x8f, 0xff, 0xfc}, 12, 5},
    {true, false, false, true, {0, 0, 0, 0, 1, 0}, {34, 34, 34, 34, 34, 34}, {}, {}, {0, 0, 0, 0, 0, 0}, 32, 3, {0x01, 0x0c, 0x0e}, 12, 5},
    {false, true, false, true, {}, {}, {0, 14, 3, 3, 3, 3}, {}, {1, 1, 0, 0, 0, 0}, 32, 3, {0x78, 0xdf, 0xae}, 22, 0},
    {false, false, true, true, {}, {}, {}, {33, 32, 32, 32, 32, 32}, {1, 0, 0, 0, 0, 0}, 32, 1, {0x50}, 14, 1},
    {false, false, true, true, {}, {}, {}, {0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0}, 51, 3, {0x5f, 0xd2, 0x7c}, 14, 12},
    {false, false, false, false, {}, {}, {}, {}, {}, 32, 3, {0x44, 0x4d, 0x5a}, 23, 0},
};

static void truth(const std::string &what, bool ok) { expect(SHARED, what, ok ? nullptr : "differs from the header's value", false); }

static void fresh(uint16_t *ctx, unsigned stride, uint16_t p = 1024)
{
    for (unsigned i = 0; i < kEntropySideContexts; ++i) ctx[i * stride] = p;
}

static bool same_ctu(const EntropySideCtu &a, const EntropySideCtu &b)
{
    return a.mode == b.mode && a.qp == b.qp && a.cls == b.cls && a.kind == b.kind && a.coded == b.coded;
}

// encode s at the stride, hold bytes and bins, decode from a buffer of exactly n_bytes, encode what came back
static uint32_t there_and_back(const std::string &what, const EntropySideCtu &s, int qp, int off, uint16_t p, unsigned stride, std::vector<uint8_t> *bytes, unsigned bins[2])
{
    std::vector<uint16_t> ctx(kEntropySideContexts * stride, 0xAAAA);
    std::vector<uint8_t> out(kEntropySideMaxBytes);
    EntropyEnc e;
    fresh(ctx.data(), stride, p);
    entropy_enc_start(e, out.data(), (uint32_t)out.size());
    entropy_side_encode_ctu(e, s, ctx.data(), stride, qp, off);
    const uint32_t n_bytes = entropy_enc_finish(e);
    truth(what + ": within the bound", n_bytes <= kEntropySideMaxBytes);
    bins[0] = e.ctx_bins;
    bins[1] = e.bypass_bins;
    fresh(ctx.data(), stride, p);
    entropy_enc_start(e, nullptr, 0);                                       // no sink: counted all the same
    entropy_side_encode_ctu(e, s, ctx.data(), stride, qp, off);
    truth(what + ": no sink", entropy_enc_finish(e) == n_bytes);
    std::vector<uint8_t> exact(out.begin(), out.begin() + n_bytes);         // an access beyond n_bytes is a finding
    EntropyDec d;
    EntropySideCtu back;
    fresh(ctx.data(), stride, p);
    entropy_dec_start(d, exact.data(), n_bytes);
    truth(what + ": the round trip", entropy_side_decode_ctu(d, ctx.data(), stride, qp, off, &back) && same_ctu(back, s));
    if (stride > 1) truth(what + ": the stride is kept", ctx[1] == 0xAAAA);
    *bytes = exact;
    return n_bytes;
}

static void shared_syntax()
{
    for (int c = 0; c < 8; ++c) {
        const Worked &v = WORKED[c];
        const std::string what = "worked value " + std::to_string(c);
        const EntropySideCtu s = entropy_side_canon(v.kinds ? v.kind : nullptr, v.kinds ? v.mode : nullptr, v.classes ? v.cls : nullptr, v.qps ? v.qp_in : nullptr,
                                                    v.flags ? v.nnz : nullptr, v.qp, 0);
        for (unsigned stride : {1u, 128u}) {
            std::vector<uint8_t> bytes;
            unsigned bins[2];
            const uint32_t n_bytes = there_and_back(what, s, v.qp, 0, 1024, stride, &bytes, bins);
            truth(what + ": bins", bins[0] == v.ctx_bins && bins[1] == v.bypass_bins);
            bool same = n_bytes == (uint32_t)v.n_bytes;
            for (int i = 0; same && i < v.n_bytes; ++i) same = bytes[i] == v.bytes[i];
            truth(what + ": bytes", same);
        }
    }
    // the canonical form: junk bytes, and what an uncoded region becomes
    {
        const uint8_t kind[6] = {2, 0, 255, 0, 0, 7}, mode[6] = {200, 3, 34, 35, 12, 99}, cls[6] = {0xF7, 0x13, 0xFE, 0x0B, 0x2C, 0x80}, qp_in[6] = {255, 52, 51, 7, 9, 200};
        const uint32_t nnz[6] = {0x80000000u, 0, 1, 2, 0, 0};
        const EntropySideCtu s = entropy_side_canon(kind, mode, cls, qp_in, nnz, 20, 5);
        uint8_t K[6], M[6], C[6], Q[6];
        uint32_t Z[6];
        entropy_side_store(s, K, M, C, Q, Z);
        const uint8_t eK[6] = {1, 0, 1, 0, 0, 0}, eM[6] = {34, 255, 34, 255, 255, 255}, eC[6] = {3, 3, 14, 3, 3, 3}, eQ[6] = {51, 51, 51, 7, 12, 12};
        const uint32_t eZ[6] = {1, 0, 1, 1, 0, 0};
        bool good = true;
        for (int q = 0; q < 6; ++q) good = good && K[q] == eK[q] && M[q] == eM[q] && C[q] == eC[q] && Q[q] == eQ[q] && Z[q] == eZ[q];
        truth("the canonical form of junk", good);
        std::vector<uint8_t> bytes;
        unsigned bins[2];
        there_and_back("junk", s, 20, 5, 1024, 1, &bytes, bins);
        const EntropySideCtu again = entropy_side_canon(K, M, C, Q, Z, 20, 5);
        truth("the canonical form is a fixed point", same_ctu(again, s));
    }
    // the lists
    {
        EntropySideCtu s = entropy_side_flat_ctu(30, 0);
        truth("mpm of a lone region", entropy_side_mpm(s, 0) == (0u | 1u << 8 | 26u << 16) && entropy_side_mpm(s, 3) == (0u | 1u << 8 | 26u << 16));
        s.kind = 0x7;
        s.mode = side_with_byte(side_with_byte(side_with_byte(s.mode, 0, 10), 1, 2), 2, 10);
        truth("mpm: A intra, B absent", entropy_side_mpm(s, 1) == (10u | 1u << 8 | 0u << 16));
        truth("mpm: A absent, B intra", entropy_side_mpm(s, 2) == (1u | 10u << 8 | 0u << 16));
        truth("mpm: A = 10, B = 2", entropy_side_mpm(s, 3) == (10u | 2u << 8 | 0u << 16));
        s.mode = side_with_byte(s.mode, 1, 10);
        truth("mpm: A == B == 10", entropy_side_mpm(s, 3) == (10u | 9u << 8 | 11u << 16));
        s.mode = side_with_byte(side_with_byte(s.mode, 1, 2), 2, 2);
        truth("mpm: A == B == 2", entropy_side_mpm(s, 3) == (2u | 33u << 8 | 3u << 16));
        s.mode = side_with_byte(side_with_byte(s.mode, 1, 34), 2, 34);
        truth("mpm: A == B == 34", entropy_side_mpm(s, 3) == (34u | 33u << 8 | 3u << 16));
        s.mode = side_with_byte(side_with_byte(s.mode, 1, 0), 2, 1);
        truth("mpm: A = 1, B = 0", entropy_side_mpm(s, 3) == (1u | 0u << 8 | 26u << 16));
        unsigned n = 0;
        truth("chroma list with M[0] = 10", entropy_side_chroma_list(s, &n) == (10ull | 0ull << 8 | 26ull << 16 | 1ull << 24) && n == 4);
        s.mode = side_with_byte(s.mode, 0, 7);
        truth("chroma list with M[0] = 7", entropy_side_chroma_list(s, &n) == (7ull | 0ull << 8 | 26ull << 16 | 10ull << 24 | 1ull << 32) && n == 5);
        s.kind = 0x6;
        truth("chroma list with Y0 inter", entropy_side_chroma_list(s, &n) == (0ull | 26ull << 8 | 10ull << 16 | 1ull << 24) && n == 4);
    }
    // the worst CTU that can be built: the header's sizes, and under the bound for the two extreme tables
    {
        const uint8_t kind[6] = {1, 1, 1, 1, 1, 1}, mode[6] = {34, 33, 32, 31, 33, 33}, cls[6] = {12, 12, 12, 12, 12, 12}, qp_in[6] = {51, 0, 51, 0, 51, 0};
        const EntropySideCtu s = entropy_side_canon(kind, mode, cls, qp_in, nullptr, 0, 0);
        for (uint16_t p : {(uint16_t)1024, (uint16_t)31, (uint16_t)2017}) {
            std::vector<uint8_t> bytes;
            unsigned bins[2];
            const uint32_t n_bytes = there_and_back("the worst CTU under " + std::to_string(p), s, 0, 0, p, 128, &bytes, bins);
            truth("the worst CTU's bins under " + std::to_string(p), bins[0] == 64 && bins[1] == 97 && (p != 1024 || n_bytes == 20) && (p != 2017 || n_bytes == 43));
        }
    }
    // no bytes are the flat CTU under every table, and the flat CTU is no bytes; every malformed case
    for (uint16_t p : {(uint16_t)1024, (uint16_t)31, (uint16_t)2017}) {
        uint16_t ctx[kEntropySideContexts];
        EntropyDec d;
        EntropySideCtu s;
        fresh(ctx, 1, p);
        entropy_dec_start(d, nullptr, 0);
        truth("no bytes decode to the flat CTU under " + std::to_string(p), entropy_side_decode_ctu(d, ctx, 1, 27, -12, &s) && same_ctu(s, entropy_side_flat_ctu(27, -12)) &&
                                                                                 side_byte(s.qp, 5) == 15 && side_byte(s.qp, 3) == 27);
        std::vector<uint8_t> bytes;
        unsigned bins[2];
        truth("the flat CTU is no bytes under " + std::to_string(p), there_and_back("flat", s, 27, -12, p, 1, &bytes, bins) == 0 && bins[0] == 11 && bins[1] == 0);
    }
    {
        const std::vector<uint8_t> ones(16, 0xFF);
        uint16_t ctx[kEntropySideContexts];
        EntropyDec d;
        EntropySideCtu s = entropy_side_flat_ctu(1, 0), kept = s;
        fresh(ctx, 1);
        entropy_dec_start(d, ones.data(), (uint32_t)ones.size());
        truth("0xFF bytes are malformed and leave *out alone", !entropy_side_decode_ctu(d, ctx, 1, 30, 0, &s) && same_ctu(s, kept));
    }
    truth("the default table", kEntropySideDefault.p[0] == 1024 && kEntropySideDefault.p[15] == 1024);
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
    static_assert(sizeof(x266_entropy_side_ctu_t) == 32 && offsetof(x266_entropy_side_ctu_t, ctx_bins) == 0 && offsetof(x266_entropy_side_ctu_t, bypass_bins) == 4 &&
                      offsetof(x266_entropy_side_ctu_t, offset) == 8 && offsetof(x266_entropy_side_ctu_t, n_words) == 16 && offsetof(x266_entropy_side_ctu_t, n_bytes) == 20 &&
                      offsetof(x266_entropy_side_ctu_t, n_intra) == 24 && offsetof(x266_entropy_side_ctu_t, n_coded) == 28,
                  "the record of the header");
    static_assert(offsetof(x266_level_region_t, offset) == 8 && offsetof(x266_level_region_t, n_words) == 16, "the first 20 bytes are the level record's");
    static_assert(offsetof(x266_entropy_side_t, d_nnz) == 32 && offsetof(x266_entropy_side_t, init) == 72 && offsetof(x266_entropy_side_t, n_ctu) == 80 &&
                      offsetof(x266_entropy_side_t, cap_words) == 88 && offsetof(x266_entropy_side_t, qp) == 96 && offsetof(x266_entropy_side_t, chroma_qp_offset) == 100,
                  "the struct of the header");
    static_assert(X266_ENTROPY_SIDE_CONTEXTS == 16 && X266_ENTROPY_SIDE_MAX_BYTES == 80, "the header's constants");
    // the derivation beside X266_ENTROPY_SIDE_MAX_BYTES: 64 context bins under 6.05 bits, 97 bypass bins under 1.0001, the termination, a multiple of 16
    static_assert((((64 * 605000 + 97 * 100010 + 799999) / 800000 + 4) + 15) / 16 * 16 == X266_ENTROPY_SIDE_MAX_BYTES, "the derived bound");
    std::printf("sizeof(x266_entropy_side_ctu_t) %zu\nsizeof(x266_entropy_side_t) %zu\n", sizeof(x266_entropy_side_ctu_t), sizeof(x266_entropy_side_t));
    for (int call = 0; call < 2; ++call) {
        ++g_checks;
        if (!(call == 0 ? args::entropy_side_encode(nullptr) : args::entropy_side_decode(nullptr))) ++g_failures, std::printf("FAIL a NULL parameter struct is accepted\n");
        for (size_t n : {(size_t)1, (size_t)65, (size_t)2040, (size_t)1 << 33})
            for (uint64_t cap : {(uint64_t)4096, (uint64_t)0, (uint64_t)3}) {
                const Tuple b = placed(n, cap);
                walk(call, b, "n_ctu " + std::to_string(n) + " cap " + std::to_string(cap) + " ");
                if (cap == 4096 && n == 65) table_scalars_and_counts(call, b);
            }
    }
    shared_syntax();
    std::printf("checks x266_entropy_side_t %d\n", g_checks);
    if (g_failures) {
        std::printf("%d of %d checks FAILED\n", g_failures, g_checks);
        return 1;
    }
    std::printf("the argument rules hold (%d checks)\n", g_checks);
    return 0;
}
