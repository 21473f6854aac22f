// CPU check of the argument rules of xInterPartitionDecideGpu (x266_amd/csrc/x266_args.hpp: partition_decide), the call whose device
// pointers are the fields of the host-read x266_part_t, and of the arithmetic the kernel shares with the host through
// x266_amd/csrc/x266_part.hpp: the clamps, the node geometry and the d_nodes offsets, the predictor, the rate and the walk, run here as plain
// C++ against values that tests/_partition_ref.py printed (literals below).  The contract is written down once more by hand from
// include/x266hip.h -- the pointer fields in struct order with their alignments, which are written and which may be NULL, their extents -- and
// one walk perturbs a base tuple one field at a time, with and without d_nodes: NULL, half an alignment, one alignment further, the top of
// the address space, every overlap of an output with any other buffer, the frame sizes and the scalars.  The addresses are made-up integers,
// nothing is dereferenced, no device is needed; the expected verdict of every check follows from these tables and from literals, never from
// the function under test.
// Test infrastructure; built and run by tests/test_partition_arg_rules.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <climits>
#include <string>

#include "rules_expect.hpp"
#include "x266_args.hpp"

using namespace x266;

static const char *CALL = "xInterPartitionDecideGpu";
static const char *SHARED = "x266_part.hpp";
enum { CUR, REF, MV, OUT, LEVEL, CTU, NODES, N_FIELDS };
struct Field {
    const char *name;
    unsigned align;
    bool optional, output;
};
static const Field FIELDS[N_FIELDS] = {{"d_cur", 16, false, false}, {"d_ref", 16, false, false}, {"d_mv", 8, false, false},   {"d_out", 8, false, true},
                                       {"d_level", 1, false, true}, {"d_ctu", 8, false, true},   {"d_nodes", 8, true, true}};
struct Tuple {
    U p[N_FIELDS];
    int w, h, range, lambda;
};

static size_t extent(int f, const Tuple &t)
{
    const size_t bw = (size_t)t.w / 8, bh = (size_t)t.h / 8;
    if (f == CUR || f == REF) return (size_t)t.w * (size_t)t.h * 2;
    if (f == MV || f == OUT) return 8 * bw * bh;
    if (f == LEVEL) return bw * bh;
    if (f == CTU) return 16 * (((size_t)t.w + 63) / 64) * (((size_t)t.h + 63) / 64);
    return 8 * ((bw / 2) * (bh / 2) + (bw / 4) * (bh / 4) + (bw / 8) * (bh / 8));
}
static const char *rule(const Tuple &t)
{
    x266_part_t s = {};
    s.d_cur = (const x266_ref_block_t *)t.p[CUR];
    s.d_ref = (const x266_ref_block_t *)t.p[REF];
    s.d_mv = (const x266_me_result_t *)t.p[MV];
    s.d_out = (x266_me_result_t *)t.p[OUT];
    s.d_level = (uint8_t *)t.p[LEVEL];
    s.d_ctu = (x266_part_ctu_t *)t.p[CTU];
    s.d_nodes = (x266_me_result_t *)t.p[NODES];
    s.width = t.w;
    s.height = t.h;
    s.range = t.range;
    s.lambda_q4 = t.lambda;
    return args::partition_decide(&s);
}
// every pointer in a region of its own, at exactly its alignment times an odd number
static Tuple placed(int w, int h)
{
    Tuple t = {};
    for (int i = 0; i < N_FIELDS; ++i) t.p[i] = ((U)(i + 1) << 44) + (U)FIELDS[i].align * (2 * i + 1);
    t.w = w;
    t.h = h;
    t.range = 1;
    t.lambda = 64;
    return t;
}

static void walk(const Tuple &base, bool with_nodes, const std::string &label)
{
    Tuple b = base;
    if (!with_nodes) b.p[NODES] = 0;
    const std::string at = label + (with_nodes ? "with d_nodes: " : "without d_nodes: ");
    expect(CALL, at + "base", rule(b), false);
    for (int f = 0; f < N_FIELDS; ++f) {
        if (!b.p[f]) continue;
        const unsigned align = FIELDS[f].align;
        const std::string name = at + FIELDS[f].name;
        const size_t bytes = extent(f, b);
        Tuple t = b;
        t.p[f] = 0;
        expect(CALL, name + " NULL", rule(t), !FIELDS[f].optional, args::kNull);
        if (align > 1) {
            t = b;
            t.p[f] += align / 2;
            expect(CALL, name + " at half its alignment", rule(t), true, args::kMisaligned);
        }
        t = b;
        t.p[f] += align;
        expect(CALL, name + " one alignment further", rule(t), false);
        if (bytes > align) {                                                // a 16 x 16 frame has one d_level byte per block, four in all
            t = b;
            t.p[f] = (U)0 - align;                                          // the last aligned address: the extent is larger and wraps
            expect(CALL, name + " running past the top of the address space", rule(t), true, args::kNoFit);
        }
        t = b;
        t.p[f] = down((U)0 - bytes - align, align);                         // the span ends just below the top
        expect(CALL, name + " ending just below the top", rule(t), false);
        t.p[f] = down((U)0 - bytes + align, align);                         // ... and just above it
        if (t.p[f]) expect(CALL, name + " ending just above the top", rule(t), true, args::kNoFit);   // (one record of one alignment: address 0)
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

static void sizes_and_scalars(const Tuple &b)
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
    for (auto wh : {std::pair<int, int>{16, 16}, {64, 64}, {80, 48}, {144, 112}, {1104, 16}, {1920, 1088}, {3840, 2176}, {7680, 4320}}) {
        Tuple t = placed(wh.first, wh.second);
        t.p[NODES] = b.p[NODES];
        expect(CALL, "frame " + std::to_string(wh.first) + "x" + std::to_string(wh.second), rule(t), false);
    }
    {   // the largest frame an int describes: the extents are exact (no product wraps 64 bits), and the frames no longer fit beside each other
        Tuple t = placed(INT_MAX - 15, INT_MAX - 15);
        t.p[NODES] = b.p[NODES];
        expect(CALL, "the largest frame", rule(t), true, args::kOverlap);
    }
    range(CALL, "range", 0, 1, [&](int v) { Tuple t = b; t.range = v; return rule(t); }, args::kPartScalars);
    range(CALL, "lambda_q4", 0, 65535, [&](int v) { Tuple t = b; t.lambda = v; return rule(t); }, args::kPartScalars);
    for (int bad : {INT_MIN, INT_MAX}) {
        Tuple t = b;
        t.range = bad;
        expect(CALL, "range " + std::to_string(bad), rule(t), true, args::kPartScalars);
        t = b;
        t.lambda = bad;
        expect(CALL, "lambda_q4 " + std::to_string(bad), rule(t), true, args::kPartScalars);
    }
}

// ---- the shared arithmetic against what tests/_partition_ref.py printed for a field of 6 x 4 blocks --------------------------------------
static const int FIELD[24][2] = {{57, 18}, {-6, 90}, {20000, -20000}, {-60, -4}, {-28, -27}, {-15, 22}, {6, -26}, {32767, -32768}, {24, 0}, {72, 13}, {-11, -78}, {2, -22},
                                 {-45, -9}, {-32768, 32767}, {-20, 17}, {21, 30}, {6, 54}, {19, -5}, {87, 8}, {-16, -63}, {-3, -27}, {-30, -14}, {23, 3}, {-25, 12}};
// {level, X, Y, Px, Py} of every node of levels 0..2 that exists
static const int PRED[32][5] = {{0, 0, 0, 0, 0}, {0, 1, 0, 57, 18}, {0, 2, 0, -6, 90}, {0, 3, 0, 20000, -20000}, {0, 4, 0, -60, -4}, {0, 5, 0, -28, -27}, {0, 0, 1, 0, 18},
                                {0, 1, 1, 6, -26}, {0, 2, 1, 20000, -20000}, {0, 3, 1, -28, -4}, {0, 4, 1, -15, 13}, {0, 5, 1, -15, -27}, {0, 0, 2, 6, -26}, {0, 1, 2, 24, -9},
                                {0, 2, 2, 24, 13}, {0, 3, 2, -11, 13}, {0, 4, 2, 2, -22}, {0, 5, 2, 2, -22}, {0, 0, 3, -45, 0}, {0, 1, 3, -20, 17}, {0, 2, 3, -16, 17},
                                {0, 3, 3, 6, 30}, {0, 4, 3, 6, -5}, {0, 5, 3, 19, 3}, {1, 0, 0, 0, 0}, {1, 2, 0, -6, 90}, {1, 4, 0, -60, -4}, {1, 0, 2, 6, 0}, {1, 2, 2, -11, 0},
                                {1, 4, 2, 21, 13}, {2, 0, 0, 0, 0}, {2, 4, 0, -60, -4}};
// {level, qx, qy, Px, Py, R}
static const int RATE[8][6] = {{0, 0, 0, 0, 0, 2}, {1, 6, -2, 4, -2, 7}, {0, 4, -2, 4, -2, 2}, {3, 32767, -32768, -32766, 32766, 67}, {2, -32768, 32767, 32766, -32766, 67},
                               {1, 5, 9, -7, 12, 15}, {2, -100, 33, 28, 1, 31}, {3, 1, 0, 0, 1, 7}};

static void truth(const std::string &what, bool ok) { expect(SHARED, what, ok ? nullptr : "differs from the reference's value", false); }

static void shared_arithmetic()
{
    const int bw = 6, bh = 4;
    x266_me_result_t mv[24];
    for (int b = 0; b < 24; ++b) {
        mv[b].mvx = (int16_t)FIELD[b][0];
        mv[b].mvy = (int16_t)FIELD[b][1];
        mv[b].cost = 0xDEADBEEFu;                                           // ignored
    }
    truth("clamp of 32767, -32768", part_in(mv, bw, 1, 1).x == 32766 && part_in(mv, bw, 1, 1).y == -32766 && part_in(mv, bw, 1, 2).x == -32766);
    truth("the candidate clamp", part_clamp_cand(32768) == 32767 && part_clamp_cand(-32769) == -32768 && part_clamp_cand(-32768) == -32768 && part_clamp_cand(5) == 5);
    for (const auto &p : PRED) {
        const PartVec got = part_predictor(mv, bw, p[1], p[2], 1 << p[0]);
        truth("predictor of level " + std::to_string(p[0]) + " at (" + std::to_string(p[1]) + ", " + std::to_string(p[2]) + ")", got.x == p[3] && got.y == p[4]);
        truth("... which exists", part_exists(bw, bh, p[0], p[1] >> p[0], p[2] >> p[0]));
    }
    for (const auto &r : RATE) truth("R of case " + std::to_string(&r - RATE), part_rate(r[0], r[1], r[2], PartVec{r[3], r[4]}) == (uint32_t)r[5]);
    truth("the price of bits", part_rate_cost(16, 7) == 7 && part_rate_cost(24, 7) == 10 && part_rate_cost(65535, 67) == 274427 && part_rate_cost(7, 3) == 1 &&
                                   part_rate_cost(7, 2) == 0 && part_rate_cost(0, 67) == 0);
    truth("L at the largest differences", seed_code_length(65535) == 33 && seed_code_length(-65535) == 33 && seed_code_length(0) == 1);
    // geometry: whole nodes per level and the d_nodes offsets of the shapes the device tests run
    const int shapes[5][5] = {{16, 16, 1, 0, 0}, {64, 64, 16, 4, 1}, {80, 48, 15, 2, 0}, {144, 112, 63, 12, 2}, {1104, 16, 69, 0, 0}};
    for (const auto &s : shapes) {
        const int w8 = s[0] / 8, h8 = s[1] / 8;
        bool ok = part_nodes_total(w8, h8) == (size_t)(s[2] + s[3] + s[4]) && part_nodes_offset(w8, h8, 1) == 0 && part_nodes_offset(w8, h8, 2) == (size_t)s[2] &&
                  part_nodes_offset(w8, h8, 3) == (size_t)(s[2] + s[3]);
        for (int k = 1; k < 4; ++k) ok = ok && part_whole_nodes(w8, h8, k) == (size_t)s[1 + k];
        truth("nodes of " + std::to_string(s[0]) + "x" + std::to_string(s[1]), ok);
    }
    truth("whole and cut nodes of 80x48", part_whole(10, 6, 2, 1, 0) && !part_whole(10, 6, 2, 2, 0) && !part_whole(10, 6, 2, 0, 1) && !part_whole(10, 6, 3, 0, 0) &&
                                              part_exists(10, 6, 2, 2, 1) && !part_exists(10, 6, 2, 3, 0) && part_exists(10, 6, 3, 1, 0) && !part_exists(10, 6, 3, 0, 1));
    // the walk: children TL, TR, BL, BR; dy ascending, then dx
    truth("walk lengths", part_walk_length(0) == 4 && part_walk_length(1) == 36);
    const int steps[6][4] = {{0, 0, -1, -1}, {4, 0, 0, 0}, {8, 0, 1, 1}, {9, 1, -1, -1}, {21, 2, -1, 0}, {35, 3, 1, 1}};      // {c, child, dx, dy} at r = 1
    for (const auto &s : steps) {
        const PartStep st = part_walk_step(s[0], 1);
        truth("walk step " + std::to_string(s[0]), st.child == s[1] && st.dx == s[2] && st.dy == s[3]);
    }
    for (int c = 0; c < 4; ++c) {
        const PartStep st = part_walk_step(c, 0);
        truth("walk step " + std::to_string(c) + " at r = 0", st.child == c && st.dx == 0 && st.dy == 0);
    }
}

int main()
{
    std::printf("%s:", CALL);
    for (int f = 0; f < N_FIELDS; ++f)
        std::printf("%s %s %u %s%s", f ? "," : "", FIELDS[f].name, FIELDS[f].align, FIELDS[f].optional ? "opt " : "", FIELDS[f].output ? "out" : "in");
    std::printf("\n");
    ++g_checks;
    if (!args::partition_decide(nullptr)) ++g_failures, std::printf("FAIL a NULL parameter struct is accepted\n");
    for (auto wh : {std::pair<int, int>{16, 16}, {80, 48}, {144, 112}, {1920, 1088}}) {
        const Tuple b = placed(wh.first, wh.second);
        const std::string label = std::to_string(wh.first) + "x" + std::to_string(wh.second) + " ";
        for (bool with_nodes : {true, false}) {
            walk(b, with_nodes, label);
            Tuple t = b;
            if (!with_nodes) t.p[NODES] = 0;
            sizes_and_scalars(t);
            t.p[REF] = t.p[CUR];                                            // the two frames may be one
            expect(CALL, label + "d_ref == d_cur", rule(t), false);
            t.p[REF] = t.p[CUR] + 512;                                      // ... or overlap in any other way
            expect(CALL, label + "d_ref a tile into d_cur", rule(t), false);
            t = b;
            t.p[OUT] = t.p[MV];                                             // in place is not allowed
            expect(CALL, label + "d_out == d_mv", rule(t), true, args::kOverlap);
        }
    }
    shared_arithmetic();
    std::printf("checks x266_part_t %d\n", g_checks);
    if (g_failures) {
        std::printf("%d of %d checks FAILED\n", g_failures, g_checks);
        return 1;
    }
    std::printf("the argument rules hold (%d checks)\n", g_checks);
    return 0;
}
