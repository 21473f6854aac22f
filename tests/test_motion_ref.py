"""CPU: the reference of the compact motion stream (tests/_motion_ref.py) against the header's worked values and against the properties the
contract rests on, over random quadtrees at the shapes the device tests run, cut CTUs included; the conditions the device tests' fixtures
must meet, asserted here on the reference; and the three host helpers of the built library (xMotionWalk, xMotionPredictor,
xMotionVectorBits) against the reference.  No GPU."""
import functools

import numpy as np
import pytest

import _motion_ref as M
import _partition_ref as PR
import _seeded_ref as S

SMALL = M.SIZES[:5]                                                         # 65664 x 16 is 1026 times the CTU of 1104 x 16: once is enough
TREES = [(w, h, seed) for w, h in SMALL for seed in range(12)]


@functools.lru_cache(None)
def packed(w, h, seed):
    mv, level = M.random_tree(w, h, seed)
    return mv, level, M.pack(mv, level, w, h)


# ---- the header's worked values ------------------------------------------------------------------------------------------------------------
def test_morton_map():
    assert [M.unmorton(i) for i in range(5)] == [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0)]
    assert M.morton(7, 7) == 63 and M.morton(2, 1) == 6 and M.morton(0, 2) == 8 and M.morton(2, 2) == 12
    assert sorted(M.morton(x, y) for x in range(8) for y in range(8)) == list(range(64))
    assert all(M.morton(*M.unmorton(i)) == i for i in range(64))


def test_worked_values_of_the_header():
    """a 32 x 32 frame that is all level 1, and the level-0 block (1, 1)"""
    w = h = 32
    level = np.ones(16, np.uint8)
    mv = np.arange(32, dtype=np.int16).reshape(16, 2)
    r = M.pack(mv, level, w, h)
    assert [p[1] for p in r["parts"]] == [0, 4, 8, 12] and [(p[2], p[3]) for p in r["parts"]] == [(0, 0), (2, 0), (0, 2), (2, 2)]
    assert int(r["ctu"]["head_mask"][0]) == 0x1111 and r["ctu"]["parts"][0] == 4 and r["ctu"]["n_words"][0] == 16
    spots, why = M.predictor_spots(4, 4, 0, 2, 2)
    assert why == "right" and spots == [None, (0, 1), (2, 1)] and M.morton(2, 1) == 6 < 8
    spots, why = M.predictor_spots(4, 4, 2, 2, 2)
    assert why == "outside" and spots[2] == (1, 1)
    spots, why = M.predictor_spots(4, 4, 1, 1, 1)
    assert why == "not yet coded" and spots == [(0, 1), (1, 0), (0, 0)] and M.morton(1, 1) == 3 < M.morton(2, 0) == 4
    fin = PR.field_in(mv, w, h)
    assert PR.predictor(fin, 1, 1, 1) != M.predictor(fin, 1, 1, 1)          # the decision's own predictor used in(2, 0) there


def test_code_length():
    assert [M.code_length(d) for d in (0, 1, -1, 2, -2, 3, 65535, -65535)] == [1, 3, 3, 5, 5, 5, 33, 33]
    for d in list(range(-70, 71)) + [16382, -16382]:
        assert M.code_length(d) == S.code_length(d), d                      # L is the seeded search's


# ---- the properties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,seed", TREES)
def test_coding_order_is_ascending_morton_and_the_mask_gives_the_levels_back(w, h, seed):
    bw, bh, cw, ch = M.grid(w, h)
    mv, level, r = packed(w, h, seed)
    for c in range(cw * ch):
        mine = [p for p in r["parts"] if p[0] == c]
        heads = [p[1] for p in mine]
        assert heads == sorted(heads) and len(set(heads)) == len(heads) and heads[0] == 0
        mask = int(r["ctu"]["head_mask"][c])
        assert mask == sum(1 << i for i in heads) and M.well_formed(bw, bh, c % cw, c // cw, mask)
        for p in mine:
            assert M.level_from_mask(bw, bh, c % cw, c // cw, mask, p[1]) == p[4], p
    assert sum(4 ** p[4] for p in r["parts"]) == bw * bh                    # the partitions tile the frame


@pytest.mark.parametrize("w,h,seed", TREES)
def test_a_b_and_above_left_precede(w, h, seed):
    bw, bh, _, _ = M.grid(w, h)
    _, _, r = packed(w, h, seed)
    for _, _, X, Y, k, _, _, _, why in r["parts"]:
        here = M.coding_position(bw, X, Y)
        for bx, by in ((X - 1, Y), (X, Y - 1), (X - 1, Y - 1)):
            if bx >= 0 and by >= 0:
                assert M.coding_position(bw, bx, by) < here, (X, Y, k, bx, by)
        if why == "right":
            assert M.coding_position(bw, X + (1 << k), Y - 1) < here


@pytest.mark.parametrize("w,h,seed", TREES)
def test_unpack_inverts_pack_and_the_differences_decode(w, h, seed):
    mv, level, r = packed(w, h, seed)
    got_mv, got_level = M.unpack(r["ctu"], r["stream"], w, h)
    assert np.array_equal(got_mv, mv) and np.array_equal(got_level, level)
    assert np.array_equal(r["mv"], mv) and np.array_equal(r["level"], level)               # a consistent field is its own canonical form
    assert np.array_equal(M.decode_differences(r["ctu"], r["stream"], w, h), mv)
    assert r["ctu"]["offset"].tolist() == [4 * sum(1 for p in r["parts"] if p[0] < c) for c in range(len(r["ctu"]))]
    assert (r["ctu"]["n_words"] == 4 * r["ctu"]["parts"]).all() and r["total"].tolist() == [4 * len(r["parts"]), len(r["ctu"])]


@pytest.mark.parametrize("w,h", SMALL)
def test_an_inconsistent_field_packs_to_its_canonical_form(w, h):
    mv, level = M.inconsistent_field(w, h, 5)
    r = M.pack(mv, level, w, h)
    again = M.pack(r["mv"], r["level"], w, h)
    assert np.array_equal(again["ctu"]["head_mask"], r["ctu"]["head_mask"]) and np.array_equal(again["stream"][0::4], r["stream"][0::4])
    got_mv, got_level = M.unpack(r["ctu"], r["stream"], w, h)
    assert np.array_equal(got_mv, r["mv"]) and np.array_equal(got_level, r["level"])
    if (w, h) != (16, 16):
        assert (level > 3).any() and not np.array_equal(level & 3, r["level"])


def test_malformed_masks():
    bw, bh = 10, 6                                                          # 80 x 48: CTU 0 is cut at the bottom, CTU 1 at the right too
    good = int(M.pack(*M.random_tree(80, 48, 1), 80, 48)["ctu"]["head_mask"][0])
    assert M.well_formed(bw, bh, 0, 0, good)
    assert not M.well_formed(bw, bh, 0, 0, good & ~1)                       # bit 0 clear
    assert not M.well_formed(bw, bh, 0, 0, good | 1 << 63)                  # block (7, 7) does not exist: bh = 6
    assert not M.well_formed(18, 14, 0, 0, 0b101)                           # heads {0, 2}: block 1 is covered by nobody
    assert M.well_formed(18, 14, 0, 0, 1) and M.level_from_mask(18, 14, 0, 0, 1, 0) == 3
    assert not M.well_formed(bw, bh, 0, 0, 1)                               # ... but a cut CTU is no partition
    assert M.well_formed(18, 14, 0, 0, 0x1111111111111111) and not M.well_formed(18, 14, 0, 0, 0x1111111111111101)


# ---- the conditions of the device tests' fixtures, on the reference --------------------------------------------------------------------------
def test_the_fixture_of_144x112_meets_its_conditions():
    w, h = 144, 112
    bw = w // 8
    mv, level = M.field(w, h)
    r = M.pack(mv, level, w, h)
    assert (np.bincount(level, minlength=4) > 0).all()
    assert r["ctu"]["max_abs"].max() == 65535 and any(M.code_length(c) == 33 for p in r["parts"] for c in p[7])
    assert any(why == "right" and (Y - 1) >> 3 < Y >> 3 and (X + (1 << k)) >> 3 > X >> 3 for _, _, X, Y, k, _, _, _, why in r["parts"])   # C in the CTU above-right
    assert any(why == "not yet coded" for p in r["parts"] for why in (p[8],))
    assert {-32768, 32767} <= set(mv.ravel().tolist())
    assert len(r["ctu"]) == 6 and M.grid(w, h)[2:] == (3, 2) and bw == 18


def test_the_long_row_crosses_the_scans_step():
    import x266_amd
    w, h = M.SIZES[-1]
    assert M.grid(w, h)[2] * M.grid(w, h)[3] == 1026 > x266_amd.levels_scan_chunk() == 1024


# ---- the host helpers of the built library ------------------------------------------------------------------------------------------------------
def test_the_walk_helper_follows_the_reference():
    import x266_amd.motion as X
    from x266_amd import X266Error
    for w, h, seed in TREES[::3]:
        bw, bh, cw, ch = M.grid(w, h)
        _, _, r = packed(w, h, seed)
        for c in range(cw * ch):
            heads, levels = X.motion_walk(w, h, c, int(r["ctu"]["head_mask"][c]))
            assert list(zip(heads.tolist(), levels.tolist())) == [(p[1], p[4]) for p in r["parts"] if p[0] == c]
    rs = np.random.RandomState(9)
    verdicts = set()
    for w, h in SMALL[1:4]:
        bw, bh, cw, ch = M.grid(w, h)
        for _ in range(300):
            c = int(rs.randint(cw * ch))
            base = int(M.pack(*M.random_tree(w, h, int(rs.randint(1 << 30))), w, h)["ctu"]["head_mask"][c])
            mask = base ^ (1 << int(rs.randint(64))) if rs.randint(2) else base ^ (1 << int(rs.randint(64))) ^ (1 << int(rs.randint(64)))
            ok = M.well_formed(bw, bh, c % cw, c // cw, mask)
            verdicts.add(ok)
            if ok:
                heads, levels = X.motion_walk(w, h, c, mask)
                assert levels.tolist() == [M.level_from_mask(bw, bh, c % cw, c // cw, mask, i) for i in heads.tolist()]
            else:
                with pytest.raises(X266Error):
                    X.motion_walk(w, h, c, mask)
    assert verdicts == {True, False}
    for bad in ((24, 16, 0, 1), (16, 16, 1, 1), (0, 16, 0, 1)):              # a bad side, a CTU the frame does not have
        with pytest.raises(X266Error):
            X.motion_walk(*bad)


def test_the_predictor_helper_follows_the_reference():
    import x266_amd.motion as X
    from x266_amd import X266Error
    for w, h, seed in TREES[::3]:
        mv, _, r = packed(w, h, seed)
        for _, _, Xb, Yb, k, _, p, _, _ in r["parts"]:
            assert X.motion_predictor(w, h, mv, Xb, Yb, k) == p, (w, h, Xb, Yb, k)
    mv = packed(80, 48, 0)[0]
    for bad in ((1, 0, 1), (0, 0, 3), (8, 0, 2), (0, 4, 2), (10, 0, 0), (0, 6, 0), (-1, 0, 0), (0, 0, 4), (0, 0, -1)):   # unaligned, cut, outside, no level
        with pytest.raises(X266Error):
            X.motion_predictor(80, 48, mv, *bad)
    assert X.motion_predictor(80, 48, mv, 4, 0, 2) == M.predictor(mv.reshape(6, 10, 2).astype(np.int64), 4, 0, 4)


def test_the_vector_bits_helper_follows_the_reference():
    import x266_amd.motion as X
    for d in list(range(-300, 301)) + [32767, -32768, 65534, 65535, -65535]:
        assert X.motion_vector_bits(d) == M.code_length(d), d
    assert [X.motion_vector_bits(d) for d in (65536, -65536, 2 ** 31 - 1, -2 ** 31)] == [-1] * 4
