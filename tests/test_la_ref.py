"""CPU: tests/_la_ref.py, the restatement of the lookahead the GPU tests compare with, against the numbers include/x266hip.h states for
every formula and against the properties that follow from the text."""
import numpy as np
import pytest

import _aq_ref as A
import _la_ref as R


# ---- 1. the box -----------------------------------------------------------------------------------------------------------------------------
def test_box_worked_numbers():
    for samples, want in (((1, 2, 3, 4), 3), ((0, 0, 0, 1), 0), ((0, 0, 1, 1), 1), ((255, 255, 255, 254), 255)):
        assert int(R.box(np.array(samples).reshape(2, 2))[0, 0]) == want, samples


@pytest.mark.parametrize("value", [0, 1, 128, 255])
def test_a_constant_frame_downsamples_to_itself_and_costs_nothing(value):
    w, h = 96, 160
    low = R.downscale(A.constant_frame(w, h, value), w, h)
    assert low.shape == (15, 512) and (low[:, :384] == value).all()
    cost, mode = R.intra_costs(low, w, h)
    if value == 128:                                                          # the corner block's 128 too
        assert not cost.any()
    assert not cost[1:].any() and not mode.any()                              # cost 0 with every candidate: the first one, planar, stays


def test_downscale_reads_u_and_v_apart_and_every_tile_once():
    w, h = 64, 32
    r = np.random.RandomState(3)
    y, u, v = r.randint(0, 256, (h, w)), r.randint(0, 256, (h // 2, w // 2)), r.randint(0, 256, (h // 2, w // 2))
    low = R.downscale(A.tiles_from_planes(y, u, v), w, h)
    ly, lu, lv = R.planes_from_tiles(low, w // 2, h // 2)
    for got, src in ((ly, y), (lu, u), (lv, v)):
        want = (src.reshape(src.shape[0] // 2, 2, src.shape[1] // 2, 2).sum((1, 3)) + 2) // 4
        assert np.array_equal(got, want)


# ---- 2. intra costs -------------------------------------------------------------------------------------------------------------------------
def test_prediction_worked_numbers():
    top, left = list(range(10, 100, 10)), list(range(100, 190, 10))
    planar, dc, hor, ver = R.predictions(top, left)
    assert (planar[0, 0], planar[5, 3], planar[7, 7]) == (65, 133, 135) and (dc == 90).all()
    assert (hor == np.array(left[:8])[:, None]).all() and (ver == np.array(top[:8])[None, :]).all()


def test_satd_worked_numbers():
    checker = (np.indices((8, 8)).sum(0) & 1)
    assert R.satd8x8(np.ones((8, 8))) == 16
    assert R.satd8x8(255 * (2 * checker - 1)) == 4080
    assert R.satd8x8(255 * checker - 128) == 2048
    assert R.satd8x8(np.zeros((8, 8))) == 0
    r = np.random.RandomState(5)
    assert max(R.satd8x8(r.choice([-255, 255], (8, 8))) for _ in range(50)) <= 32640


def test_neighbour_rules_on_the_frame_edges():
    y = np.arange(32 * 48).reshape(48, 32) % 251
    assert R.neighbours(y, 0, 0) == ([128] * 9, [128] * 9)
    top, left = R.neighbours(y, 8, 0)                                        # only y0 == 0: every top is left[0]
    assert top == [int(y[0, 7])] * 9 and left == [int(y[i, 7]) for i in range(9)]
    top, left = R.neighbours(y, 0, 8)                                        # only x0 == 0: every left is top[0]
    assert left == [int(y[7, 0])] * 9 and top == [int(y[7, i]) for i in range(9)]
    top, left = R.neighbours(y, 24, 40)                                      # the last block: TR and BL stop at the frame's last column and row
    assert top[8] == top[7] == int(y[39, 31]) and left[8] == left[7] == int(y[47, 23])
    top, left = R.neighbours(y, 16, 32)
    assert top[8] == int(y[31, 24]) and left[8] == int(y[40, 15])


def test_intra_tie_goes_to_the_first_candidate():
    w, h = 64, 64
    yy, xx = np.indices((h // 2, w // 2))
    cols = A.tiles_from_planes(np.repeat(np.repeat(xx * 7 % 256, 2, 0), 2, 1), np.zeros((h // 2, w // 2)), np.zeros((h // 2, w // 2)))
    rows = A.tiles_from_planes(np.repeat(np.repeat(yy * 7 % 256, 2, 0), 2, 1), np.zeros((h // 2, w // 2)), np.zeros((h // 2, w // 2)))
    cost, mode = R.intra_costs(R.downscale(cols, w, h), w, h)
    assert mode[5] == 26 and cost[5] == 0                                    # columns: vertical is exact, nothing earlier is
    cost, mode = R.intra_costs(R.downscale(rows, w, h), w, h)
    assert mode[5] == 10 and cost[5] == 0
    y = np.full((32, 32), 77)
    c = R.block_costs(y, 8, 8)
    assert c == [0, 0, 0, 0] and R.intra_costs(R.downscale(A.constant_frame(64, 64, 77), 64, 64), 64, 64)[1][5] == 0


# ---- 3. frame cost --------------------------------------------------------------------------------------------------------------------------
def _me(costs, mv=(3, -2)):
    a = np.zeros(len(costs), R.ME_DTYPE)
    a["cost"], a["mvx"], a["mvy"] = costs, mv[0], mv[1]
    return a


def test_frame_cost_worked_ties():
    intra, mode = np.array([400, 400, 399, 400], np.uint32), np.array([26, 10, 1, 0], np.uint8)
    l0, l1 = _me([500, 500, 500, 500]), _me([500, 499, 500, 400], (-7, 9))
    rec, tot = R.frame_cost(intra, mode, l0, l1, 100)
    assert rec["kind"].tolist() == [1, 2, 0, 2] and rec["cost"].tolist() == [500, 499, 499, 400]
    assert rec["mvx"].tolist() == [3, -7, 0, -7] and rec["mvy"].tolist() == [-2, 9, 0, 9]
    assert rec["mode"].tolist() == [26, 10, 1, 0] and rec["intra"].tolist() == intra.tolist() and not rec["reserved"].any()
    assert tot.tolist() == [1898, 1599, 1, 1, 2, 2000, 1899, 4]
    rec, tot = R.frame_cost(intra, None, None, None, 100)                    # an I frame: the penalty is in the cost, not in intra
    assert rec["kind"].tolist() == [0] * 4 and rec["cost"].tolist() == [500, 500, 499, 500] and not rec["mode"].any()
    assert tot.tolist() == [1999, 1599, 4, 0, 0, 0, 0, 4]
    rec, tot = R.frame_cost(intra, mode, None, l1, 0)                        # one list, and it is list 1; equal cost stays with the list
    assert rec["kind"].tolist() == [0, 0, 0, 2] and tot[5] == 0 and tot[6] == 1899


def test_scene_cut_worked_numbers():
    assert [R.scene_cut_bias(102, g, 25, 250) for g in (5, 10, 100)] == [1632, 2611, 13056]
    assert R.scene_cut_bias(102, 30, 25, 25) == 26112 and R.scene_cut_bias(102, 6, 25, 250) == 1632 and R.scene_cut_bias(102, 7, 25, 250) == 1827
    assert R.scene_cut_bias(102, 25, 25, 250) == 6528 and R.scene_cut_bias(102, 250, 25, 250) == 26112
    tot = lambda p, i: [p, i, 0, 0, 0, 0, 0, 60]
    assert R.scene_cut(tot(90000, 100000), 102, 100, 25, 250) == 1 and R.scene_cut(tot(80000, 100000), 102, 100, 25, 250) == 0
    assert R.scene_cut(tot(80080, 100000), 102, 100, 25, 250) == 1 and R.scene_cut(tot(80078, 100000), 102, 100, 25, 250) == 0   # 52480 / 65536
    assert R.scene_cut(tot(0, 0), 0, 0, 1, 1) == 1
    assert R.scene_cut(None, 102, 100, 25, 250) == -1 and R.scene_cut(tot(-1, 5), 102, 100, 25, 250) == -1
    assert R.scene_cut(tot(1, 1), 257, 100, 25, 250) == -1 and R.scene_cut(tot(1, 1), 102, 100, 25, 24) == -1


# ---- 5. propagate ---------------------------------------------------------------------------------------------------------------------------
def test_propagate_worked_numbers():
    assert R.amount(600, 1000, 5000) == 2400 and R.amount(1200, 1000, 5000) == 0
    assert R.amount(0, 1000, 2 ** 40) == 1000 + 2 ** 32 - 1                  # d_prop is held to 2^32 - 1
    t = R.targets(1, 3, -11, 5)                                              # px = -3: floor division, dx = 5
    assert t == [(-1, 3, 9), (0, 3, 15), (-1, 4, 15), (0, 4, 25)]
    assert [(2400 * w + 32) >> 6 for _, _, w in t] == [338, 563, 563, 938]
    rec = np.zeros(60, R.BLOCK_DTYPE)                                        # 160 x 96: 10 x 6 blocks
    rec[31] = (600, 1000, -11, 5, 1, 0, 0)
    prop = np.zeros(60, np.uint64)
    prop[31] = 5000
    ref0, ref1 = R.propagate(rec, prop, np.zeros(60, np.uint64), np.zeros(60, np.uint64), 160, 96)
    want = np.zeros(60, np.uint64)
    want[30], want[40] = 563, 938                                            # (0, 3) and (0, 4); the two at X = -1 are dropped
    assert np.array_equal(ref0, want) and not ref1.any()
    rec["kind"][31] = 2
    ref0, ref1 = R.propagate(rec, prop, None, want.copy(), 160, 96)          # a NULL target; the other one is added INTO
    assert ref0 is None and np.array_equal(ref1, 2 * want)
    for skip in (dict(kind=0), dict(intra=0)):
        one = rec.copy()
        for k, v in skip.items():
            one[k][31] = v
        assert not any(a.any() for a in R.propagate(one, prop, np.zeros(60, np.uint64), np.zeros(60, np.uint64), 160, 96))


def test_what_a_block_hands_on_is_its_amount_within_two():
    """four targets inside the grid, each rounded by less than 1/2: the shares add up to amount - 2 .. amount + 2"""
    r = np.random.RandomState(11)
    for _ in range(500):
        intra, cost, prop = int(r.randint(1, 40000)), int(r.randint(0, 40000)), int(r.randint(0, 1 << 34))
        a = R.amount(cost, intra, prop)
        mvx, mvy = int(r.randint(-64, 65)), int(r.randint(-64, 65))
        t = R.targets(20, 20, mvx, mvy)
        assert sum(w for _, _, w in t) == 64 and all(0 <= X < 40 and 0 <= Y < 40 for X, Y, _ in t)
        handed = sum((a * w + 32) >> 6 for _, _, w in t if w > 0)
        assert a - 2 <= handed <= a + 2, (a, handed, mvx, mvy)
        if mvx % 8 == 0 and mvy % 8 == 0:
            assert handed == a


# ---- 6. tree qp -----------------------------------------------------------------------------------------------------------------------------
def test_gain_worked_numbers_and_monotone():
    assert int(A.log2_q8(1000)) == 2551 and int(A.log2_q8(4000)) == 3063
    assert R.gain(1000, 3000, 512) == 1024 and R.gain(1000, 3000, 1024) == 2048 and R.gain(1000, 0, 512) == 0
    assert R.gain(1, 2 ** 40, 1024) == 32764 and R.gain(0, 2 ** 40, 1024) == 0
    r = np.random.RandomState(13)
    for _ in range(60):
        intra, strength = int(r.randint(1, 70000)), int(r.randint(0, 1025))
        props = np.sort(np.concatenate([r.randint(0, 1 << 20, 20), r.randint(0, 1 << 40, 20), [0, 2 ** 32 - 1 - intra, 2 ** 32, 2 ** 63]]).astype(np.uint64))
        gains = [R.gain(intra, p, strength) for p in props]
        assert gains[0] == 0 and all(a <= b for a, b in zip(gains, gains[1:])) and min(gains) >= 0


def test_tree_qp_without_propagation_is_the_source_analysis_decision():
    """d_prop zero and an AQ offset given: the bytes are those of tests/_aq_ref.py's decide for the same offsets"""
    for w, h in ((96, 160), (160, 96), (64, 64)):
        tiles, _ = A.halves_frame(w, h, 0xB0 + w + h), None
        rec = A.tile_stats(tiles)
        for mode, strength, qp, chroma in ((1, 256, 30, 0), (2, 1024, 51, 12), (2, 700, 0, -12)):
            off, qps = A.decide(rec, A.totals(rec), w, h, mode, strength, qp, chroma)
            blocks = np.zeros(rec.size, R.BLOCK_DTYPE)
            blocks["intra"] = np.random.RandomState(w).randint(0, 5000, rec.size)
            for prop in (None, np.zeros(rec.size, np.uint64)):
                got_off, got_qp = R.tree_qp(blocks, prop, off, w, h, 512, qp, chroma)
                assert np.array_equal(got_off, off) and np.array_equal(got_qp, qps)


def test_tree_qp_clamps_from_both_sides():
    blocks = np.zeros(4, R.BLOCK_DTYPE)
    blocks["intra"] = [1, 1, 1000, 0]
    prop = np.array([2 ** 40, 0, 3000, 2 ** 40], np.uint64)
    off, qp = R.tree_qp(blocks, prop, np.array([0, 3072, 100, -3072], np.int16), 32, 32, 1024, 30, 2)
    assert off.tolist() == [-3072, 3072, 100 - 2048, -3072]
    assert qp.tolist() == [30 + A.delta(int(off.sum()), 4)] + [30] * 3 + [32 + A.delta(int(off.sum()), 4)] * 2
