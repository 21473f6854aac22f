"""CPU: tests/_partition_ref.py, the numpy statement of the inter partition decision, against the header's worked values and the
consequences include/x266hip.h states; the d_nodes offsets, cut nodes and the tie rule at a merge.  No GPU."""
import functools

import numpy as np
import pytest

import _partition_ref as R
import _seeded_ref as S
import _subpel_ref as Q


@functools.lru_cache(None)
def frames(w, h):
    out = R.motion_frames(w, h, 0) + (R.motion_field(w, h, 0),)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(None)
def decided(oracle_id, w, h, lam, r):
    cur, ref, mv = frames(w, h)
    return R.decide(_ORACLES[oracle_id], cur, ref, mv, r, lam)


_ORACLES = {}


def decision(oracle, w, h, lam, r):
    _ORACLES[id(oracle)] = oracle
    return decided(id(oracle), w, h, lam, r)


def test_the_headers_worked_values():
    fin = np.zeros((4, 4, 2), np.int64)
    fin[0, 0], fin[0, 1], fin[1, 0], fin[1, 1], fin[0, 2] = (4, -8), (12, -2), (3, 5), (-7, 9), (5, 1)
    assert R.predictor(fin, 1, 0, 1) == (4, -8)                              # one neighbour inside the frame
    assert R.predictor(fin, 0, 1, 1) == (4, -2)                              # two: the third counts as (0, 0)
    assert R.predictor(fin, 1, 1, 1) == (5, 1)                               # three
    assert R.predictor(fin, 0, 0, 1) == R.predictor(fin, 0, 0, 4) == (0, 0)  # none
    moved = fin.copy()
    moved[1, 1] = (100, -100)                                                # the level-1 node at (2, 2): no block (4, 1), C = in(1, 1)
    moved[2, 1], moved[1, 2] = (100, 7), (9, -100)
    assert R.predictor(moved, 2, 2, 2) == (100, -100)
    assert R.rate(1, (6, -2), (4, -2)) == 7 and R.rate_cost(16, 7) == 7 and R.rate_cost(24, 7) == 10
    assert R.rate(0, (4, -2), (4, -2)) == 2
    assert [S.code_length(d) for d in (0, 1, -1, 2, -3, 4, 65535, -65535)] == [1, 3, 3, 5, 5, 7, 33, 33]
    assert R.rate(3, (32767, -32768), (-32766, 32766)) <= 67
    assert R.clamp_in(-32768) == -32766 and R.clamp_in(32767) == 32766 and R.clamp16(32768) == 32767 and R.clamp16(-32769) == -32768
    assert R.walk([(1, 2), (0, 0), (5, 5), (32767, -32768)], 1)[:4] == [(0, 1), (1, 1), (2, 1), (0, 2)]
    assert R.walk([(1, 2), (0, 0), (5, 5), (32767, -32768)], 1)[27:30] == [(32766, -32768), (32767, -32768), (32767, -32768)]
    assert len(R.walk([(0, 0)] * 4, 1)) == 36 and R.walk([(1, 2), (3, 4), (5, 6), (7, 8)], 0) == [(1, 2), (3, 4), (5, 6), (7, 8)]


def test_node_geometry_and_the_d_nodes_offsets():
    for (w, h), counts in (((16, 16), (1, 0, 0)), ((64, 64), (16, 4, 1)), ((80, 48), (15, 2, 0)), ((144, 112), (63, 12, 2)), ((1104, 16), (69, 0, 0))):
        bw, bh = w // 8, h // 8
        assert tuple((bw >> k) * (bh >> k) for k in (1, 2, 3)) == counts
        assert [R.nodes_offset(bw, bh, k) for k in (1, 2, 3)] == [0, counts[0], counts[0] + counts[1]] and R.nodes_total(bw, bh) == sum(counts)
    bw, bh = 10, 6                                                          # 80 x 48
    assert R.whole(bw, bh, 2, 1, 0) and not R.whole(bw, bh, 2, 2, 0) and not R.whole(bw, bh, 2, 0, 1) and not R.whole(bw, bh, 3, 0, 0)
    assert R.exists(bw, bh, 2, 2, 1) and not R.exists(bw, bh, 2, 3, 0) and R.exists(bw, bh, 3, 1, 0) and not R.exists(bw, bh, 3, 0, 1)


@pytest.mark.parametrize("w,h", [(64, 64), (80, 48), (144, 112)])
def test_consequences_1_and_3(oracle, w, h):
    cur, ref, mv = frames(w, h)
    fin = R.field_in(mv, w, h).reshape(-1, 2)
    for lam in (0, 64, 65535):
        d = decision(oracle, w, h, lam, 0)
        for b, rec in enumerate(d["out"]):                                   # 1. every output vector is an input vector of the same CTU
            mine = [tuple(fin[o]) for o in range(len(fin)) if R.ctu_of_block(w, o) == R.ctu_of_block(w, b)]
            assert (int(rec["mvx"]), int(rec["mvy"])) in mine
    d = decision(oracle, w, h, 0, 0)                                         # 3. the unmerged field is one of the choices
    own = Q.block_satd(oracle, cur, Q.mc_luma(ref, fin)[0]).astype(np.int64)
    assert np.array_equal(own, d["d0"])
    for c, rec in enumerate(d["ctu"]):
        blocks = [b for b in range(len(fin)) if R.ctu_of_block(w, b) == c]
        assert int(rec["j"]) <= own[blocks].sum() and int(rec["j"]) == int(rec["dist"])
    # 4. the output field reproduces its own costs
    out = np.stack([d["out"]["mvx"], d["out"]["mvy"]], axis=1)
    assert np.array_equal(Q.block_satd(oracle, cur, Q.mc_luma(ref, out)[0]), d["out"]["cost"])


@pytest.mark.parametrize("lam", [0, 8, 16, 4096, 65535])
def test_consequence_2_a_constant_field(oracle, lam):
    w, h, q = 144, 112, (5, -3)
    cur, ref, _ = frames(w, h)
    bw, bh = w // 8, h // 8
    mv = np.tile(np.array([q], np.int16), (bw * bh, 1))
    d = R.decide(oracle, cur, ref, mv, 0, lam)
    largest = [max(k for k in range(4) if R.whole(bw, bh, k, (b % bw) >> k, (b // bw) >> k)) for b in range(bw * bh)]
    assert d["level"].tolist() == largest and set(largest) == {1, 2, 3}
    assert all(d["merged"].values()) and len(d["cut_split"]) == 12
    assert (d["out"]["mvx"] == q[0]).all() and (d["out"]["mvy"] == q[1]).all()
    assert np.array_equal(d["out"]["cost"], Q.block_satd(oracle, cur, Q.mc_luma(ref, mv)[0]))
    assert d["ctu"]["parts"].tolist()[:3] == [1, 1, 4] and d["ctu"]["parts"].sum() == sum(1.0 / 4 ** k for k in largest)


def test_below_lambda_8_the_floors_can_favour_the_split(oracle):
    """the header's counter-example to consequence 2: lambda_q4 7, (7 * 3) >> 4 = 1 against 4 * ((7 * 2) >> 4) + (7 >> 4) = 0"""
    w, h = 128, 64
    cur, ref, _ = frames(w, h)
    d = R.decide(oracle, cur, ref, np.tile(np.array([[5, -3]], np.int16), (128, 1)), 0, 7)
    second = np.array([R.ctu_of_block(w, b) == 1 for b in range(128)])
    assert not d["merged"][3, 1, 0] and (d["level"][second] == 0).all()     # every node of the second CTU has P = q
    assert d["merged"][3, 0, 0] and (d["level"][~second] == 3).all()        # the first CTU's P is (0, 0): its own rate hides the flag's


def test_cut_nodes_split_without_a_flag(oracle):
    w, h = 80, 48                                                           # no whole level-3 node, level 2 whole only in the top row
    d = decision(oracle, w, h, 4096, 1)
    assert sorted(d["cut_split"]) == [(2, 0, 1), (2, 1, 1), (2, 2, 0), (2, 2, 1), (3, 0, 0), (3, 1, 0)]
    assert set(d["merged"]) == {(1, x, y) for x in range(5) for y in range(3)} | {(2, 0, 0), (2, 1, 0)} and d["level"].max() <= 2
    lam_flag = 4096 >> 4
    for c, rec in enumerate(d["ctu"]):
        blocks = [b for b in range(60) if R.ctu_of_block(w, b) == c]
        parts = sum(1.0 / 4 ** int(d["level"][b]) for b in blocks)
        assert int(rec["parts"]) == parts
        assert int(rec["dist"]) == int(d["out"]["cost"][blocks].sum())       # the partitions' distortion is the sum of their blocks' own SATDs
        splits = sum(1 for (k, nx, ny), m in d["merged"].items() if not m and (nx << k) >> 3 == c)
        assert int(rec["j"]) >= int(rec["dist"]) + splits * lam_flag
    whole_frame = R.decide(oracle, *frames(64, 64)[:2], frames(64, 64)[2], 1, 4096)
    assert set(whole_frame["merged"]) >= {(3, 0, 0)} and not whole_frame["cut_split"]


def test_a_tie_merges_and_the_first_of_the_walk_wins(oracle):
    """constant frames: every SATD is 0.  With lambda_q4 0 every Jw ties at 0: the first candidate of the walk wins at every level (the
    top-left child's vector moved by (-r, -r)) and every node merges on the tie."""
    w, h = 64, 64
    flat = np.full((h, w), 77, np.uint8)
    mv = R.motion_field(w, h, 3)
    for r in (0, 1):
        d = R.decide(oracle, flat, flat, mv, r, 0)
        assert all(d["merged"].values()) and (d["level"] == 3).all() and not d["ctu"]["j"].any() and d["ctu"]["parts"].tolist() == [1]
        assert (int(d["out"]["mvx"][0]), int(d["out"]["mvy"][0])) == (int(mv[0, 0]) - 3 * r, int(mv[0, 1]) - 3 * r)
        first_l1 = d["nodes"][R.nodes_offset(8, 8, 1) + 1]                  # the level-1 node at block (2, 0)
        assert (int(first_l1["mvx"]), int(first_l1["mvy"]), int(first_l1["cost"])) == (int(mv[2, 0]) - r, int(mv[2, 1]) - r, 0)
    d = R.decide(oracle, flat, flat, mv, 0, 16)                              # with a price on the bits the cheapest vector wins, not the first
    assert int(d["ctu"]["j"][0]) == int(d["ctu"]["bits"][0]) and not d["ctu"]["dist"].any()


def test_the_condition_of_the_gpu_case(oracle):
    d = decision(oracle, 144, 112, 4096, 1)
    assert (np.bincount(d["level"], minlength=4) > 0).all()
    assert d["cut_split"] and any(not m for m in d["merged"].values())
