"""CPU: the reference statement of bi-directional prediction (tests/_bipred_ref.py) against the quarter-sample statement it extends,
the identities the header states, the range of the intermediate V, and the coverage the GPU cases of tests/test_gpu_bipred.py rely
on (so that a recipe cannot quietly stop testing something)."""
import numpy as np
import pytest

import _bipred_ref as B
import _subpel_ref as R


def _sample_v(S, x, y, mvx, mvy, kind):
    """V of ONE sample in plain Python integers"""
    tab, lg, o, _ = R.PLANE[kind]
    T = [[int(t) for t in row] for row in tab]
    n = len(T[0])
    ix, fx, iy, fy = mvx >> lg, mvx & ((1 << lg) - 1), mvy >> lg, mvy & ((1 << lg) - 1)
    return sum(T[fy][j] * sum(T[fx][k] * S(y + iy + j - o, x + ix + k - o) for k in range(n)) for j in range(n)) >> 6


@pytest.mark.parametrize("kind", ["luma", "chroma"])
def test_v_against_plain_loops(kind):
    w, h = 32, 16
    plane = R.plane("extreme", w, h, 5)
    edge = R.PLANE[kind][3]
    mv = R.mv_mix_q((w // edge) * (h // edge), w, h, 6)
    got = B.V(plane, mv, kind)
    S = lambda y, x: int(plane[min(max(y, 0), h - 1)][min(max(x, 0), w - 1)])
    for y in range(h):
        for x in range(w):
            mvx, mvy = (int(t) for t in mv[(y // edge) * (w // edge) + x // edge])
            assert got[y, x] == _sample_v(S, x, y, mvx, mvy, kind), (x, y)


@pytest.mark.parametrize("w,h", [(32, 32), (144, 80)])
@pytest.mark.parametrize("kind", R.KINDS)
def test_uni_path_is_the_quarter_sample_statement(w, h, kind):
    y, u, v = R.planes(kind, w, h, 11 + w)
    y1, u1, v1 = R.planes(kind, w, h, 12 + w)
    mv0, mv1 = B.vectors(w, h, w * h)
    nb = len(mv0)
    for d, mv, (py, pu, pv) in ((1, mv0, (y, u, v)), (2, mv1, (y1, u1, v1))):
        direction = np.full(nb, d, np.uint8)
        assert np.array_equal(B.bi_plane(y, y1, mv0, mv1, direction, None, "luma", 0, y), R.mc_luma(py, mv)[0])
        assert np.array_equal(B.bi_plane(u, u1, mv0, mv1, direction, None, "chroma", 1, u), R.mc_plane(pu, mv, "chroma")[0])
        assert np.array_equal(B.bi_plane(v, v1, mv0, mv1, direction, None, "chroma", 2, v), R.mc_plane(pv, mv, "chroma")[0])


def test_unit_weights_are_the_default_for_every_denominator():
    w, h = 48, 32
    mv0, mv1 = B.vectors(w, h, 21)
    direction = B.directions(len(mv0), 22)
    for kind in R.KINDS:
        p0, p1 = R.planes(kind, w, h, 23), R.planes(kind, w, h, 26)
        for d in range(8):
            wp = B.unit_weights(d, 7 - d)
            for comp, which in ((0, "luma"), (1, "chroma"), (2, "chroma")):
                want = B.pre_plane(p0[comp], p1[comp], mv0, mv1, direction, None, which, comp)[0]
                assert np.array_equal(B.pre_plane(p0[comp], p1[comp], mv0, mv1, direction, wp, which, comp)[0], want), (kind, d, comp)


def test_bi_of_identical_lists_is_the_uni_prediction():
    w, h = 48, 32
    mv = R.mv_mix_q((w // 8) * (h // 8), w, h, 31)
    for kind in R.KINDS:
        y, u, v = R.planes(kind, w, h, 32)
        assert np.array_equal(B.bi_plane(y, y, mv, mv, None, None, "luma", 0, y), R.mc_luma(y, mv)[0])
        assert np.array_equal(B.bi_plane(u, u, mv, mv, None, None, "chroma", 1, u), R.mc_plane(u, mv, "chroma")[0])


def test_crafted_planes_reach_the_stated_extremes_of_v():
    hi, lo = B.crafted_extremes()
    mv = np.tile(np.int16([[2, 2]]), (16, 1))
    assert B.V(hi, mv, "luma").max() == 33150 and B.V(hi, mv, "luma")[16, 16] == 33150
    assert B.V(lo, mv, "luma").min() == -16830 and B.V(lo, mv, "luma")[16, 16] == -16830
    # no content goes further: 255 times the sum of the positive (negative) tap products, floored by the shift.  The header's chroma
    # range -5897..22217 holds every value; its upper end is 255 * 5576 / 64 = 22216.875 rounded up, the largest V itself is 22216.
    for tab, lo_v, hi_v in ((R.TL, -16830, 33150), (R.TC, -5897, 22216)):
        prods = [np.outer(a, b) for a in tab for b in tab]
        assert max((255 * np.maximum(p, 0).sum()) >> 6 for p in prods) == hi_v
        assert min((255 * np.minimum(p, 0).sum()) >> 6 for p in prods) == lo_v
    assert 33150 > 32767                                                    # V does not fit int16


def test_decide_takes_the_earlier_of_equal_costs():
    c = np.array([[5, 5, 5], [6, 5, 5], [6, 6, 5], [5, 6, 0], [7, 6, 0]], np.uint32)
    assert B.decide(c, 0).tolist() == [1, 2, 3, 3, 3]
    assert B.decide(c, 5).tolist() == [1, 2, 1, 1, 3]
    assert B.decide(c, 65535).tolist() == [1, 2, 1, 1, 2]


# ---- the coverage the GPU cases rely on ---------------------------------------------------------------------------------------------
def test_direction_recipe_takes_all_four_values():
    for w, h in B.SIZES:
        d = B.directions((w // 8) * (h // 8), w + h)
        assert set((d & 3).tolist()) == {0, 1, 2, 3}
        assert (d > 3).any()                                                # the upper bits are noise


def test_extreme_content_reaches_both_clips_before_the_bi_rounding():
    w, h = 144, 80
    mv0, mv1 = B.vectors(w, h, w * h)
    p0, p1 = B.case_planes("extreme", w, h)
    pre = B.pre_plane(p0[0], p1[0], mv0, mv1, None, None, "luma", 0)[0]
    print("bi values below 0: %d, above 255: %d" % ((pre < 0).sum(), (pre > 255).sum()))
    assert (pre < 0).sum() > 0 and (pre > 255).sum() > 0


def test_every_phase_class_occurs_for_each_list():
    for (w, h), lg, n in (((32, 32), 2, 16), ((64, 64), 3, 64)):
        for mv in B.vectors(w, h, w * h):
            f = np.asarray(mv, np.int64) & ((1 << lg) - 1)
            assert len(set(map(tuple, f.tolist()))) == n
    mv0, mv1 = B.vectors(144, 80, 144 * 80)
    assert not np.array_equal(mv0, mv1)
    for mv in (mv0, mv1):
        m = mv.astype(np.int64)
        assert (np.abs(m) >= 32766).any() and ((m[:, 0] > 4 * 144) | (m[:, 0] < -4 * 152)).any()      # int16 extremes, wholly outside


def test_weighted_cases_cover_what_they_are_for():
    ws = list(B.WEIGHTS.values())
    assert any((wp.w < 0).any() for wp in ws) and any((wp.o != 0).any() for wp in ws)
    denoms = {d for wp in ws for d in wp.log2_denom}
    assert 0 in denoms and any(d > 0 for d in denoms)
    for wp in ws:
        assert wp.w.min() >= -128 and wp.w.max() <= 127 and wp.o.min() >= -128 and wp.o.max() <= 127 and all(0 <= d <= 7 for d in wp.log2_denom)


def test_decision_recipe_lets_every_direction_win_and_a_tie_goes_to_list_0(oracle):
    w, h = 144, 80
    cur, ref0, ref1, mv0, mv1 = B.decision_case(oracle, w, h, 900)
    costs, direction = B.costs3(oracle, cur, ref0, ref1, mv0, mv1, None, 0)
    share = np.bincount(direction, minlength=4)
    print("winners 1, 2, 3: %s of %d blocks" % (share[1:].tolist(), len(direction)))
    assert share[0] == 0 and (share[1:] >= len(direction) // 6).all()
    assert B.costs3(oracle, cur, ref0, ref1, mv0, mv1, None, 65535)[1].max() == 2      # a large penalty prices the second vector out
    # identical lists: the three costs are equal in every block, and the earlier wins
    costs, direction = B.costs3(oracle, cur, ref0, ref0, mv0, mv0, None, 0)
    assert (costs[:, 0] == costs[:, 1]).all() and (costs[:, 0] == costs[:, 2]).all() and (direction == 1).all()
