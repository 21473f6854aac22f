"""CPU: the reference statement of tests/_mixed_frame_ref.py (xDct32CodeMixedFrameGpu) against the two statements it must agree with --
consequence (a) against Q.code_ctu_tiles, consequence (b) against R.code_frame -- the worked numbers of the header, the conditions the
inputs of tests/test_gpu_mixed_frame.py must meet for that test to mean something (both kinds occur), the tie rule and the chroma
candidate list."""
import os
import re

import numpy as np
import pytest

import _intra_frame_ref as R
import _mixed_frame_ref as M
import _quant_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QP, ROUNDING = 22, 171


def _qps(n):
    return (20 + R._noise(77, (n, 6), 0, 40)).astype(np.uint8)             # some above 51: clamped


@pytest.mark.parametrize("w,h", R.SIZES)
def test_every_kind_inter_is_the_fused_ctu_call(oracle, w, h):
    """consequence (a)"""
    cur, pred = M.pred_planes(w, h, 0)
    n = (w // 64) * (h // 64)
    for qps in (None, _qps(n)):
        got = M.code_frame(oracle, cur, pred, w, h, qps, QP, ROUNDING, 0, np.zeros((n, 6), np.uint8))
        base = R.tiles(oracle, pred, 3)
        level, nnz, recon = Q.code_ctu_tiles(oracle, R.tiles(oracle, cur, 1), base, w, h, qps, QP, ROUNDING)
        assert np.array_equal(got.levels, level) and np.array_equal(got.nnz, nnz)
        assert np.array_equal(got.recon_tiles(oracle, base), recon)
        assert not got.kinds.any() and (got.modes == M.INTER_MODE).all() and (got.costs == M.NO_COST).all()


@pytest.mark.parametrize("w,h", R.SIZES)
def test_every_kind_intra_is_the_intra_frame(oracle, w, h):
    """consequence (b); the prediction is poison and changes nothing"""
    cur, _ = M.pred_planes(w, h, 0)
    n = (w // 64) * (h // 64)
    poison = tuple(np.full_like(p, 0xA5) for p in cur)
    got = M.code_frame(oracle, cur, poison, w, h, None, QP, ROUNDING, 4096, np.ones((n, 6), np.uint8))
    want = R.coded(oracle, "oriented", w, h, QP, ROUNDING)
    assert np.array_equal(got.levels, want.levels) and np.array_equal(got.nnz, want.nnz) and np.array_equal(got.modes, want.modes)
    assert all(np.array_equal(a, b) for a, b in zip(got.planes, want.planes))
    assert (got.kinds == 1).all() and (got.costs[:, :, 0] == M.NO_COST).all() and (got.costs[:, :, 1] < 1 << 26).all()
    assert np.array_equal(got.costs[:, 4], got.costs[:, 5])
    # with the modes fed back the same frame, and no intra cost: the call scored nothing
    again = M.code_frame(oracle, cur, poison, w, h, None, QP, ROUNDING, 0, np.ones((n, 6), np.uint8), want.modes)
    assert np.array_equal(again.levels, want.levels) and (again.costs == M.NO_COST).all()


def test_the_worked_numbers_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    m = re.search(r"with inter_cost (\d+) and\s+\*?\s*intra_cost (\d+) the region is intra at penalty 0 and at (\d+), and inter at (\d+) \(the tie\) and at (\d+)", hdr)
    assert m, "the header's worked decision"
    inter, intra, below, tie, above = map(int, m.groups())
    assert (inter, intra, below, tie, above) == (6087, 4699, 1387, 1388, 4096)
    assert M.is_intra(2, inter, intra, 0) and M.is_intra(2, inter, intra, below)
    assert not M.is_intra(2, inter, intra, tie) and not M.is_intra(2, inter, intra, above)
    assert M.is_intra(1, 0, M.NO_COST, 1 << 24) and not M.is_intra(0, M.NO_COST, 0, 0)      # a given kind stands


@pytest.mark.parametrize("flip", (0, 1))
@pytest.mark.parametrize("w,h", R.SIZES)
def test_both_kinds_occur(oracle, w, h, flip):
    """a condition of the GPU test: every size gives both kinds in luma, every size with two or more CTUs both kinds in chroma, 64 x 64 one
    chroma kind per flip"""
    for penalty in (0, 4096):
        got = M.coded(oracle, w, h, flip, penalty)
        assert set(got.kinds[:, :4].ravel()) == {0, 1}
        assert np.array_equal(got.kinds[:, 4], got.kinds[:, 5]) and np.array_equal(got.modes[:, 4], got.modes[:, 5])
        assert set(got.kinds[:, 4]) == ({0, 1} if w * h > 64 * 64 else {flip})
        assert ((got.modes == M.INTER_MODE) == (got.kinds == 0)).all() and (got.modes[got.kinds == 1] < 35).all()
        assert (got.costs < 1 << 26).all()                                  # every region decided: both costs written


def test_the_penalty_moves_a_region(oracle):
    """at 128 x 64, flip 0, region 9 (CTU 1, quadrant 3): inter cost 6036, intra cost 4699 -- intra at penalty 0, inter at 4096"""
    a, b = M.coded(oracle, 128, 64, 0, 0), M.coded(oracle, 128, 64, 0, 4096)
    assert tuple(a.costs[1, 3]) == (6036, 4699) and tuple(b.costs[1, 3]) == (6036, 4699)
    assert a.kinds[1, 3] == 1 and b.kinds[1, 3] == 0


def first_intra(m):
    """(ctu, entry) of the first region in coding order that ended intra"""
    for ctu in range(m.kinds.shape[0]):
        for e in range(5):
            if m.kinds[ctu, e]:
                return ctu, e
    raise AssertionError("no intra region")


@pytest.mark.parametrize("flip", (0, 1))
@pytest.mark.parametrize("w,h", R.SIZES)
def test_a_tie_is_inter(oracle, w, h, flip):
    """the first region that is intra at penalty 0, with intra_penalty = inter_cost - intra_cost: inter; with one less: intra.  The
    regions before it are all inter and cannot change, so its costs stand"""
    free = M.coded(oracle, w, h, flip, 0)
    ctu, e = first_intra(free)
    inter, intra = (int(x) for x in free.costs[ctu, e])
    assert intra < inter
    cur, pred = M.pred_planes(w, h, flip)
    tie = M.code_frame(oracle, cur, pred, w, h, None, QP, ROUNDING, inter - intra)
    less = M.code_frame(oracle, cur, pred, w, h, None, QP, ROUNDING, inter - intra - 1)
    for got in (tie, less):
        assert tuple(got.costs[ctu, e]) == (inter, intra)
        assert not got.kinds.ravel()[:6 * ctu + e].any()
    assert tie.kinds[ctu, e] == 0 and tie.modes[ctu, e] == M.INTER_MODE
    assert less.kinds[ctu, e] == 1 and less.modes[ctu, e] == free.modes[ctu, e]


def test_the_chroma_candidate_list(oracle):
    """(0, 26, 10, 1), then quadrant 0's mode only if quadrant 0 ended intra"""
    assert M.chroma_candidates(0, 255) == [0, 26, 10, 1] and M.chroma_candidates(1, 7) == [0, 26, 10, 1, 7]
    seen = set()
    for w, h in R.SIZES:
        for flip in (0, 1):
            got = M.coded(oracle, w, h, flip, 0)
            for ctu, cand in enumerate(got.candidates):
                assert cand == M.chroma_candidates(got.kinds[ctu, 0], got.modes[ctu, 0])
                seen.add(len(cand))
    assert seen == {4, 5}
    # quadrant 0's mode can win only where it is in the list: force it to be the one good candidate
    w, h = 64, 64
    cur, pred = M.pred_planes(w, h, 1)                                     # flip 1: quadrant 0 and the chroma are intra
    got = M.coded(oracle, w, h, 1, 0)
    assert got.kinds[0, 0] == 1 and got.kinds[0, 4] == 1 and len(got.candidates[0]) == 5
    kinds = np.array([[0, 2, 2, 2, 2, 2]], np.uint8)                       # quadrant 0 given as inter: four candidates
    forced = M.code_frame(oracle, cur, pred, w, h, None, QP, ROUNDING, 0, kinds)
    assert forced.candidates[0] == [0, 26, 10, 1] and forced.kinds[0, 0] == 0 and forced.modes[0, 4] in (0, 26, 10, 1, M.INTER_MODE)


def test_a_region_depends_only_on_earlier_regions(oracle):
    """consequence (c): changing the kind of the last CTU changes nothing in front of it"""
    w, h = 128, 128
    cur, pred = M.pred_planes(w, h, 0)
    k = M.kinds_mixed(4)
    a = M.code_frame(oracle, cur, pred, w, h, None, QP, ROUNDING, 0, k)
    k2 = k.copy()
    k2[3] = 1 - np.minimum(k[3], 1)
    b = M.code_frame(oracle, cur, pred, w, h, None, QP, ROUNDING, 0, k2)
    assert np.array_equal(a.levels[:3], b.levels[:3]) and np.array_equal(a.kinds[:3], b.kinds[:3]) and np.array_equal(a.costs[:3], b.costs[:3])
    assert set(np.minimum(k, 2).ravel()) == {0, 1, 2} and (k > 2).any()   # the mix has every kind and bytes above 2
