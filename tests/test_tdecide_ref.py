"""CPU: tests/_tdecide_ref.py, the statement of xTransformDecideCtuTilesGpu by composition of the committed references, held against
what the contract says in words: the winners of five kinds of synthetic content, ties worked by hand, the d_cost sentinels and the
d_cand fallback.  The bindings must exist for the statement to mean anything: the module asserts them first."""
import numpy as np
import pytest

import _tdecide_ref as T
import x266_amd

LAM = 368


@pytest.fixture(autouse=True)
def _the_bindings_exist():
    assert hasattr(x266_amd, "TDecideParams") and callable(getattr(x266_amd.Codec, "transform_decide_dev", None))


def test_the_statement_is_of_a_call_the_library_has():
    assert hasattr(x266_amd.load_library(), "xTransformDecideCtuTilesGpu") and callable(x266_amd.Codec.transform_decide_dev)
    assert x266_amd.TDECIDE_CLASSES == T.CLASSES and len(T.CLASS_LIST) == 13 and 7 not in T.CLASS_LIST


def _winner(oracle, res, qp, mask=T.CLASSES, bits=None):
    cls, level, stat, cost = T.decide_regions(oracle, res[None], [mask], [qp], LAM, bits)
    return int(cls[0]), cost[0]


# content kind, seed, qp -> the winner among all 13 classes at lambda 368 without side bits
WINNERS = [("sinusoid", 9, 27, 3), ("sinusoid", 9, 37, 3), ("edge", 9, 27, 3), ("edge", 9, 37, 3), ("ramp8", 9, 27, 3), ("ramp8", 9, 37, 3),
           ("noise6", 9, 27, 5), ("noise6", 9, 37, 5), ("spot", 9, 27, 12), ("spot", 8, 27, 8), ("spot", 9, 37, 4)]


@pytest.mark.parametrize("kind,seed,qp,want", WINNERS)
def test_winners_of_the_five_kinds_of_content(oracle, kind, seed, qp, want):
    got, cost = _winner(oracle, T.content(kind, seed), qp)
    assert got == want, (got, cost)
    c = cost[T.CLASS_LIST].astype(np.float64)
    if kind in ("sinusoid", "edge", "ramp8"):                                # DCT-II 32 wins by 10 % and more
        assert np.sort(c)[1] >= 1.10 * c.min()
    if kind == "noise6":                                                     # ... DST-VII 8 by a fraction of a percent
        assert np.sort(c)[1] < 1.01 * c.min()


def test_the_choice_is_not_degenerate(oracle):
    winners = {_winner(oracle, T.content(kind, seed), qp)[0] for kind, seed, qp, _ in WINNERS}
    assert len(winners) >= 4 and winners == {3, 4, 5, 8, 12}


def test_ties_worked_by_hand(oracle):
    """cur == pred: every coefficient is 0, the all-zero region has dist 0 and bits 0, J_k = lambda * class_bits[k]"""
    zero = np.zeros((32, 32), np.int16)
    for mask, lowest in ((T.CLASSES, 0), (0x7770, 4), (0x0408, 3), (0x4000, 14)):
        for bits in (None, [48] * 16):                                       # equal side bits: the lowest set bit wins
            got, cost = _winner(oracle, zero, 30, mask, bits)
            assert got == lowest
            assert all(int(cost[k]) == (LAM * 48 if bits else 0) for k in T.CLASS_LIST if (mask >> k) & 1)
    bits = [48] * 16
    bits[9] = 47                                                             # one cheaper class wins
    got, cost = _winner(oracle, zero, 30, T.CLASSES, bits)
    assert got == 9 and int(cost[9]) == LAM * 47 and int(cost[0]) == LAM * 48
    got, cost = _winner(oracle, zero, 30, 0x0033, bits)                      # ... unless it is no candidate
    assert got == 0 and cost[9] == T.ALL_ONES
    # side bits flip a real decision: the sinusoid's runner-up takes over once class 3 costs more than the gap
    res = T.content("sinusoid", 9)
    got, cost = _winner(oracle, res, 27)
    second = min((k for k in T.CLASS_LIST if k != 3), key=lambda k: int(cost[k]))
    gap = (int(cost[second]) - int(cost[3])) // LAM                          # in 1/16 bit, rounded down: J_3 + lambda * gap <= J_second
    assert 0 < gap < 65535
    for extra, want in ((gap, 3), (gap + 1, second)):
        bits = [0] * 16
        bits[3] = extra
        assert _winner(oracle, res, 27, T.CLASSES, bits)[0] == want, extra


def test_cost_sentinels_and_the_record_of_the_winner(oracle):
    res = np.stack([T.content(kind, 9) for kind in T.KINDS])
    masks = [0x0008, 0x0028, T.CLASSES, 0x7000, 0x0101]
    cls, level, stat, cost = T.decide_regions(oracle, res, masks, [27] * 5, LAM, list(range(16)))
    for r, mask in enumerate(masks):
        cand = [(mask >> k) & 1 == 1 for k in range(16)]
        assert np.array_equal(cost[r] != T.ALL_ONES, cand)
        k = int(cls[r])
        assert cand[k] and int(cost[r, k]) == min(int(cost[r, j]) for j in range(16) if cand[j])
        assert int(cost[r, k]) == int(stat["dist"][r]) + LAM * (int(stat["bits"][r]) + k)
        assert int(stat["n_nz"][r]) == np.count_nonzero(level[r])
    assert cls[0] == 3 and set(cls.tolist()) <= set(T.CLASS_LIST)


def test_d_cand_falls_back_when_no_valid_bit_is_set():
    n = 12
    cand = np.array([0, 0x0008, 0x0880, 0x8000, 0xFFFF, 0x0080, 0, 0x0800, 0x7000, 0x0080, 0x0002, 0x8880], np.uint16)
    got = T.effective_masks(n, 0x0030, 0x0700, cand)
    luma, chroma = 0x0030, 0x0700
    assert got.tolist() == [luma, 0x0008, luma, luma, 0x777F, chroma, luma, luma, 0x7000, luma, 0x0002, chroma]
    assert T.effective_masks(n, luma, chroma).tolist() == [luma] * 4 + [chroma] * 2 + [luma] * 4 + [chroma] * 2


def test_the_frame_statement_and_the_shared_content(oracle):
    """a frame's regions are those of xTransformCtuFromTilesDev's statement: 6 ctu + q, zero outside the frame; a region wholly outside
    follows the general rule"""
    w, h = 80, 48
    cur, pred = T.content_frames(oracle, w, h)
    res = T.residual_regions(cur, pred, w, h)
    assert res.shape == (12, 32, 32) and not res[7].any() and not res[9].any() and res[6].any() and not res[6][:, 16:].any()
    assert np.array_equal(res[0], T.content(T.KINDS[3 % 5], 3))               # cell (0, 0) of the luma plane
    cls, level, stat, cost = T.decide(oracle, cur, pred, w, h, qp=32, lam=LAM, class_bits=[16] * 16, regions=[0, 7, 10])
    assert cls[1] == 0 and int(cost[1, 0]) == LAM * 16 and not level[1].any()
    masks = T.encoder_masks(w, h)
    assert masks.tolist() == [0, 0, 0x7777, 0x7777, 0x3333, 0x3333, 0x7777, 0, 0x7777, 0, 0x3333, 0x3333]
