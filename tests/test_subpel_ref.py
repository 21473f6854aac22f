"""CPU: the reference statement of quarter-sample prediction (tests/_subpel_ref.py) against plain Python loops sample by sample,
its vector-split convention, the tap tables' symmetries, its agreement with the integer statements of the existing test modules
on vectors 4m, and the coverage the GPU cases of tests/test_gpu_subpel.py rely on (so that a recipe change shows here first)."""
import numpy as np
import pytest

import _subpel_ref as R
from test_gpu_mc_chroma import _mcc_plane_np, _mv_mix
from test_gpu_me_tiles import _mc_np


# ---- plain loops ------------------------------------------------------------------------------------------------------------------------
def _sample(S, x, y, mvx, mvy, kind):
    """ONE sample in plain Python integers, S(y, x) the clamped plane -> (value before the clip, v or None)"""
    tab, lg, o, _ = R.PLANE[kind]
    T = [[int(t) for t in row] for row in tab]
    n = len(T[0])
    ix, fx, iy, fy = mvx >> lg, mvx & ((1 << lg) - 1), mvy >> lg, mvy & ((1 << lg) - 1)
    if not fx and not fy:
        return S(y + iy, x + ix), None
    if not fy:
        return (sum(T[fx][k] * S(y + iy, x + ix + k - o) for k in range(n)) + 32) >> 6, None
    if not fx:
        return (sum(T[fy][k] * S(y + iy + k - o, x + ix) for k in range(n)) + 32) >> 6, None
    hs = [sum(T[fx][k] * S(y + iy + r - o, x + ix + k - o) for k in range(n)) for r in range(n)]
    lo, hi = ((-6120, 22440) if kind == "luma" else (-2550, 18870))        # 255 * (sum of negative taps), 255 * (sum of positive taps)
    assert all(lo <= t <= hi for t in hs)
    v = sum(T[fy][r] * hs[r] for r in range(n)) >> 6
    return (v + 32) >> 6, v


def _plane_loops(plane, mv, kind):
    _, lg, _, edge = R.PLANE[kind]
    ph, pw = plane.shape
    n = 1 << lg
    out = np.zeros((ph, pw), np.uint8)
    c = R.Counts(n)
    S = lambda y, x: int(plane[min(max(y, 0), ph - 1)][min(max(x, 0), pw - 1)])
    for y in range(ph):
        for x in range(pw):
            mvx, mvy = (int(t) for t in mv[(y // edge) * (pw // edge) + x // edge])
            pre, v = _sample(S, x, y, mvx, mvy, kind)
            cls = (mvx & (n - 1), mvy & (n - 1))
            c.samples[cls] += 1
            c.below[cls] += pre < 0
            c.above[cls] += pre > 255
            c.negative_v[cls] += v is not None and v < 0
            out[y, x] = min(max(pre, 0), 255)
    return out, c


@pytest.mark.parametrize("w,h", [(16, 16), (48, 32)])
@pytest.mark.parametrize("kind", R.KINDS)
def test_statement_against_plain_loops(w, h, kind):
    y, u, v = R.planes(kind, w, h, 3 * w + h)
    mv = R.vectors(w, h, w * h)
    for plane, which in ((y, "luma"), (u, "chroma"), (v, "chroma")):
        got, counts = R.mc_plane(plane, mv, which)
        want, wcounts = _plane_loops(plane, mv, which)
        assert np.array_equal(got, want)
        assert counts == wcounts, (counts, wcounts)
        assert counts.samples.sum() == plane.size
    # a zero vector copies, a whole-sample vector moves bytes, a constant plane stays constant
    nb = (w // 8) * (h // 8)
    assert np.array_equal(R.mc_luma(y, np.zeros((nb, 2), np.int16))[0], y)
    assert np.array_equal(R.mc_luma(y, np.tile(np.int16([[4, -8]]), (nb, 1)))[0][2:, :-1], y[:-2, 1:])
    assert np.array_equal(R.mc_plane(u, np.tile(np.int16([[8, -16]]), (nb, 1)), "chroma")[0][2:, :-1], u[:-2, 1:])
    assert (R.mc_luma(np.full_like(y, 201), mv)[0] == 201).all()
    assert (R.mc_plane(np.full_like(u, 7), mv, "chroma")[0] == 7).all()


def test_vector_split_is_arithmetic():
    for lg, mv, want in ((2, -1, (-1, 3)), (2, -32768, (-8192, 0)), (2, 32767, (8191, 3)), (2, -5, (-2, 3)), (2, -4, (-1, 0)),
                         (3, -1, (-1, 7)), (3, -32768, (-4096, 0)), (3, 32767, (4095, 7)), (3, -9, (-2, 7))):
        i, f = R.split(mv, lg)
        assert (int(i), int(f)) == want == (mv >> lg, mv & ((1 << lg) - 1))
    S = lambda y, x: 10 * y + x
    assert _sample(S, 20, 20, -32768, 32764, "luma") == (10 * (20 + 8191) + 20 - 8192, None)
    one = np.full((16, 16), 9, np.uint8)
    assert (R.mc_luma(one, np.int16([[-32768, 32767], [32767, -32767], [-1, -1], [1, 1]]))[0] == 9).all()


def test_tap_rows_sum_to_64_and_mirror():
    assert (R.TL.sum(axis=1) == 64).all() and (R.TC.sum(axis=1) == 64).all()
    assert np.array_equal(R.TL[3], R.TL[1][::-1]) and np.array_equal(R.TL[2], R.TL[2][::-1])
    for f in range(1, 8):
        assert np.array_equal(R.TC[8 - f], R.TC[f][::-1])
    assert R.TL[0].tolist() == [0, 0, 0, 64, 0, 0, 0, 0] and R.TC[0].tolist() == [0, 64, 0, 0]
    assert R.TC[4].tolist() == [-4, 36, 36, -4]                              # the half-sample filter of xMotionCompChromaDev
    # what the header says about the horizontal stage
    for tab, lo, hi in ((R.TL, -6120, 22440), (R.TC, -2550, 18870)):
        assert 255 * np.minimum(tab, 0).sum(axis=1).min() == lo and 255 * np.maximum(tab, 0).sum(axis=1).max() == hi


@pytest.mark.parametrize("w,h", [(48, 32), (144, 80)])
def test_vectors_4m_are_the_integer_statements(w, h):
    nb = (w // 8) * (h // 8)
    y, u, v = R.planes("random", w, h, 50 + w)
    m = np.clip(_mv_mix(nb, w, h, 60 + h).astype(np.int64), -8191, 8191)
    assert np.abs(m).max() == 8191 and (m & 1).any()
    q = (4 * m).astype(np.int16)
    assert np.array_equal(R.mc_luma(y, q)[0], _mc_np(y, m, w, h))
    for plane in (u, v):
        got, counts = R.mc_plane(plane, q, "chroma")
        assert np.array_equal(got, _mcc_plane_np(plane, m, w, h)[0])
        assert counts.samples[[0, 0, 4, 4], [0, 4, 0, 4]].sum() == plane.size  # only phases 0 and 4


def test_winner_rule():
    c = np.full((4, 49), 9, np.uint32)
    c[1, 30] = c[1, 40] = 3
    c[2, 24] = c[2, 5] = 2
    c[3, 24], c[3, 5] = 2, 1
    assert R.winner(c).tolist() == [24, 30, 24, 5]


# ---- the coverage the GPU cases assert, from the statement alone -------------------------------------------------------------------
def case_counts(w, h):
    """(luma Counts, chroma Counts) of a size's case of tests/test_gpu_subpel.py, summed over its plane kinds"""
    luma, chroma = R.Counts(4), R.Counts(8)
    mv = R.vectors(w, h, w * h)
    for n, kind in enumerate(R.KINDS):
        y, u, v = R.planes(kind, w, h, 31 + w + 7 * n)
        luma += R.mc_luma(y, mv)[1]
        chroma += R.mc_chroma(u, v, mv)[2]
    return luma, chroma


@pytest.mark.parametrize("w,h", R.SIZES)
def test_cases_cover_what_they_are_for(w, h):
    from test_gpu_subpel import assert_coverage
    luma, chroma = case_counts(w, h)
    assert_coverage(w, h, luma, chroma)
    if (w, h) == (32, 32):                                                  # every luma class reaches both clips and a negative v
        filtered = luma.samples > 0
        filtered[0, 0] = False                                              # the gather has nothing to clip
        assert (luma.below[filtered] > 0).all() and (luma.above[filtered] > 0).all() and (luma.negative_v[1:, 1:] > 0).all(), luma
