"""CPU: the reference statement of the seeded SATD search (tests/_seeded_ref.py) against the numbers of include/x266hip.h, against the
oracle's exhaustive search and the quarter-sample statement, and -- what the call is for -- on a translated texture through the whole
hierarchy: reference downscale, the oracle's +-32 search of the half-size pair, the seeded walk around the doubled winners."""
import functools

import numpy as np
import pytest

import _seeded_ref as R
import _subpel_ref as S
from _la_ref import box


def test_the_code_lengths_of_the_header():
    want = {0: 1, 1: 3, -1: 3, 2: 5, -2: 5, 3: 5, -3: 5, 4: 7, -7: 7, 8: 9, 16382: 29, -16382: 29}
    assert {d: R.code_length(d) for d in want} == want
    assert max(R.code_length(d) for d in range(-16382, 16383)) == 29
    assert [R.code_length(d) for d in range(-4, 5)] == [7, 5, 5, 3, 1, 3, 5, 5, 7]
    # lambda_q4 16: the predictor 2, one sample off 4, (2, -4) off 12
    assert [R.vector_cost(16, v, (5, -3)) for v in ((5, -3), (6, -3), (7, -7))] == [2, 4, 12]
    assert R.vector_cost(0, (100, 100), (0, 0)) == 0 and R.vector_cost(65535, (8191, -8191), (-8191, 8191)) == (65535 * 58) >> 4 < 1 << 18


def test_the_clamp_at_the_int16_extremes():
    for scale in (0, 1):
        assert R.clamp_seed(-32768, scale) == -8183 and R.clamp_seed(32767, scale) == 8183
        assert R.clamp_seed(0, scale) == 0 and R.clamp_seed(-3, scale) == -3 << scale
    assert [R.clamp_seed(v, 0) for v in (8183, 8184, -8183, -8184, 8191)] == [8183, 8183, -8183, -8183, 8183]
    assert [R.clamp_seed(v, 1) for v in (4091, 4092, -4091, -4092, 64)] == [8182, 8183, -8182, -8183, 128]


def test_the_centre_list_at_corners_and_edges():
    gw, gh = 3, 2
    seeds = [(10 * (i % gw) + 1, 10 * (i // gw) + 2) for i in range(gw * gh)]
    S0 = lambda x, y: seeds[y * gw + x]
    L = lambda sx, sy, c: R.centre_list(seeds, gw, gh, sx, sy, 0, c)
    assert L(0, 0, 31) == [S0(0, 0), (0, 0), S0(1, 0), S0(0, 1)]              # top-left: no left, no top
    assert L(2, 0, 31) == [S0(2, 0), (0, 0), S0(1, 0), S0(2, 1)]              # top-right: no top, no right
    assert L(0, 1, 31) == [S0(0, 1), (0, 0), S0(0, 0), S0(1, 1)]              # bottom-left: no left, no bottom
    assert L(2, 1, 31) == [S0(2, 1), (0, 0), S0(1, 1), S0(2, 0)]              # bottom-right
    assert L(1, 0, 31) == [S0(1, 0), (0, 0), S0(0, 0), S0(2, 0), S0(1, 1)]    # the top edge: everything but top
    assert L(1, 1, 31) == [S0(1, 1), (0, 0), S0(0, 1), S0(1, 0), S0(2, 1)]
    assert L(1, 0, 0) == [S0(1, 0)]
    for bit, want in ((1, (0, 0)), (2, S0(0, 0)), (4, None), (8, S0(2, 0)), (16, S0(1, 1))):
        assert L(1, 0, bit) == [S0(1, 0)] + ([want] if want else []), bit
    assert R.centre_list([(7, -7)], 1, 1, 0, 0, 0, 31) == [(7, -7), (0, 0)]   # one cell: every neighbour is skipped
    # seed_scale 1: the seeds are doubled, then clamped
    assert R.centre_list([(5000, -3), (-32768, 32767)], 2, 1, 0, 0, 1, 8) == [(8183, -6), (-8183, 8183)]
    assert R.grid(96, 80, 0) == (12, 10) and R.grid(96, 80, 1) == (6, 5)


def test_the_walk_order():
    w = R.walk([(5, -3), (0, 0)], 1)
    assert len(w) == 18 and w[:4] == [(4, -4), (5, -4), (6, -4), (4, -3)] and w[4] == (5, -3) and w[8] == (6, -2)
    assert w[9] == (-1, -1) and w[13] == (0, 0) and w[17] == (1, 1)
    assert R.walk([(2, 2)], 0) == [(2, 2)] and len(R.walk([(0, 0)] * 6, 8)) == 6 * 289
    assert R.walk([(1, 1), (1, 1)], 0) == [(1, 1), (1, 1)]                    # duplicates are allowed


@functools.lru_cache(None)
def _pair(w, h):
    return R.frame_pair("random", w, h, 3)


@pytest.mark.parametrize("w,h", [(16, 16), (48, 32)])
def test_a_zero_seed_is_the_exhaustive_search_at_range_8(oracle, w, h):
    """consequence 1 of the header, against the oracle's brute-force search on the edge-padded plane"""
    cur, ref = _pair(w, h)
    nb = (w // 8) * (h // 8)
    best, j, _ = R.search(oracle, cur, ref, np.zeros((nb, 2), np.int16), 0, 0, 8, 0)
    mv, cost, _ = oracle.satd_search(cur, np.pad(ref, 8, mode="edge"), 8, 8)
    assert np.array_equal(best["mvx"], mv[:, 0]) and np.array_equal(best["mvy"], mv[:, 1]) and np.array_equal(best["cost"], cost)
    assert np.array_equal(j, cost)


def test_range_0_gives_the_clamped_seed_and_the_refinements_centre_cost(oracle):
    """consequence 2: entry [49 b + 24] of the quarter-sample refinement's cost map for the same vector"""
    w, h = 32, 16
    cur, ref = _pair(w, h)
    for scale in (0, 1):
        seeds = R.seed_vectors("small", w, h, scale, 5)
        seeds[0] = (-32768, 32767)
        best, j, _ = R.search(oracle, cur, ref, seeds, scale, 0, 0, 200)
        gw = R.grid(w, h, scale)[0]
        cell = np.array([(b // (w // 8) >> scale) * gw + (b % (w // 8) >> scale) for b in range(best.size)])
        want = np.clip(seeds.astype(np.int64)[cell] << scale, -8183, 8183)
        assert np.array_equal(best["mvx"], want[:, 0]) and np.array_equal(best["mvy"], want[:, 1])
        costs = S.refine(oracle, cur, ref, want)[2]
        assert np.array_equal(best["cost"], costs[:, 24])
        assert np.array_equal(j, best["cost"] + ((200 * 2) >> 4))            # the predictor costs L(0) + L(0)


def test_constant_frames_tie(oracle):
    """every SATD ties: lambda 0 -> the first entry of the walk, own + (-r, -r); lambda > 0 -> the predictor"""
    w, h = 32, 16
    cur, ref = R.frame_pair("constant", w, h, 0)
    seeds = R.seed_vectors("small", w, h, 0, 9)
    for centres in (0, 31):
        first, _, index = R.search(oracle, cur, ref, seeds, 0, centres, 2, 0)
        assert not index.any() and np.array_equal(first["mvx"], seeds[:, 0] - 2) and np.array_equal(first["mvy"], seeds[:, 1] - 2) and not first["cost"].any()
        pred, j, index = R.search(oracle, cur, ref, seeds, 0, centres, 2, 16)
        assert (index == 12).all() and np.array_equal(pred["mvx"], seeds[:, 0]) and np.array_equal(pred["mvy"], seeds[:, 1]) and (j == 2).all()


# ---- what the call is for ---------------------------------------------------------------------------------------------------------------------
W, H, MARGIN = 160, 128, 48


@functools.lru_cache(None)
def _texture():
    return R.smooth_texture(W + 2 * MARGIN, H + 2 * MARGIN, 0x7E87)


@pytest.mark.parametrize("mv", [(38, -22), (37, -21)])
def test_the_hierarchy_finds_a_translation(oracle, mv):
    """the current frame is the reference translated by mv: cur(x, y) = ref(x + mvx, y + mvy).  Downscale both, search the half-size
    pair at +-32, walk around the doubled winners (centres 31, r = 2, lambda 0): every block whose displaced lowres block lies inside
    the frame gets exactly mv with SATD 0.  (38, -22) is exact by construction, even shifts commute with the 2x2 mean; for (37, -21) the
    truth lies within +-2 of every doubled lowres winner near it."""
    big = _texture()
    ref = big[MARGIN:MARGIN + H, MARGIN:MARGIN + W]
    cur = big[MARGIN + mv[1]:MARGIN + mv[1] + H, MARGIN + mv[0]:MARGIN + mv[0] + W]
    cur_low, ref_low = box(cur), box(ref)
    low_mv, low_cost, _ = oracle.satd_search(cur_low, np.pad(ref_low, 32, mode="edge"), 32, 32, threads=4)
    best, j, _ = R.search(oracle, cur, ref, low_mv, 1, 31, 2, 0)
    assert np.array_equal(j, best["cost"])                                    # lambda 0
    bw = W // 8
    lx, ly = mv[0] / 2.0, mv[1] / 2.0
    inside = np.array([0 <= 8 * ((b % bw) >> 1) + np.floor(lx) and 8 * ((b % bw) >> 1) + np.ceil(lx) + 7 <= W // 2 - 1 and
                       0 <= 8 * ((b // bw) >> 1) + np.floor(ly) and 8 * ((b // bw) >> 1) + np.ceil(ly) + 7 <= H // 2 - 1 for b in range(best.size)])
    assert inside.sum() >= best.size // 2
    hit = (best["mvx"] == mv[0]) & (best["mvy"] == mv[1]) & (best["cost"] == 0)
    print("translation %s: %d of %d blocks inside, %d of them exact, lowres winners %s" %
          (mv, inside.sum(), best.size, (hit & inside).sum(), sorted(set(map(tuple, low_mv[inside.reshape(H // 8, bw)[::2, ::2].ravel()].tolist())))))
    assert hit[inside].all(), np.flatnonzero(inside & ~hit)[:10]
