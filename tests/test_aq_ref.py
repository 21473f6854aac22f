"""CPU: the numpy restatement of the source analysis (tests/_aq_ref.py) against the values include/x266hip.h states, against floating
point and exact rational arithmetic, and -- through the built library, no GPU -- xWeightsFromTotals against it."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import _aq_ref as R


def test_known_values_of_the_logarithm():
    got = R.log2_q8(np.array([0, 1, 2, 3, 5, 1000, 6242400])).tolist()
    assert got == [0, 0, 256, 405, 594, 2551, 5778], got


def test_the_logarithm_is_the_floor_of_256_log2():
    e = np.arange(1, 200001)
    got = R.log2_q8(e)
    err = 256.0 * np.log2(e.astype(np.float64)) - got
    assert err.min() > -1e-9 and err.max() < 1.0, (err.min(), err.max())
    for x in (1, 2, 3, 7, 1023, 1024, 1025, 65535, 199999, 6242400, 2 ** 32 - 1):   # exact: 2^L <= e^256 < 2^(L + 1)
        L = int(R.log2_q8(np.array([x]))[0])
        assert 2 ** L <= x ** 256 < 2 ** (L + 1), x
    assert (np.diff(got) >= 0).all()


def test_the_three_rounding_cases_of_delta():
    for n in (1, 3, 4, 16):
        assert R.delta(-128 * n, n) == 0 and R.delta(-129 * n, n) == -1 and R.delta(128 * n, n) == 1
        assert R.delta(127 * n, n) == 0 and R.delta(-3072 * n, n) == -12 and R.delta(3072 * n, n) == 12
    assert R.delta(0, 0) == 0 and R.delta(-1, 3) == 0
    for s in range(-700, 700, 7):                                            # the mean, rounded half up, exactly
        assert R.delta(s, 3) == math.floor(Fraction(s, 3 * 256) + Fraction(1, 2)), s


def test_the_uint32_edge_and_the_maximum_energy():
    rec = R.tile_stats(R.constant_frame(16, 16, 255))
    assert int(rec["sum_y"][0]) == 65280 and int(rec["sum_y"][0]) ** 2 > 2 ** 31         # fits uint32, not int32
    assert int(rec["ssq_y"][0]) == 256 * 65025 and int(rec["energy"][0]) == 0 and int(rec["log2_q8"][0]) == 0
    rec = R.tile_stats(R.max_energy_frame(32, 16))
    assert rec["energy"].tolist() == [R.MAX_ENERGY] * 2 and rec["log2_q8"].tolist() == [5778] * 2
    assert rec["sum_y"].tolist() == [128 * 255] * 2 and rec["sum_u"].tolist() == [32 * 255] * 2 and rec["sum_v"].tolist() == [32 * 255] * 2
    # no other split of a plane into 0 and 255 gives more: the energy of k samples of 255 among n is 65025 k (n - k) / n
    assert max(65025 * k - ((255 * k) ** 2 >> 8) for k in range(257)) == 4161600


def test_records_against_plain_loops():
    t = R.noise_frame(48, 32, 3)
    rec = R.tile_stats(t)
    for i in (0, 2, 5):
        y, c = t[i, :256].astype(int).tolist(), t[i, 256:384].astype(int).tolist()
        u, v = c[0::2], c[1::2]
        want = [sum(y), sum(a * a for a in y), sum(u), sum(a * a for a in u), sum(v), sum(a * a for a in v)]
        assert [int(rec[n][i]) for n in R.TILE_DTYPE.names[:6]] == want
        e = (want[1] - (want[0] ** 2 >> 8)) + (want[3] - (want[2] ** 2 >> 6)) + (want[5] - (want[4] ** 2 >> 6))
        assert int(rec["energy"][i]) == e
    other = t.copy()
    other[:, 384:] ^= 0xFF                                                   # m_I is not read
    assert np.array_equal(R.tile_stats(other), rec)
    tot = R.totals(rec)
    assert tot[7] == 6 and tot[0] == int(t[:, :256].astype(int).sum()) and tot[6] == int(rec["log2_q8"].astype(int).sum())


def test_the_qp_map_of_a_cut_frame():
    w, h = 48, 80                                                            # 3 x 5 tiles: CTUs cut in both directions
    rec = R.tile_stats(R.halves_frame(w, h, 11))
    tot = R.totals(rec)
    off1, qp1 = R.decide(rec, tot, w, h, 1, 256, 30, 0)
    off2, qp2 = R.decide(rec, tot, w, h, 2, 256, 30, 0)
    assert qp1.size == 12 and not np.array_equal(off1, off2)
    d = qp2.astype(int) - 30
    assert d.min() < 0 < d.max()                                             # the flat half is coded finer, the textured one coarser
    _, flat = R.decide(rec, tot, w, h, 2, 0, 30, 0)
    assert (flat == 30).all()                                                # strength 0: every qp is the base
    # CTU 0 by hand: quadrant 1 has the single column tx = 2, the chroma regions all 12 tiles of the CTU
    o = off2.astype(int).reshape(5, 3)
    assert int(qp2[1]) == 30 + R.delta(int(o[0:2, 2].sum()), 2) and int(qp2[4]) == 30 + R.delta(int(o[0:4].sum()), 12) and qp2[4] == qp2[5]
    # CTU 1 (the second row of CTUs) holds tile row 4 alone: quadrants 2 and 3 are outside the frame and keep the base qp
    assert qp2[6 + 2] == 30 and qp2[6 + 3] == 30 and int(qp2[6]) == 30 + R.delta(int(o[4, 0:2].sum()), 2)
    _, lo = R.decide(rec, tot, w, h, 1, 1024, 0, -12)
    _, hi = R.decide(rec, tot, w, h, 1, 1024, 51, 12)
    assert lo.min() == 0 and hi.max() == 51 and (lo[4::6] == 0).all() and (hi[4::6] == 51).all()


def _exact(cur_planes, ref_planes, d):
    """w and o from the definition in rational arithmetic: w = round-half-up of 2^d sqrt(var_cur / var_ref) via the integer square
    root of the header, o = floor(mean_cur - mean_ref w / 2^d + 1 / 2)"""
    out = []
    for c, r in zip(cur_planes, ref_planes):
        c, r = [int(x) for x in c.ravel()], [int(x) for x in r.ravel()]
        n = len(c)
        var_c, var_r = n * sum(x * x for x in c) - sum(c) ** 2, n * sum(x * x for x in r) - sum(r) ** 2
        w = 1 << d if var_r == 0 else (math.isqrt(Fraction(var_c << (2 * d + 2), var_r).__floor__()) + 1) >> 1
        w = min(max(w, 1), 127)
        o = math.floor(Fraction(sum(c), n) - Fraction(sum(r) * w, n << d) + Fraction(1, 2))
        out.append((w, min(max(o, -128), 127)))
    return out


def _planes(tiles):
    t = np.asarray(tiles).reshape(-1, 512)
    return t[:, :256], t[:, 256:384:2], t[:, 257:384:2]


def _fade_pair(w=64, h=48, seed=21):
    ref = R.noise_frame(w, h, seed)
    cur = ref.copy()
    cur[:, :384] = ((ref[:, :384].astype(np.int64) * 96 + 64) >> 7) + 10
    return cur, ref


def test_fade_weights_against_rational_arithmetic():
    cur, ref = _fade_pair()
    tc, tr = R.totals(R.tile_stats(cur)), R.totals(R.tile_stats(ref))
    w, o = R.weights(tc, tr, (7, 7))
    assert list(zip(w, o)) == _exact(_planes(cur), _planes(ref), 7)
    assert w == [96, 96, 96] and all(9 <= x <= 11 for x in o), (w, o)         # the fade that was applied: 96 / 128 and +10
    # identity totals with denominator 6
    assert R.weights(tr, tr, (6, 6)) == ([64] * 3, [0] * 3)
    # a flat reference has no variance to scale: w = 1 << d, and o carries the whole difference of the means
    flat, flat2 = R.totals(R.tile_stats(R.constant_frame(32, 32, 100))), R.totals(R.tile_stats(R.constant_frame(32, 32, 131)))
    assert R.weights(flat2, flat, (5, 3)) == ([32, 8, 8], [31] * 3)
    assert R.weights(tc, flat, (7, 7))[0] == [128 - 1] * 3                    # 1 << 7, clamped to 127
    # the clamps of o
    black, white = R.totals(R.tile_stats(R.constant_frame(16, 16, 0))), R.totals(R.tile_stats(R.constant_frame(16, 16, 255)))
    assert R.weights(white, black, (0, 0)) == ([1] * 3, [127] * 3) and R.weights(black, white, (0, 0)) == ([1] * 3, [-128] * 3)


def test_weights_at_8k_pass_64_bits():
    n_tiles = (7680 // 16) * (4320 // 16)
    ref = np.array([n_tiles * 256 * 128, n_tiles * 256 * 128 * 128 + n_tiles * 256 * 3000, n_tiles * 64 * 100, n_tiles * 64 * 10900, n_tiles * 64 * 90,
                    n_tiles * 64 * 9000, 0, n_tiles], np.int64)
    assert int(ref[1]) * n_tiles * 256 > 2 ** 63
    assert R.weights(ref, ref, (7, 7)) == ([128 - 1] * 3, [1, 1, 1])         # w clamps to 127: o makes up the missing 1 / 128 of the mean
    assert R.weights(ref, ref, (6, 6)) == ([64] * 3, [0] * 3)


# ---- the library's host call against the restatement (needs the built library, no GPU) ------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import x266_amd
    x266_amd.build_library()
    return x266_amd.load_library()


def _call(lib, cur, ref, lst, log2_denom):
    import x266_amd
    wp = x266_amd.Codec.wp_params(w=((-5, -5, -5), (-6, -6, -6)), o=((77, 77, 77), (78, 78, 78)), log2_denom=log2_denom)
    c, r = np.ascontiguousarray(cur, np.int64), np.ascontiguousarray(ref, np.int64)
    rc = lib.xWeightsFromTotals(c.ctypes.data, r.ctypes.data, lst, ctypes.byref(wp))
    return rc, wp


def test_the_host_call_matches_the_restatement(lib):
    cur, ref = _fade_pair()
    tc, tr = R.totals(R.tile_stats(cur)), R.totals(R.tile_stats(ref))
    n8k = (7680 // 16) * (4320 // 16)
    big = np.array([n8k * 256 * 128, n8k * 256 * 128 * 128 + n8k * 256 * 3000, n8k * 64 * 100, n8k * 64 * 10900, n8k * 64 * 90, n8k * 64 * 9000, 0, n8k], np.int64)
    big2 = big.copy()
    big2[1] += n8k * 256 * 1000
    flat, white = R.totals(R.tile_stats(R.constant_frame(64, 48, 100))), R.totals(R.tile_stats(R.constant_frame(64, 48, 255)))
    for c, r in ((tc, tr), (tr, tc), (tr, tr), (big, big), (big2, big), (big, big2), (tc, flat), (flat, tc), (white, flat), (flat, white)):
        for denom in ((7, 7), (6, 6), (0, 3), (5, 0)):
            for lst in (0, 1):
                rc, wp = _call(lib, c, r, lst, denom)
                assert rc == 0
                w, o = R.weights(c, r, denom)
                assert [wp.w[lst][i] for i in range(3)] == w and [wp.o[lst][i] for i in range(3)] == o, (denom, lst)
                other = 1 - lst                                             # the other list and the denominators are left alone
                assert [wp.w[other][i] for i in range(3)] == [-6 + lst] * 3 and [wp.o[other][i] for i in range(3)] == [78 - lst] * 3
                assert (wp.log2_denom[0], wp.log2_denom[1]) == denom


def test_the_host_call_refuses(lib):
    import x266_amd
    tr = R.totals(R.tile_stats(R.noise_frame(32, 32, 5)))
    assert _call(lib, tr, tr, 0, (7, 7))[0] == 0
    assert _call(lib, tr, tr, 2, (7, 7))[0] == -1 and _call(lib, tr, tr, -1, (7, 7))[0] == -1
    assert _call(lib, tr, tr, 0, (8, 7))[0] == -1 and _call(lib, tr, tr, 0, (7, 8))[0] == -1
    other = tr.copy()
    other[7] += 1
    assert _call(lib, tr, other, 0, (7, 7))[0] == -1                          # two frames of different sizes
    none = tr.copy()
    none[7] = 0
    assert _call(lib, none, none, 0, (7, 7))[0] == -1
    wp = x266_amd.Codec.wp_params()
    assert lib.xWeightsFromTotals(None, tr.ctypes.data, 0, ctypes.byref(wp)) == -1
    assert lib.xWeightsFromTotals(tr.ctypes.data, None, 0, ctypes.byref(wp)) == -1
    assert lib.xWeightsFromTotals(tr.ctypes.data, tr.ctypes.data, 0, None) == -1
    with pytest.raises(x266_amd.X266Error):
        x266_amd.Codec.weights_from_totals(tr, other)
    got = x266_amd.Codec.weights_from_totals(tr, tr, 1, (6, 6))
    assert [got.w[1][i] for i in range(3)] == [64] * 3 and [got.w[0][i] for i in range(3)] == [64] * 3 and got.log2_denom[1] == 6
