"""CPU: the numpy statement of rate-distortion optimised quantisation (tests/_rdoq_ref.py) against cases worked by hand from the text of
include/x266hip.h, one rule at a time; the rate tables against values written out by hand; `bits` from the levels alone; the host
helpers xLevelBits, xLastPosBits and xCgFlagBits of the built library against the reference's tables.  No GPU.

Most hand-worked cases use a 32x32 block at qp 4: f = 16384 and qbits = 16, so x = a * 2^14, e = 64 |a - 4 l| exactly and
D(l) = 4096 (a - 4 l)^2."""
import numpy as np
import pytest

import _levels_ref as lref
import _rdoq_ref as ref


def block(n, **at):
    """an all-zero block of 1 << n in scan order with coefficients at the given scan indices: block(5, p0=4, p2=-4)"""
    c = np.zeros(1 << (2 * n), np.int64)
    for key, v in at.items():
        c[int(key[1:])] = v
    return c


# ---- the tables -----------------------------------------------------------------------------------------------------------------------
def test_level_rates_by_hand():
    # l:                 0   1   2   3    4    5    6    7    8    9
    want = {0: [24, 36, 61, 88, 104, 120, 136, 168, 168, 200],
            1: [12, 48, 73, 100, 116, 132, 148, 180, 180, 212],
            2: [6, 62, 87, 114, 130, 146, 162, 194, 194, 226]}
    for cls, row in want.items():
        assert [ref.level_bits(l, cls) for l in range(10)] == row
    # rem(13105) = 3 + 2 * 13 + 1 = 30: the largest level the optimisation can emit, and the largest magnitude of an int16
    assert ref.level_bits(13108, 2) == 36 + 16 + 24 + 22 + 16 * 30 == 578
    assert ref.level_bits(32768, 2) == 36 + 16 + 24 + 22 + 16 * 32
    assert [ref.rem_bits(r) for r in range(8)] == [1, 2, 3, 4, 6, 6, 8, 8]
    assert [ref.cg_flag_bits(0), ref.cg_flag_bits(1)] == [9, 26]


def test_last_position_rates_by_hand():
    pos4 = [1, 2, 3, 3]                                                      # n = 2: the prefix is capped at 2 n - 1 = 3
    pos32 = [1, 2, 3, 4, 6, 6, 7, 7, 9, 9, 9, 9, 10, 10, 10, 10] + [12] * 16  # n = 5: g = 8 and 9 both give 9 + 3
    assert [ref.pos_bits(t, 2) for t in range(4)] == pos4
    assert [ref.pos_bits(t, 5) for t in range(32)] == pos32
    for n, pos in ((2, pos4), (5, pos32)):
        for u in range(1 << n):
            for v in range(1 << n):
                assert ref.last_pos_bits(u, v, n) == 16 * (pos[u] + pos[v])
    assert ref.last_pos_bits(0, 0, 5) == 32 and ref.last_pos_bits(31, 31, 5) == 384 and ref.last_pos_bits(3, 3, 2) == 96


def test_position_classes_follow_the_scan():
    for n in (2, 3, 4, 5):
        off, cls, rlast = ref._block_geometry(n)
        assert np.array_equal(off, lref.scan(1 << n))
        assert cls[0] == 0 and (cls[1:16] == 1).all() and (cls[16:] == 2).all()   # CG 0 is the first 16 scan positions


# ---- step 1 -----------------------------------------------------------------------------------------------------------------------------
def test_step1_tie_takes_the_smaller_level():
    """DC, a = 5: h = (5 * 2^14 + 2^15) >> 16 = 1.  J(1) = 4096 + 36 lambda, J(0) = 4096 * 25 + 24 lambda: equal at lambda = 8192
    (299008 both), and then 0 wins; at 8191 level 1 is cheaper by 12."""
    assert ref.rdoq_block(block(5, p0=5), 5, 4, 8192, steps=1)[0][0] == 0
    assert ref.rdoq_block(block(5, p0=5), 5, 4, 8191, steps=1)[0][0] == 1
    assert ref.rdoq_block(block(5, p0=-5), 5, 4, 8191, steps=1)[0][0] == -1   # the sign is the coefficient's
    # lambda = 0, a = 6 outside CG 0: h = 2, D(2) = D(1) = 4096 * 4: a tie between h and h - 1
    lv, _, _, changed, _, _ = ref.rdoq_block(block(5, p16=6), 5, 4, 0, steps=1)
    assert lv[16] == 1 and changed == 1


def test_step1_candidates():
    """a = 13 outside CG 0, lambda 368: h = 3; candidates 3 and 2 only (0 is none at h = 3).  D(3) = 4096, D(2) = 4096 * 25;
    J(3) = 4096 + 368 * 114 = 46048 < J(2) = 102400 + 368 * 87 = 134416.  a = 9: h = 2, J(2) = 4096 + 32016, J(1) = 102400 + 22816,
    J(0) = 331776 + 2208."""
    assert ref.rdoq_block(block(5, p16=13), 5, 4, 368, steps=1)[0][16] == 3
    assert ref.rdoq_block(block(5, p16=9), 5, 4, 368, steps=1)[0][16] == 2
    # a = 2: h = 1 exactly at the half; J(1) = 4096 * 4 + 62 lambda against J(0) = 4096 * 4 + 6 lambda: 0 for every lambda, 0 included
    for lam in (0, 1, 368):
        assert ref.rdoq_block(block(5, p16=2), 5, 4, lam, steps=1)[0][16] == 0


# ---- step 2 -----------------------------------------------------------------------------------------------------------------------------
def test_step2_equality_stays_coded():
    """32x32 at qp 9 (f = 18396, qbits = 17), a = 23 at the first position of CG 1, lambda = 3072.  x = 423108, h = 3.
    D(3): err = 29892, e = (29892 + 256) >> 9 = 58, D = 3364.  D(2): err = 160964, e = 314, D = 98596.  D(0): e = 826, D = 682276.
    J(3) = 3364 + 3072 * 114 = 353572 < J(2) = 98596 + 3072 * 87 = 365860, so q = 3.
    Jc = 353572 + 15 * 6 * 3072 + 26 * 3072 = 709924;  Jz = 682276 + 9 * 3072 = 709924: equal, the CG stays.  At lambda = 3073 Jc grows
    by 221 and Jz by 9: the CG goes."""
    lv, _, _, _, zeroed, _ = ref.rdoq_block(block(5, p16=23), 5, 9, 3072, steps=2)
    assert lv[16] == 3 and zeroed == 0
    lv, _, _, _, zeroed, _ = ref.rdoq_block(block(5, p16=23), 5, 9, 3073, steps=2)
    assert lv[16] == 0 and zeroed == 1
    # CG 0 is never touched here: the same coefficient at DC's neighbour stays at any lambda that keeps level 3 in step 1
    lv, _, _, _, zeroed, _ = ref.rdoq_block(block(5, p1=23), 5, 9, 3073, steps=2)
    assert lv[1] == 3 and zeroed == 0


# ---- step 3 -----------------------------------------------------------------------------------------------------------------------------
def test_step3_tie_keeps_the_larger_position():
    """qp 4, lambda 1024, a = 4 at DC and at scan position 2 (u = 1, v = 0): both q = 1 with D(1) = 0, D(0) = 65536.
    Total(0) = 0 + 1024 * (36 - 10) + 65536 + 1024 * 16 * (1 + 1) = 124928.
    Total(2) = J(q[0]) + J(q[1]) + 0 + 1024 * (48 - 22) + 0 + 1024 * 16 * (2 + 1) = 36864 + 12288 + 26624 + 49152 = 124928.
    Total(none) = 131072.  The tie goes to p = 2."""
    totals = {}
    lv, dist, bits, _, _, moved = ref.rdoq_block(block(5, p0=4, p2=4), 5, 4, 1024, totals=totals)
    assert totals == {0: 124928, 2: 124928, None: 131072}
    assert lv[:4].tolist() == [1, 0, 1, 0] and moved == 0 and dist == 0
    assert bits == 48 + (36 + 12 + 48) - 22                                 # Rlast(1, 0) + R of positions 0, 1, 2 - sig[1][1]
    # at lambda = 1025 Total(0) = 1025 * 58 + 65536 = 124986 < Total(2) = 1025 * 122 = 125050: the last position moves in
    lv, _, _, _, _, moved = ref.rdoq_block(block(5, p0=4, p2=4), 5, 4, 1025)
    assert lv[:4].tolist() == [1, 0, 0, 0] and moved == 1


def test_step3_a_block_goes_to_none():
    """qp 4, lambda 8192, a = 6 at DC: h = 2, J(2) = 16384 + 61 * 8192, J(1) = 16384 + 36 * 8192 = 311296, J(0) = 147456 + 24 * 8192 = 344064:
    q = 1.  Total(0) = 16384 + 8192 * 26 + 0 + 8192 * 32 = 491520 > Total(none) = 147456: every level goes."""
    totals = {}
    lv, dist, bits, changed, _, moved = ref.rdoq_block(block(5, p0=6), 5, 4, 8192, totals=totals)
    assert totals == {0: 491520, None: 147456}
    assert not lv.any() and moved == 1 and changed == 1 and dist == 147456 and bits == 0
    # equality goes to p: Total(p) = Total(none) keeps the level.  a = 4 at DC, lambda = 65536 / 58 is no integer, so a 4x4 at qp 4
    # (qbits = 19, level = a / 32): a = 32, D(1) = 0, D(0) = 65536, Total(0) = lambda * (26 + 32) -- 1129 * 58 = 65482 <= 65536 < 1130 * 58
    assert ref.rdoq_block(block(2, p0=32), 2, 4, 1129)[0][0] == 1
    assert ref.rdoq_block(block(2, p0=32), 2, 4, 1130)[0][0] == 0


# ---- the region call ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0, 368, 8192])
def test_bits_follow_from_the_levels_alone(lam):
    cls = np.array([3, 2, 1, 0, 7, 254], np.uint8)
    qps = np.array([32, 22, 37, 0, 51, 200], np.uint8)
    coef = ref.laplacian(6, cls, qps, 0, 3.0, seed=77)
    lv, stat, counters = ref.rdo_quant(coef, cls, qps, 0, lam)
    again = ref.levels_bits(lv, cls)
    assert np.array_equal(again["bits"], stat["bits"]) and np.array_equal(again["n_nz"], stat["n_nz"]) and not again["dist"].any()
    assert np.array_equal(stat["n_nz"], np.count_nonzero(lv, axis=1))
    assert (np.sign(lv) * np.sign(coef) >= 0).all()                          # signs are the coefficients'
    if lam:
        assert counters["changed"] and counters["cg_zeroed"] and counters["last_moved"]
    # 4x4 blocks have a single CG: step 2 never fires there
    assert ref.rdo_quant(coef[3:4], cls[3:4], qps[3:4], 0, 368)[2]["cg_zeroed"] == 0
    # a region with a zero count reports zeros
    counts = stat["n_nz"].copy()
    counts[2] = 0
    assert ref.levels_bits(lv, cls, counts)[2].tolist() == (0, 0, 0)


def test_lambda_zero_is_round_to_nearest_up_to_ties():
    import _quant_ref as qref
    coef = ref.laplacian(4, None, None, 30, 3.0, seed=5)
    lv, stat, _ = ref.rdo_quant(coef, None, None, 30, 0)
    nearest, _ = qref.quant_regions(coef, False, None, None, 30, 256)
    diff = np.abs(lv.astype(np.int64)) - np.abs(nearest.astype(np.int64))
    assert ((diff == 0) | (diff == -1)).all() and np.count_nonzero(diff) < 82      # a tie needs both errors within 1/256 of a level of the half


# ---- the host helpers of the built library ----------------------------------------------------------------------------------------------------
def test_host_helpers_against_the_reference():
    import x266_amd
    x266_amd.build_library()
    L = x266_amd.load_library()
    for cls in range(3):
        for l in list(range(0, 300)) + [1000, 4098, 4099, 13108, 32767, 32768]:
            assert L.xLevelBits(l, cls) == ref.level_bits(l, cls) == x266_amd.level_bits(l, cls), (l, cls)
    for n in range(2, 6):
        for u in range(1 << n):
            for v in range(1 << n):
                assert L.xLastPosBits(u, v, n) == ref.last_pos_bits(u, v, n), (u, v, n)
    assert [L.xCgFlagBits(0), L.xCgFlagBits(1)] == [9, 26] and x266_amd.Codec.cg_flag_bits(1) == 26
    assert x266_amd.last_pos_bits(31, 31, 5) == 384
    for bad in ((-1, 0), (32769, 0), (0, -1), (0, 3)):
        assert L.xLevelBits(*bad) == -1
    for bad in ((0, 0, 1), (0, 0, 6), (4, 0, 2), (0, 4, 2), (-1, 0, 5), (0, 32, 5)):
        assert L.xLastPosBits(*bad) == -1
    assert L.xCgFlagBits(2) == -1 and L.xCgFlagBits(-1) == -1
    with pytest.raises(x266_amd.X266Error):
        x266_amd.level_bits(5, 3)


def test_host_helpers_reproduce_bits():
    """a host coder walks xLevelScan and adds up the three helpers: the region's `bits`"""
    import x266_amd
    x266_amd.build_library()
    cls = np.array([3, 1], np.uint8)
    coef = ref.laplacian(2, cls, None, 30, 3.0, seed=9)
    lv, stat, _ = ref.rdo_quant(coef, cls, None, 30, 368)
    for r in range(2):
        n = 2 + int(cls[r])
        size = 1 << n
        order = x266_amd.level_scan(size)
        total = 0
        for b in range(1024 // (size * size)):
            mag = np.abs(lv[r, b * size * size + order].astype(np.int64))
            nz = np.flatnonzero(mag)
            if nz.size == 0:
                continue
            p = int(nz[-1])
            pos_class = lambda i: 0 if i == 0 else 1 if i < 16 else 2
            total += x266_amd.last_pos_bits(int(order[p]) % size, int(order[p]) // size, n) - (x266_amd.level_bits(1, pos_class(p)) - 16 - 10)
            for s in range(p // 16 + 1):
                coded = bool(mag[16 * s:16 * s + 16].any())
                if 0 < s < p // 16:
                    total += x266_amd.cg_flag_bits(coded)
                if s == 0 or s == p // 16 or coded:
                    total += sum(x266_amd.level_bits(int(mag[i]), pos_class(i)) for i in range(16 * s, min(16 * s + 15, p) + 1))
        assert total == int(stat["bits"][r])


# ---- the wide content of the fuzz list ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["heavy_head", "heavy_cg"])
def test_wide_content_is_int16_wide_at_its_qp_and_seeded(kind):
    """tests/_frame_cases.py's two recipes: every block they make heavy has a sum of D(0) of 2^32 and more at the class and qp the call
    will use for its region; "heavy_cg" puts the low dword of its CG's sum as low as the CG's last magnitude can"""
    import _frame_cases as F
    import _quant_ref as qref
    cases = [c for c in F.cases("rdoq", 1) if c["kind"] == kind]
    assert len(cases) >= 4 and all(0 <= c["qp"] <= F.wide_qp(2, c["mag"][0]) for c in cases)
    assert [F.wide_qp(n, 20000) for n in (2, 3, 4, 5)] == [11, 17, 23, 29]      # D(0) = ((20000 f + 2^(qbits - 9)) >> (qbits - 8))^2 >= 2^32
    for c in cases:
        coef, cls, qps = F.rdoq_content(c)
        again = F.rdoq_content(c)
        assert coef.dtype == np.int16 and all(np.array_equal(a, b) for a, b in zip((coef, cls, qps), again))
        assert not np.array_equal(coef, F.rdoq_content(dict(c, seed=c["seed"] + 1))[0])
        n_of = qref.region_n(None if "d_class" in c["null"] else cls, coef.shape[0])
        qp_of = qref.region_qp(None if "d_qp" in c["null"] else qps, c["qp"], coef.shape[0])
        lo, hi = c["mag"]
        for r in range(coef.shape[0]):
            n, qb, f = int(n_of[r]), int(qref.qbits(n_of[r], qp_of[r])), int(qref.F[qp_of[r] % 6])
            if kind == "heavy_cg" and n == 2:
                continue
            for idx in ref._region_blocks(n - 2):
                d0 = ref.dist(np.abs(coef[r, idx].astype(np.int64)) * f, 0, qb)
                assert int(d0.sum()) >= 1 << 32, (F.tag(c), r)
                heavy = np.flatnonzero((np.abs(coef[r, idx].astype(np.int64)) >= lo) & (np.abs(coef[r, idx].astype(np.int64)) <= hi))
                if kind == "heavy_head":
                    assert set(range(c["heads"])) <= set(heavy.tolist()) and int(d0[:c["heads"]].min()) >= 1 << 32
                else:
                    cg = [s for s in range(1, idx.size // 16) if set(range(16 * s, 16 * s + 16)) <= set(heavy.tolist())]
                    assert len(cg) == 1, (F.tag(c), r)
                    rest = int(d0[16 * cg[0]:16 * cg[0] + 15].sum())                 # no other last magnitude brings the low dword of the sum lower
                    assert (rest + int(d0[16 * cg[0] + 15])) % (1 << 32) == int(((rest + ref.dist(np.arange(lo, hi + 1, dtype=np.int64) * f, 0, qb)) % (1 << 32)).min())
