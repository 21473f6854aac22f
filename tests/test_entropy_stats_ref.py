"""CPU: the host half of the per-context bin statistics -- xEntropyInitFromCounts, xEntropyCountRegion and xEntropyCountSideCtu, the
definition the device calls are held against -- against tests/_entropy_stats_ref.py, whose counts are counted off the bin lists of the two
coders' references.  No GPU."""
import numpy as np
import pytest

import _entropy_ref as E
import _entropy_side_ref as S
import _entropy_stats_ref as R


@pytest.fixture(scope="module")
def X():
    import x266_amd
    import x266_amd.entropy as X
    x266_amd.build_library()
    return X


# ---- xEntropyInitFromCounts -------------------------------------------------------------------------------------------------------------------
def test_the_table_rule_on_the_headers_values(X):
    pairs = [(0, 0), (1, 0), (0, 1), (1, 1), (1, 4095), (3, 1)]
    want = [1024, 2017, 31, 1024, 31, 1536]                                   # (1, 4095): 0.5 rounds half up to 1, then the clamp
    assert X.entropy_init_from_counts(pairs).tolist() == want == R.init_from_counts(pairs)
    assert X.entropy_init_from_counts(np.zeros((0, 2), np.uint64)).size == 0


def test_the_table_rule_is_the_integer_rule_up_to_2_to_the_51(X):
    from x266_amd import X266Error
    rs = np.random.RandomState(7)
    big = [(2 ** 40, 2 ** 40), (2 ** 40, 0), (0, 2 ** 40), (2 ** 40, 1), (1, 2 ** 40), (3 * 2 ** 40, 2 ** 40), (2 ** 51 - 1, 2 ** 51 - 1), (2 ** 51 - 1, 1),
           (2 ** 40 + 1, 2 ** 40 - 1), (2 ** 50, 3 * 2 ** 49)]
    big += [(int(rs.randint(0, 2 ** 31)) << int(rs.randint(0, 20)), int(rs.randint(0, 2 ** 31)) << int(rs.randint(0, 20))) for _ in range(300)]
    small = [(z, o) for z in range(0, 70) for o in range(0, 70)]
    for pairs in (big, small):
        assert X.entropy_init_from_counts(pairs).tolist() == R.init_from_counts(pairs)
    assert X.entropy_init_from_counts([(3 * 2 ** 40, 2 ** 40)]).tolist() == [1536]
    for bad in ([(2 ** 51, 0)], [(0, 2 ** 51)], [(1, 1), (2 ** 63, 5)], [(5, 2 ** 64 - 1)]):
        with pytest.raises(X266Error):
            X.entropy_init_from_counts(bad)
    lib = __import__("x266_amd").load_library()
    out = np.zeros(2, np.uint16)
    one = np.array([1, 1], np.uint64)
    assert lib.xEntropyInitFromCounts(None, 1, out.ctypes.data) == -1 and lib.xEntropyInitFromCounts(one.ctypes.data, 1, None) == -1
    assert lib.xEntropyInitFromCounts(None, 0, None) == 0


def test_the_table_of_a_side_frame_is_the_timing_tools_float_table(X):
    """the frame's own table as tools/gpu_entropy_side.py finds it (floor(2048 z / n + 0.5) in doubles) against the integer rule on the same
    counts: no entry differs on this frame -- where one ever does, the integer rule is the contract"""
    n, qp, off = 300, 30, -2
    arrays = S.random_arrays(n, 11)
    counts, _ = R.side_stats(n, *arrays, qp=qp, off=off)
    z, o = counts[:, 0].astype(float), counts[:, 1].astype(float)
    tool = np.clip(np.where(z + o > 0, np.floor(2048.0 * z / np.maximum(z + o, 1) + 0.5), 1024), 31, 2017).astype(np.uint16)
    got = X.entropy_init_from_counts(counts)
    assert got.tolist() == R.init_from_counts(counts)
    assert got.tolist() == tool.tolist(), [(c, int(a), int(b)) for c, (a, b) in enumerate(zip(got, tool)) if a != b]
    assert (counts.sum(axis=1) > 0).sum() >= 14 and len(set(got.tolist())) > 8      # a frame that says something


# ---- xEntropyCountRegion ----------------------------------------------------------------------------------------------------------------------
def region_cases():
    lv, cls = E.mixed(24)
    cases = [("mixed %d" % r, lv[r], int(cls[r])) for r in range(24)]
    for k in range(4):
        cases.append(("maximal, size %d" % k, E.maximal(), k))
        cases.append(("zeros, size %d" % k, np.zeros(1024, np.int16), k))
        cases += [("%s, size %d" % (name, k), level, k + 4 * k) for name, level in R.special_regions(k)]      # only cls & 3 counts
    return cases


def test_count_region_is_the_reference_on_every_case(X):
    cases = region_cases()
    assert {c & 3 for _, _, c in cases} == {0, 1, 2, 3} and sum("CG 0 empty" in n for n, _, _ in cases) == 3
    for name, level, cls in cases:
        got = X.entropy_count_region(level, cls)
        want = R.region_counts(level, cls)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:6].tolist())
        assert int(got.sum()) == X.entropy_encode_region(level, cls)[2], name        # bins[0] of xEntropyEncodeRegion
        k = cls & 3
        assert not np.delete(got, np.s_[25 * k:25 * k + 25], axis=0).any(), name    # nothing outside the size's 25 contexts


def test_count_region_adds_and_the_uncoded_region(X):
    lv, cls = E.mixed(6)
    total = np.zeros((100, 2), np.uint64)
    want = np.zeros((100, 2), np.uint64)
    for r in range(6):
        assert X.entropy_count_region(lv[r], cls[r], counts=total) is total
        want += R.region_counts(lv[r], cls[r])
    assert np.array_equal(total, want)
    for k in range(4):
        got = X.entropy_count_region(lv[1], k, coded=False)                  # the d_nnz[r] == 0 case: levels that are there are not read
        assert np.array_equal(got, R.region_counts(lv[1], k, coded=False))
        assert int(got[25 * k, 0]) == 64 >> (2 * k) == int(got.sum())
        assert np.array_equal(X.entropy_count_region(None, k, coded=False), got)
        assert np.array_equal(got, X.entropy_count_region(np.zeros(1024, np.int16), k))
        assert int(got.sum()) == X.entropy_encode_region(np.zeros(1024, np.int16), k)[2]
    from x266_amd import X266Error
    with pytest.raises(X266Error):
        X.entropy_count_region(None, 3, coded=True)
    lib = __import__("x266_amd").load_library()
    assert lib.xEntropyCountRegion(np.zeros(1024, np.int16).ctypes.data, 3, 1, None) == -1


def test_the_counts_do_not_depend_on_the_table(X):
    lv, cls = E.mixed(3)
    for r in range(3):
        for init in (None, E.worst_init(), np.full(100, 31, np.uint16)):
            assert X.entropy_encode_region(lv[r], cls[r], init)[2] == int(X.entropy_count_region(lv[r], cls[r]).sum())


# ---- xEntropyCountSideCtu ---------------------------------------------------------------------------------------------------------------------
Z0 = [0] * 6
WORKED = [                                                                # the header's eight worked CTUs as input arrays: (kind, mode, class, qp, nnz), qp
    ((Z0, [9] * 6, None, None, Z0), 32, 11),
    (([1, 0, 0, 0, 0, 0], [26] * 6, None, None, Z0), 32, 12),
    (([1, 0, 0, 0, 0, 0], [10] * 6, None, None, Z0), 32, 12),
    (([0, 0, 0, 0, 1, 0], [34] * 6, None, None, Z0), 32, 12),
    ((None, None, [0, 14, 3, 3, 3, 3], None, [1, 1, 0, 0, 0, 0]), 32, 22),
    ((None, None, None, [33, 32, 32, 32, 32, 32], [1, 0, 0, 0, 0, 0]), 32, 14),
    ((None, None, None, [0] * 6, [1, 0, 0, 0, 0, 0]), 51, 14),
    ((None, None, None, None, None), 32, 23),
]


def side_same(X, arrays, qp, off, what):
    got = X.entropy_count_side_ctu(*arrays, qp=qp, chroma_qp_offset=off)
    want = R.ctu_counts(S.canon(*arrays, qp, off), qp, off)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:6].tolist())
    assert int(got.sum()) == X.entropy_encode_side_ctu(*arrays, qp=qp, chroma_qp_offset=off)[2], what    # bins[0] of xEntropyEncodeSideCtu
    return got


def test_count_side_ctu_on_the_worked_ctus_and_the_worst(X):
    for i, (arrays, qp, bins) in enumerate(WORKED):
        assert int(side_same(X, arrays, qp, 0, ("worked", i)).sum()) == bins
    K, M, Z, C, Q = S.worst_ctu()
    assert int(side_same(X, (K, M, C, Q, Z), 0, 0, "worst").sum()) == 64


def test_count_side_ctu_on_random_ctus_and_every_null_convention(X):
    n = 200
    arrays = S.random_arrays(n, 21, 0.3)
    total = np.zeros((16, 2), np.uint64)
    for c in range(n):
        six = [a[6 * c:6 * c + 6] for a in arrays]
        qp, off = [(32, 0), (0, -12), (51, 12), (20, 5)][c % 4]
        side_same(X, six, qp, off, c)
        if c < 40:
            for missing in ((0,), (0, 1), (2,), (3,), (4,), (0, 1, 2, 3, 4)):
                side_same(X, [None if i in missing else a for i, a in enumerate(six)], qp, off, (c, missing))
        X.entropy_count_side_ctu(*six, qp=30, chroma_qp_offset=-2, counts=total)
    assert np.array_equal(total, R.side_stats(n, *arrays, qp=30, off=-2)[0])
    from x266_amd import X266Error
    six = np.zeros(6, np.uint8)
    for bad in (dict(kind=six), dict(qp=-1), dict(qp=52), dict(chroma_qp_offset=-13), dict(chroma_qp_offset=13), dict(classes=np.zeros(5, np.uint8)),
                dict(counts=np.zeros((16, 2), np.uint32))):
        with pytest.raises(X266Error):
            X.entropy_count_side_ctu(**bad)


def test_the_rows_helper(X):
    for n, per, want in ((0, 32, 0), (1, 32, 1), (32, 32, 1), (33, 32, 2), (12240, 32, 383), (2040, 64, 32), (5, 0, 0), (2 ** 64 - 1, 32, 2 ** 59)):
        assert X.entropy_stats_rows(n, per) == want
    import x266_amd
    assert x266_amd.ENTROPY_STATS_REGIONS == R.REGIONS_PER_ROW and x266_amd.ENTROPY_SIDE_STATS_CTUS == R.CTUS_PER_ROW
