"""CPU: the numpy statement of the compact level stream (tests/_levels_ref.py) against plain loops written from the text of
include/x266hip.h, the host helper xLevelScan of the built library against it, and the conditions the fixtures of
tests/test_gpu_levels.py must meet.  No GPU."""
import ctypes

import numpy as np
import pytest

import _levels_ref as ref


# ---- plain loops, from the text -------------------------------------------------------------------------------------------------------
def loop_diag(m):
    out = []
    for s in range(2 * m - 1):
        for x in range(m):
            y = s - x
            if 0 <= y < m:
                out.append((x, y))
    return out


def loop_pack(levels, classes, nnz, cap):
    """-> (records as tuples, stream list (None where not written), total words, regions that fit)"""
    recs, payloads = [], []
    for r, lv in enumerate(levels):
        n = 4 << (int(classes[r]) & 3) if classes is not None else 32
        zero = nnz is not None and int(nnz[r]) == 0
        cgs = []                                                               # (bit, map, levels)
        g = 0
        for blk in range((32 // n) ** 2):
            for cgx, cgy in loop_diag(n // 4):
                m, vals = 0, []
                for i, (x, y) in enumerate(loop_diag(4)):
                    v = 0 if zero else int(lv[blk * n * n + (4 * cgy + y) * n + 4 * cgx + x])
                    if v:
                        m |= 1 << i
                        vals.append(v)
                cgs.append((g, m, vals))
                g += 1
        assert g == 64
        mask = sum(1 << b for b, m, _ in cgs if m)
        n_nz = sum(len(v) for _, _, v in cgs)
        payload = [m for _, m, _ in cgs if m] + [x & 0xFFFF for _, m, v in cgs if m for x in v]
        recs.append([mask, 0, len(payload), n_nz, sum(abs(x) for _, _, v in cgs for x in v), max([abs(x) for _, _, v in cgs for x in v] + [0])])
        payloads.append(payload)
    off = 0
    for rec in recs:
        rec[1] = off
        off += rec[2]
    stream, fit = [None] * cap, 0
    for rec, payload in zip(recs, payloads):
        if rec[1] + rec[2] <= cap:
            fit += 1
            stream[rec[1]:rec[1] + rec[2]] = payload
    return recs, stream, off, fit


def check_pack(levels, classes=None, nnz=None, cap=None):
    rec, stream, total = ref.pack(levels, classes, nnz, cap)
    want, want_stream, words, fit = loop_pack(np.asarray(levels).reshape(-1, 1024), classes, nnz, int(total[0]) if cap is None else cap)
    assert [list(map(int, r)) for r in rec.tolist()] == want
    assert total.tolist() == [words, fit]
    assert stream.tolist() == [0 if w is None else w for w in want_stream]
    return rec, stream, total


# ---- the scans -----------------------------------------------------------------------------------------------------------------------
def test_the_4x4_scan_is_the_sixteen_numbers_of_the_header():
    assert ref.scan(4).tolist() == [0, 4, 1, 8, 5, 2, 12, 9, 6, 3, 13, 10, 7, 14, 11, 15]
    assert [y * 4 + x for x, y in loop_diag(4)] == ref.scan(4).tolist()


@pytest.mark.parametrize("size", [4, 8, 16, 32])
def test_every_scan_is_a_permutation_and_equals_the_loops(size):
    pos = ref.scan(size)
    assert sorted(pos.tolist()) == list(range(size * size))
    want = [(4 * cgy + y) * size + 4 * cgx + x for cgx, cgy in loop_diag(size // 4) for x, y in loop_diag(4)]
    assert pos.tolist() == want
    k = {4: 0, 8: 1, 16: 2, 32: 3}[size]
    assert sorted(ref.region_order(k).ravel().tolist()) == list(range(1024))
    assert ref.region_order(k).ravel()[:size * size].tolist() == want


def test_level_scan_of_the_built_library():
    import x266_amd
    x266_amd.build_library()
    lib = x266_amd.load_library()
    for size in (4, 8, 16, 32):
        assert np.array_equal(x266_amd.level_scan(size), ref.scan(size)), size
        assert np.array_equal(x266_amd.Codec.level_scan(size), ref.scan(size)), size
    buf = np.full(64 * 64, 0xABCD, np.uint16)
    for size in (0, 2, 64, -4):
        assert lib.xLevelScan(size, ctypes.c_void_p(buf.ctypes.data)) == -1, size
        with pytest.raises(x266_amd.X266Error):
            x266_amd.level_scan(size)
    assert (buf == 0xABCD).all()
    assert lib.xLevelScan(8, None) == -1
    assert x266_amd.levels_scan_chunk() >= 64


# ---- pack and unpack ------------------------------------------------------------------------------------------------------------------
def test_pack_equals_the_loops_on_the_fixtures():
    lv, cls = ref.sparse()
    rec, stream, total = check_pack(lv, cls)
    assert int(total[1]) == lv.shape[0]
    check_pack(lv, None)
    check_pack(ref.dense(), np.array([0, 1, 2], np.uint8))
    check_pack(np.zeros((3, 1024), np.int16), np.array([3, 0, 1], np.uint8))
    for k in range(4):
        hot, c = ref.one_hot(k)
        check_pack(hot[k::97], c[k::97])
    nnz = (lv != 0).sum(1).astype(np.uint32)
    check_pack(lv, cls, nnz)
    nnz[7] = 0
    assert lv[7].any()
    rec2, _, _ = check_pack(lv, cls, nnz)
    assert int(rec2["n_words"][7]) == 0 and int(rec2["cg_mask"][7]) == 0
    for cap in (int(total[0]) - 1, int(total[0]) // 2, 0):
        _, _, t = check_pack(lv, cls, None, cap)
        assert int(t[0]) == int(total[0]) and int(t[1]) < lv.shape[0]


def test_dense_regions_take_1088_words_and_hold_both_extremes():
    lv = ref.dense()
    rec, stream, total = ref.pack(lv)
    assert (rec["n_words"] == ref.MAX_WORDS).all() and (rec["cg_mask"] == np.uint64(2 ** 64 - 1)).all()
    assert lv.min() == -32768 and lv.max() == 32767 and int(rec["max_abs"].max()) == 32768
    assert int(total[0]) == 1088 * lv.shape[0]


def test_unpack_inverts_pack():
    for lv, cls in (ref.sparse(), ref.mixed(37), (ref.dense(), None), (np.zeros((2, 1024), np.int16), None)) + tuple(ref.one_hot(k) for k in range(4)):
        rec, stream, total = ref.pack(lv, cls)
        back, nnz = ref.unpack(rec, stream, lv.shape[0], cls)
        assert np.array_equal(back, lv)
        assert np.array_equal(nnz, (lv != 0).sum(1))
        assert np.array_equal(nnz, rec["n_nz"])


def test_unpack_trusts_only_mask_and_offset_and_reads_nothing_beyond_the_capacity():
    lv, cls = ref.sparse()
    rec, stream, total = ref.pack(lv, cls)
    liar = rec.copy()
    liar["n_words"], liar["n_nz"], liar["sum_abs"], liar["max_abs"] = 7, 9, 1, 2
    assert np.array_equal(ref.unpack(liar, stream, lv.shape[0], cls)[0], lv)
    r = int(np.flatnonzero(rec["n_words"] > 70)[3])
    for cut in (int(rec["offset"][r]) + 3, int(rec["offset"][r] + rec["n_words"][r]) - 1):    # inside the maps, inside the levels
        back, nnz = ref.unpack(rec, stream[:cut], lv.shape[0], cls)
        assert np.array_equal(back[:r], lv[:r]) and not back[r:].any() and not nnz[r:].any()
    # a zero map under a set mask bit contributes no level
    one = np.zeros((1, 1024), np.int16)
    one[0, [0, 40, 900]] = [5, -6, 7]
    rec1, s1, _ = ref.pack(one)
    rec1["cg_mask"][0] |= np.uint64(1 << 63)
    n_cg = bin(int(rec1["cg_mask"][0])).count("1")
    s1 = np.concatenate([s1[:n_cg - 1], [0], s1[n_cg - 1:]]).astype(np.uint16)
    back, nnz = ref.unpack(rec1, s1, 1)
    assert np.array_equal(back, one) and int(nnz[0]) == 3


# ---- the conditions of the GPU test's inputs --------------------------------------------------------------------------------------------
def test_the_sparse_fixture_meets_its_conditions():
    lv, cls = ref.sparse()
    rec, _, _ = ref.pack(lv, cls)
    full = np.uint64(2 ** 64 - 1)
    assert (cls > 3).any()                                                      # garbage above the low bits of a class byte
    for k in range(4):
        sel = np.flatnonzero((cls & 3) == k)
        m = rec["cg_mask"][sel]
        assert ((m != 0) & (m != full)).any(), k                                # a coded region with at least one uncoded CG
        assert (m == full).any(), k                                             # a region with all 64 CGs coded
        assert (lv[sel] == -32768).any() and (lv[sel] == 32767).any(), k
        assert any(m[i] == 0 and m[i - 1] != 0 and m[i + 1] != 0 for i in range(1, len(sel) - 1)), k   # all zero between two coded ones
    # geometric magnitudes: small levels dominate, large ones occur
    mags = np.abs(lv[lv != 0].astype(np.int64))
    assert (mags == 1).mean() > 0.05 and (mags > 30).any()


def test_the_one_hot_fixture_walks_every_table_entry():
    for k in range(4):
        lv, cls = ref.one_hot(k)
        assert ((lv != 0).sum(1) == 1).all() and (lv[np.arange(1024), np.arange(1024)] != 0).all() and (cls == k).all()
        rec, _, _ = ref.pack(lv, cls)
        order = ref.region_order(k)
        g, i = np.nonzero(order == np.arange(1024)[:, None, None])[1:]
        assert np.array_equal(rec["cg_mask"], np.uint64(1) << g.astype(np.uint64))
        assert len(set(zip(g.tolist(), i.tolist()))) == 1024
