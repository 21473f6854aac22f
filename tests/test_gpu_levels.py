"""GPU (-m gpu): the compact level stream (xLevelsPackGpu, xLevelsUnpackGpu) against tests/_levels_ref.py, bit-exact.  Every buffer of
every call sits between the guard bands of tests/_arena.py at exactly its documented alignment; the guards, the stream's unwritten
words and the inputs are checked after every call."""
import ctypes

import numpy as np
import pytest

import _levels_ref as R
import x266_amd
from _arena import Arena
from _dev import EINVAL, call_struct, dev, sync_or_exit

pytestmark = pytest.mark.gpu

try:
    CHUNK = x266_amd.levels_scan_chunk()                                   # the scan's step, as the implementation exposes it
except x266_amd.X266Error:                                                  # collected without a built library: the GPU tests then fail on their own
    CHUNK = 1024
PTRS = {"d_level": 16, "d_class": 1, "d_nnz": 4, "d_region": 8, "d_stream": 16, "d_total": 8}
DISP = {name: align * (2 * i + 1) for i, (name, align) in enumerate(PTRS.items())}          # exactly the documented alignment, no more


def _ptr(slots, name):
    return slots[name].ptr if name in slots else 0


def _written_words(rec, cap):
    w = np.zeros(cap, bool)
    for off, nw in zip(rec["offset"].tolist(), rec["n_words"].tolist()):
        if off + nw <= cap:
            w[off:off + nw] = True
    return w


def pack(codec, lv, cls=None, nnz=None, cap=None, null_stream=False, stream=None):
    """the call inside an arena, held against the reference: records, the written words, the untouched ones, the totals"""
    lv = np.ascontiguousarray(lv, np.int16).reshape(-1, 1024)
    n = lv.shape[0]
    want_rec, want_stream, want_total = R.pack(lv, cls, nnz, cap)
    cap = want_stream.size
    written = _written_words(want_rec, cap)
    a, s = Arena(codec), {}
    s["d_level"] = a.input("d_level", lv, 16, DISP["d_level"], 21)
    if cls is not None:
        s["d_class"] = a.input("d_class", np.asarray(cls, np.uint8), 1, DISP["d_class"], 22)
    if nnz is not None:
        s["d_nnz"] = a.input("d_nnz", np.asarray(nnz, np.uint32), 4, DISP["d_nnz"], 23)
    s["d_region"] = a.output("d_region", 32 * n, 8, DISP["d_region"])
    if not null_stream:
        s["d_stream"] = a.output("d_stream", 2 * cap, 16, DISP["d_stream"], written=np.repeat(written, 2))
    s["d_total"] = a.output("d_total", 16, 8, DISP["d_total"])
    p = codec.levels_params(*[_ptr(s, name) for name in PTRS], n_regions=n, cap_words=0 if null_stream else cap)
    call_struct(codec, "xLevelsPackGpu", p, stream)
    got = a.check()                                                         # guard bands, unwritten words, inputs
    rec = got["d_region"].view(R.RECORD_DTYPE)
    total = got["d_total"].view(np.uint64)
    assert total.tolist() == want_total.tolist(), (total, want_total)
    bad = np.flatnonzero(rec != want_rec)
    assert bad.size == 0, (bad[:4], rec[bad[:4]], want_rec[bad[:4]])
    words = got["d_stream"].view(np.uint16) if not null_stream else np.zeros(0, np.uint16)
    if not null_stream:
        bad = np.flatnonzero((words != want_stream) & written)
        assert bad.size == 0, (bad[:8], words[bad[:8]], want_stream[bad[:8]])
    return rec, words, total


def unpack(codec, rec, words, n, cls=None, cap=None, with_nnz=True, guard_seed=31, want=None):
    """the call inside an arena, held against the reference (or `want`): all 1024 levels of every region and the counts"""
    words = np.ascontiguousarray(words, np.uint16)
    cap = words.size if cap is None else cap
    want_lv, want_nnz = R.unpack(rec, words[:cap], n, cls) if want is None else want
    a, s = Arena(codec), {}
    s["d_region"] = a.input("d_region", np.ascontiguousarray(rec).view(np.uint8), 8, DISP["d_region"], guard_seed)
    s["d_stream"] = a.input("d_stream", words[:cap], 16, DISP["d_stream"], guard_seed + 1)
    if cls is not None:
        s["d_class"] = a.input("d_class", np.asarray(cls, np.uint8), 1, DISP["d_class"], guard_seed + 2)
    s["d_level"] = a.output("d_level", 2048 * n, 16, DISP["d_level"])
    if with_nnz:
        s["d_nnz"] = a.output("d_nnz", 4 * n, 4, DISP["d_nnz"])
    p = codec.levels_params(*[_ptr(s, name) for name in PTRS], n_regions=n, cap_words=cap)
    rc = codec.L.xLevelsUnpackGpu(codec.ctx, ctypes.byref(p), None)
    sync_or_exit(codec, rc)
    assert rc == 0, codec.L.xHipLastError(codec.ctx)
    got = a.check()
    lv = got["d_level"].view(np.int16).reshape(n, 1024)
    bad = np.flatnonzero((lv != want_lv).any(1))
    assert bad.size == 0, (bad[:8], n)
    if with_nnz:
        assert np.array_equal(got["d_nnz"].view(np.uint32), want_nnz)
    return lv


def round_trip(codec, lv, cls=None, nnz=None):
    lv = np.ascontiguousarray(lv, np.int16).reshape(-1, 1024)
    rec, words, total = pack(codec, lv, cls, nnz)
    assert int(total[1]) == lv.shape[0]
    counts = (lv != 0).sum(1).astype(np.uint32)
    unpack(codec, rec, words, lv.shape[0], cls, want=(lv, counts))          # the exact inverse, and it writes d_nnz
    return rec, words, total


# ---- 1. every entry of every scan table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_one_hot_sweep(codec, k):
    lv, cls = R.one_hot(k)
    rec, words, total = round_trip(codec, lv, cls)
    assert int(total[0]) == 2048 and (rec["n_words"] == 2).all()


# ---- 2. region counts around the scan's step ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 6, 7, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_region_counts(codec, n):
    assert CHUNK == x266_amd.levels_scan_chunk()
    lv, cls = R.mixed(n, seed=100 + n % 97)
    rec, words, total = round_trip(codec, lv, cls)
    if n > CHUNK:
        assert int(rec["offset"][CHUNK]) > 0 and int(total[0]) > int(rec["offset"][CHUNK])   # the running total crosses a step


def test_all_zero_input(codec):
    rec, words, total = round_trip(codec, np.zeros((9, 1024), np.int16), np.arange(9, dtype=np.uint8))
    assert total.tolist() == [0, 9] and not rec["cg_mask"].any()


def test_fully_dense_input(codec):
    lv = R.dense()
    rec, words, total = round_trip(codec, lv, np.array([0, 1, 2], np.uint8))
    assert (rec["n_words"] == 1088).all() and int(rec["max_abs"].max()) == 32768 and lv.max() == 32767
    round_trip(codec, lv)


def test_sparse_fixture_with_and_without_classes_and_counts(codec):
    lv, cls = R.sparse()
    round_trip(codec, lv, cls)
    round_trip(codec, lv, None)                                              # d_class == NULL: every region 32x32
    nnz = (lv != 0).sum(1).astype(np.uint32)
    round_trip(codec, lv, cls, nnz)                                          # d_nnz given and correct
    nnz[7] = 0                                                               # a zero entry over non-zero levels: the region packs as empty
    assert lv[7].any()
    rec, words, total = pack(codec, lv, cls, nnz)
    assert int(rec["n_words"][7]) == 0 and int(rec["cg_mask"][7]) == 0
    emptied = lv.copy()
    emptied[7] = 0
    unpack(codec, rec, words, lv.shape[0], cls, want=(emptied, (emptied != 0).sum(1).astype(np.uint32)))
    # ... and the levels under a zero count are not read: garbage there changes nothing
    rec2, words2, _ = pack(codec, np.where(np.arange(40)[:, None] == 7, np.int16(-7), lv), cls, nnz)
    assert np.array_equal(rec2, rec) and np.array_equal(words2, words)


# ---- 3. capacity --------------------------------------------------------------------------------------------------------------------------
def test_capacity(codec):
    lv, cls = R.sparse()
    full_rec, full_words, full_total = pack(codec, lv, cls)
    words_total = int(full_total[0])
    last = int(np.flatnonzero(full_rec["n_words"])[-1])
    rec, words, total = pack(codec, lv, cls, cap=words_total - 1)            # the last coded region is absent, the guard behind is untouched
    assert int(total[1]) == last and np.array_equal(rec, full_rec)
    first = int(full_rec["offset"][last])
    assert np.array_equal(words[:first], full_words[:first])
    rec, words, total = pack(codec, lv, cls, cap=words_total // 2)
    assert 0 < int(total[1]) < last and np.array_equal(rec, full_rec)
    rec, words, total = pack(codec, lv, cls, cap=0, null_stream=True)       # the count-only call
    assert np.array_equal(rec, full_rec) and int(total[0]) == words_total
    assert int(total[1]) == int(np.flatnonzero(full_rec["n_words"])[0])      # the leading empty regions fit into no words


# ---- 4. unpack on streams this library did not write --------------------------------------------------------------------------------------
def test_unpack_of_hostile_streams(codec):
    lv, cls = R.sparse()
    n = lv.shape[0]
    rec, words, _ = R.pack(lv, cls)
    liar = rec.copy()
    liar["n_words"], liar["n_nz"], liar["sum_abs"], liar["max_abs"] = 7, 9, 1, 2   # only cg_mask and offset are trusted
    unpack(codec, liar, words, n, cls, want=(lv, (lv != 0).sum(1).astype(np.uint32)))
    unpack(codec, rec, words, n, cls, with_nnz=False)
    r = int(np.flatnonzero(rec["n_words"] > 70)[3])
    for cut in (int(rec["offset"][r]) + 3, int(rec["offset"][r] + rec["n_words"][r]) - 1, int(rec["offset"][r])):
        for seed in (31, 77):                                               # whatever lies behind the capacity must not reach the result
            got = unpack(codec, rec, words, n, cls, cap=cut, guard_seed=seed)
            assert np.array_equal(got[:r], lv[:r]) and not got[r:].any()
    # a zero map under a set mask bit
    one = np.zeros((2, 1024), np.int16)
    one[0, [0, 40, 900]], one[1, 5] = [5, -6, 7], -1
    rec1, s1, _ = R.pack(one)
    rec1["cg_mask"][0] |= np.uint64(1 << 63)
    n_cg = bin(int(rec1["cg_mask"][0])).count("1")
    s1 = np.concatenate([s1[:n_cg - 1], [0], s1[n_cg - 1:]]).astype(np.uint16)
    rec1["offset"][1] += 1
    unpack(codec, rec1, s1, 2, want=(one, np.array([3, 1], np.uint32)))
    # offsets up to 64 words past the capacity (inside the arena's guard band): each such region comes back all zero
    far = rec.copy()
    coded = np.flatnonzero(rec["n_words"])
    moved = coded[::3]
    far["offset"][moved] = words.size + np.arange(moved.size) * 64 // max(moved.size - 1, 1)
    assert int(far["offset"][moved].max()) == words.size + 64 and int(far["offset"][moved].min()) == words.size
    want = lv.copy()
    want[moved] = 0
    for seed in (31, 77):
        unpack(codec, far, words, n, cls, guard_seed=seed, want=(want, (want != 0).sum(1).astype(np.uint32)))
    # a mask whose maps would start inside and end outside
    edge = rec.copy()
    edge["offset"][r] = words.size - 2
    want = lv.copy()
    want[r] = 0
    unpack(codec, edge, words, n, cls, want=(want, (want != 0).sum(1).astype(np.uint32)))


# ---- 5. end to end: the coding calls' levels through the stream and back into the chain -----------------------------------------------------
@pytest.mark.parametrize("qp", [22, 37])
@pytest.mark.parametrize("w,h", [(64, 64), (128, 64)])
def test_end_to_end_with_the_fused_coding_call(codec, w, h, qp):
    from test_gpu_quant import _tiles_mix
    n = codec.ctu_count(w, h)
    cur, pred, base = _tiles_mix(w, h, 0x7000 + w), _tiles_mix(w, h, 0x7100 + w), _tiles_mix(w, h, 0x7200 + w)
    dc, dp, dr = dev(codec, cur), dev(codec, pred), dev(codec, base)
    dl, dn = codec.alloc(n * 12288), codec.alloc(n * 24)
    codec.dct32_code_ctu_tiles_dev(dc.ptr, dp.ptr, w, h, 0, qp, 171, dl.ptr, dn.ptr, dr.ptr)
    codec.stream_sync()
    level, nnz, recon = dl.download(np.int16, n * 6144).reshape(-1, 1024), dn.download(np.uint32, 6 * n), dr.download(np.uint8, w * h * 2)
    assert level.any() and np.array_equal(nnz, (level != 0).sum(1))
    rec, words, total = pack(codec, level, None, nnz)
    assert np.array_equal(rec["n_nz"], nnz)
    back = unpack(codec, rec, words, 6 * n, want=(level, nnz))
    dz, dr2 = dev(codec, back), dev(codec, base)
    codec.quant_regions_dev(1, dz.ptr, dz.ptr, 6 * n, 0, 0, qp, 171)
    codec.dct32_inv_ctu_to_tiles_dev(dz.ptr, dp.ptr, w, h, dr2.ptr)
    codec.stream_sync()
    assert np.array_equal(dr2.download(np.uint8, w * h * 2), recon)


def test_end_to_end_with_the_mixed_transform_set(codec):
    from test_gpu_quant import _bytes, _tiles_mix
    w, h = 80, 48                                                            # cut CTUs
    n = codec.ctu_count(w, h)
    cur, pred, base = _tiles_mix(w, h, 0x7400), _tiles_mix(w, h, 0x7401), _tiles_mix(w, h, 0x7402)
    cls, qps = _bytes(6 * n, 0x7403, 15), 20 + _bytes(6 * n, 0x7404, 15)
    cls[[0, 4, 7, 11]] = (cls[[0, 4, 7, 11]] & 12) | np.arange(4, dtype=np.uint8)      # every block size, in luma and in chroma regions
    assert len(set((cls & 3).tolist())) == 4
    dc, dp, dr, dk, dq = dev(codec, cur), dev(codec, pred), dev(codec, base), dev(codec, cls), dev(codec, qps)
    dz, dn = dev(codec, np.zeros(n * 6144, np.int16)), codec.alloc(n * 24)
    codec.transform_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dk.ptr, dz.ptr)
    codec.quant_regions_dev(0, dz.ptr, dz.ptr, 6 * n, dk.ptr, dq.ptr, 0, 171, dn.ptr)
    codec.stream_sync()
    level, nnz = dz.download(np.int16, n * 6144).reshape(-1, 1024), dn.download(np.uint32, 6 * n)
    codec.quant_regions_dev(1, dz.ptr, dz.ptr, 6 * n, dk.ptr, dq.ptr, 0, 171)
    codec.transform_ctu_to_tiles_dev(dz.ptr, dk.ptr, dp.ptr, w, h, dr.ptr)
    codec.stream_sync()
    recon = dr.download(np.uint8, w * h * 2)
    rec, words, total = pack(codec, level, cls, nnz)
    back = unpack(codec, rec, words, 6 * n, cls, want=(level, nnz))
    dz2, dr2 = dev(codec, back), dev(codec, base)
    codec.quant_regions_dev(1, dz2.ptr, dz2.ptr, 6 * n, dk.ptr, dq.ptr, 0, 171)
    codec.transform_ctu_to_tiles_dev(dz2.ptr, dk.ptr, dp.ptr, w, h, dr2.ptr)
    codec.stream_sync()
    assert np.array_equal(dr2.download(np.uint8, w * h * 2), recon)


# ---- 6. the same bytes on every run ---------------------------------------------------------------------------------------------------------
def test_two_runs_on_two_streams_give_identical_bytes(codec):
    lv, cls = R.sparse()
    streams = [codec.stream_create(), codec.stream_create()]
    try:
        runs = [pack(codec, lv, cls, stream=st) for st in streams]
    finally:
        for st in streams:
            codec.stream_destroy(st)
    for a, b in zip(runs[0], runs[1]):
        assert a.tobytes() == b.tobytes()


def test_numpy_conveniences(codec):
    lv, cls = R.sparse()
    want_rec, want_stream, want_total = R.pack(lv, cls)
    rec, words, total = codec.levels_pack(lv, cls)
    assert np.array_equal(rec, want_rec) and np.array_equal(words, want_stream) and total.tolist() == want_total.tolist()
    back, nnz = codec.levels_unpack(rec, words, lv.shape[0], cls)
    assert np.array_equal(back, lv) and np.array_equal(nnz, (lv != 0).sum(1))
    rec, words, total = codec.levels_pack(lv, cls, cap_words=100)
    want_rec, want_stream, want_total = R.pack(lv, cls, None, 100)
    assert np.array_equal(rec, want_rec) and np.array_equal(words, want_stream) and total.tolist() == want_total.tolist()


# ---- 7. one graph ---------------------------------------------------------------------------------------------------------------------------
def test_pack_and_unpack_in_one_graph(codec):
    inputs = [R.mixed(70, seed=s) for s in (5, 6)]
    n, cap = 70, 70 * 1088
    d_lv, d_cls, d_rec, d_str, d_tot = codec.alloc(n * 2048), codec.alloc(n), codec.alloc(n * 32), codec.alloc(cap * 2), codec.alloc(16)
    d_back, d_nnz = codec.alloc(n * 2048), codec.alloc(n * 4)
    p_pack = codec.levels_params(d_lv.ptr, d_cls.ptr, 0, d_rec.ptr, d_str.ptr, d_tot.ptr, n, cap)
    p_unpack = codec.levels_params(d_back.ptr, d_cls.ptr, d_nnz.ptr, d_rec.ptr, d_str.ptr, 0, n, cap)
    st = codec.stream_create()
    try:
        d_lv.upload(inputs[0][0])
        d_cls.upload(inputs[0][1])
        codec.graph_begin(st)
        codec.levels_pack_dev(p_pack, stream=st)
        codec.levels_unpack_dev(p_unpack, stream=st)
        graph = codec.graph_end(st)
        try:
            for i in (1, 0):                                                 # replayed twice, on other data than it was captured with
                lv, cls = inputs[i]
                d_lv.upload(lv)
                d_cls.upload(cls)
                d_back.upload(np.full(n * 1024, 0x5A5A, np.int16))
                codec.graph_launch(graph, st)
                sync_or_exit(codec, 0, st)
                want_rec, want_stream, want_total = R.pack(lv, cls)
                assert d_tot.download(np.uint64, 2).tolist() == want_total.tolist()
                assert np.array_equal(d_rec.download(np.uint8, n * 32).view(R.RECORD_DTYPE), want_rec)
                assert np.array_equal(d_str.download(np.uint16, want_stream.size), want_stream)
                assert np.array_equal(d_back.download(np.int16, n * 1024).reshape(n, 1024), lv)
                assert np.array_equal(d_nnz.download(np.uint32, n), (lv != 0).sum(1))
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 8. refusals through the ABI --------------------------------------------------------------------------------------------------------------
def test_argument_errors(codec):
    """every rule once per call: X266HIP_EINVAL, the call named in the error text, nothing launched, the outputs untouched"""
    L, ctx = codec.L, codec.ctx
    M = 1 << 20
    buf = codec.alloc(8 * M)
    fill = np.random.RandomState(9).randint(1, 255, 8 * M).astype(np.uint8)
    buf.upload(fill)
    n, cap = 7, 4000
    lvl, cls, nnz, rec, strm, tot = (buf.ptr + i * M for i in range(1, 7))
    top = 2 ** 64 - 4096
    good = dict(d_level=lvl, d_class=cls, d_nnz=nnz, d_region=rec, d_stream=strm, d_total=tot, n_regions=n, cap_words=cap)

    def refused(name, **change):
        p = codec.levels_params(**dict(good, **change))
        assert getattr(L, name)(ctx, ctypes.byref(p), None) == EINVAL, (name, change)
        assert name.encode() in L.xHipLastError(ctx), (name, change)

    for name in ("xLevelsPackGpu", "xLevelsUnpackGpu"):
        assert getattr(L, name)(ctx, None, None) == EINVAL and name.encode() in L.xHipLastError(ctx)    # NULL p
        assert getattr(L, name)(None, ctypes.byref(codec.levels_params(**good)), None) == EINVAL
        for field in ("d_level", "d_region", "d_stream"):
            refused(name, **{field: 0})
        for field, half in (("d_level", 8), ("d_nnz", 2), ("d_region", 4), ("d_stream", 8)):
            refused(name, **{field: good[field] + half})
        for field, at in (("d_level", top), ("d_class", 2 ** 64 - 1), ("d_nnz", 2 ** 64 - 4), ("d_region", 2 ** 64 - 8), ("d_stream", top)):
            refused(name, **{field: at})                                     # aligned, and the extent does not fit behind it
        refused(name, n_regions=2 ** 53)                                     # n_regions * 2048 wraps
        refused(name, cap_words=2 ** 63)
    refused("xLevelsPackGpu", d_total=0)
    refused("xLevelsPackGpu", d_total=tot + 4)
    refused("xLevelsPackGpu", d_total=2 ** 64 - 8)
    refused("xLevelsPackGpu", n_regions=0, d_total=0)
    for field, other, extent in (("d_region", "d_level", n * 2048), ("d_stream", "d_level", n * 2048), ("d_total", "d_level", n * 2048),
                                 ("d_region", "d_class", n), ("d_stream", "d_nnz", 4 * n), ("d_total", "d_region", 32 * n), ("d_total", "d_stream", 2 * cap),
                                 ("d_stream", "d_region", 32 * n)):
        refused("xLevelsPackGpu", **{field: good[other] + (extent - 1) // PTRS[field] * PTRS[field]})   # onto the other's last bytes
        refused("xLevelsPackGpu", **{field: good[other]})
    for field, other, extent in (("d_level", "d_stream", 2 * cap), ("d_level", "d_region", 32 * n), ("d_level", "d_class", n), ("d_nnz", "d_level", 2048 * n),
                                 ("d_nnz", "d_stream", 2 * cap), ("d_nnz", "d_region", 32 * n), ("d_nnz", "d_class", n)):
        refused("xLevelsUnpackGpu", **{field: good[other] + (extent - 1) // PTRS[field] * PTRS[field]})
        refused("xLevelsUnpackGpu", **{field: good[other]})
    sync_or_exit(codec, 0)
    assert np.array_equal(buf.download(np.uint8, 8 * M), fill)             # nothing was launched
    # the edges of what is accepted: no regions (pack writes the totals alone), optional arrays NULL, d_total NULL in unpack
    for rc in (L.xLevelsUnpackGpu(ctx, ctypes.byref(codec.levels_params(n_regions=0)), None),
               L.xLevelsPackGpu(ctx, ctypes.byref(codec.levels_params(d_total=tot, n_regions=0)), None)):
        sync_or_exit(codec, rc)
        assert rc == 0, L.xHipLastError(ctx)
    now = buf.download(np.uint8, 8 * M)
    assert not now[6 * M:6 * M + 16].any()
    now[6 * M:6 * M + 16] = fill[6 * M:6 * M + 16]
    assert np.array_equal(now, fill)
