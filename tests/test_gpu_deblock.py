"""In-loop deblocking of tiled frames: xDeblockLumaGpu / ChromaGpu / Gpu against the reference statement of tests/_deblock_ref.py
(the header's arithmetic in numpy int64, checked against plain loops by tests/test_deblock_ref.py).  Every comparison is bit-exact;
every test here is marked gpu."""
import ctypes

import numpy as np
import pytest

import _deblock_ref as R
from _dev import EINVAL, arena_slots, dev, displacements, records, sentinels, sync_or_exit, tile_written
from _dev import tiles as _tiles                                       # `tiles` is what the tests here call their tile arrays
from _util import me_frames
from x266_amd._lib import DeblockParams

gpu = pytest.mark.gpu
CALLS = {"xDeblockLumaGpu": "luma", "xDeblockChromaGpu": "chroma", "xDeblockGpu": "both"}


# ---- data -------------------------------------------------------------------------------------------------------------------------------
def _records(mv):
    return records(mv, cost=0xFFFFFFFF)                                     # the cost field is ignored


class DevSide:
    """a Side's arrays on the device, and the x266_deblock_t that points at them"""

    def __init__(self, codec, side):
        self.host = {"d_class": side.cls, "d_intra": side.intra, "d_nnz": side.nnz, "d_qp": side.qps,
                     "d_mv": None if side.mv is None else _records(side.mv)}
        self.host = {k: None if a is None else np.ascontiguousarray(a).view(np.uint8).ravel() for k, a in self.host.items()}
        self.dev = {k: None if a is None else dev(codec, a) for k, a in self.host.items()}
        self.params = DeblockParams(*[self.dev[k].ptr if self.dev[k] else None for k in ("d_class", "d_intra", "d_nnz", "d_qp", "d_mv")],
                                    side.qp, side.beta_offset_div2, side.tc_offset_div2)

    def assert_unchanged(self):
        for k, a in self.host.items():
            if a is not None:
                assert np.array_equal(self.dev[k].download(np.uint8, a.size), a), k


def _call(codec, planes, d_in, w, h, ds, d_out, stream=0):
    {"luma": codec.deblock_luma_dev, "chroma": codec.deblock_chroma_dev, "both": codec.deblock_dev}[planes](d_in.ptr, w, h, ds.params, d_out.ptr, stream)


def _both_ways(codec, oracle, tiles, w, h, side, planes, base, tag):
    """out of place over a pre-fill, then in place: the result, the bytes the call does not own, the inputs"""
    ds = DevSide(codec, side)
    d_in, d_out = dev(codec, tiles), dev(codec, base)
    _call(codec, planes, d_in, w, h, ds, d_out)
    codec.stream_sync()
    got = d_out.download(np.uint8, tiles.size)
    assert np.array_equal(got, R.deblock_tiles(oracle, tiles, w, h, side, base, planes)), tag
    assert np.array_equal(d_in.download(np.uint8, tiles.size), tiles), tag
    _call(codec, planes, d_in, w, h, ds, d_in)
    codec.stream_sync()
    assert np.array_equal(d_in.download(np.uint8, tiles.size), R.deblock_tiles(oracle, tiles, w, h, side, None, planes)), tag
    ds.assert_unchanged()


# ---- 1. each call against the statement -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", R.SIZES)
def test_each_call_against_the_statement(codec, oracle, w, h):
    """every data kind with mixed classes, a mixed intra / coded / qp pattern and mixed vectors: the plane a call owns equals the
    statement, every other byte of d_out is the pre-fill, d_in and the side arrays are unchanged; in place gives the same planes"""
    total = R.new_counts()
    base = sentinels(w, h)
    for kind in R.KINDS:
        y, u, v, side = R.case(kind, w, h)
        tiles = _tiles(oracle, (y, u, v), 40 + h)
        R.deblock_tiles(oracle, tiles, w, h, side, None, "both", total)
        for planes in ("luma", "chroma", "both"):
            _both_ways(codec, oracle, tiles, w, h, side, planes, base, (kind, planes))
    print({k: dict(c) for k, c in total.items()})
    R.assert_coverage(w, h, total)


# ---- 2. the fused call is the pair -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", R.COMPOSITE)
def test_fused_call_is_luma_then_chroma(codec, oracle, w, h):
    base = sentinels(w, h, 78)
    for kind in ("blocks", "extreme"):
        y, u, v, side = R.case(kind, w, h)
        tiles = _tiles(oracle, (y, u, v), 41 + h)
        ds = DevSide(codec, side)
        d_in, d_two, d_one, d_two_ip, d_one_ip = (dev(codec, a) for a in (tiles, base, base, tiles, tiles))
        _call(codec, "luma", d_in, w, h, ds, d_two)
        _call(codec, "chroma", d_in, w, h, ds, d_two)
        _call(codec, "both", d_in, w, h, ds, d_one)
        _call(codec, "luma", d_two_ip, w, h, ds, d_two_ip)
        _call(codec, "chroma", d_two_ip, w, h, ds, d_two_ip)
        _call(codec, "both", d_one_ip, w, h, ds, d_one_ip)
        codec.stream_sync()
        one, two = d_one.download(np.uint8, tiles.size), d_two.download(np.uint8, tiles.size)
        assert np.array_equal(one, two), kind
        assert np.array_equal(one, R.deblock_tiles(oracle, tiles, w, h, side, base)), kind
        one_ip, two_ip = d_one_ip.download(np.uint8, tiles.size), d_two_ip.download(np.uint8, tiles.size)
        assert np.array_equal(one_ip, two_ip), kind
        assert np.array_equal(one_ip, R.deblock_tiles(oracle, tiles, w, h, side, None)), kind
        ds.assert_unchanged()


# ---- 3. NULL forms, offsets --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["cls", "intra", "nnz", "qps", "mv"])
def test_null_side_array_takes_its_default(codec, oracle, name):
    w, h = 80, 48
    y, u, v, side = R.case("blocks", w, h)
    tiles = _tiles(oracle, (y, u, v), 42)
    s = side.replace(**{name: None, "qp": 33})
    _both_ways(codec, oracle, tiles, w, h, s, "both", sentinels(w, h, 79), name)
    if name == "qps":                                                       # ... and NULL equals an array filled with qp
        filled = side.replace(qps=np.full_like(side.qps, 33), qp=7)
        assert np.array_equal(codec.deblock(tiles, w, h, **s.kwargs()), codec.deblock(tiles, w, h, **filled.kwargs()))


@gpu
@pytest.mark.parametrize("qp", [0, 26, 51])
def test_offsets_at_the_ends_of_the_qp_range(codec, oracle, qp):
    w, h = 64, 64
    y, u, v, side = R.case("blocks", w, h)
    tiles = _tiles(oracle, (y, u, v), 43)
    base = sentinels(w, h, 80)
    changed = 0
    for bo in (-6, 0, 6):
        for to in (-6, 0, 6):
            s = side.replace(qps=None, qp=qp, beta_offset_div2=bo, tc_offset_div2=to)
            want = R.deblock_tiles(oracle, tiles, w, h, s, base)
            assert np.array_equal(codec.deblock(tiles, w, h, base=base, **s.kwargs()), want), (bo, to)
            changed += int((want.reshape(-1, 512)[:, :384] != tiles.reshape(-1, 512)[:, :384]).sum())
    assert (changed > 0) == (qp > 0)                                        # at qp 0 even +6 leaves tc = 0 and beta = 0


# ---- 4. behind the coding call, eagerly and in a graph -----------------------------------------------------------------------------------
def _coding_inputs(oracle, w, h, seed):
    cur_y, ref_y = me_frames(w, h, 0, seed, mv=(-3, 2), noise=5)
    cur_u, ref_u = me_frames(w // 2, h // 2, 0, seed + 1, mv=(-1, 1), noise=5)
    cur_v, ref_v = me_frames(w // 2, h // 2, 0, seed + 2, mv=(-1, 1), noise=5)
    return _tiles(oracle, (cur_y, cur_u, cur_v), seed + 3), _tiles(oracle, (ref_y, ref_u, ref_v), seed + 4)


@gpu
def test_chain_behind_the_coding_call(codec, oracle):
    """xDct32CodeCtuTilesGpu's d_nnz, its d_qp and the recon it wrote go straight into xDeblockGpu in place: the statement on the
    downloaded recon; the result is accepted as d_ref by xMotionCompQpelGpu"""
    w, h, n = 128, 64, codec.ctu_count(128, 64)
    cur, pred = _coding_inputs(oracle, w, h, 900)
    side = R.case("blocks", w, h)[3]
    qps = np.array([[38, 30, 45, 70, 33, 41], [29, 44, 36, 51, 47, 40]], np.uint8)
    dc, dp, dq, dl, dn = dev(codec, cur), dev(codec, pred), dev(codec, qps), codec.alloc(n * 12288), codec.alloc(n * 24)
    codec.dct32_code_ctu_tiles_dev(dc.ptr, dp.ptr, w, h, dq.ptr, 0, 171, dl.ptr, dn.ptr, dp.ptr)
    codec.stream_sync()
    recon, nnz = dp.download(np.uint8, w * h * 2), dn.download(np.uint32, n * 6).reshape(n, 6)
    assert (nnz != 0).any() and not np.array_equal(recon, pred)
    d_intra, d_mv = dev(codec, side.intra), dev(codec, _records(side.mv))
    params = codec.deblock_params(0, d_intra.ptr, dn.ptr, dq.ptr, d_mv.ptr, 0, 1, -1)
    codec.deblock_dev(dp.ptr, w, h, params, dp.ptr)
    codec.stream_sync()
    got = dp.download(np.uint8, w * h * 2)
    s = R.Side(None, side.intra, nnz, qps, side.mv, 0, 1, -1)
    counts = R.new_counts()
    assert np.array_equal(got, R.deblock_tiles(oracle, recon, w, h, s, None, "both", counts))
    assert not np.array_equal(got, recon) and counts["luma_v"]["rule_coded"] > 0 and counts["luma_v"]["bs0"] > 0
    d_next = codec.alloc(w * h * 2)
    codec.motion_comp_qpel_dev(dp.ptr, d_mv.ptr, w, h, d_next.ptr)
    codec.stream_sync()


@gpu
def test_code_and_deblock_in_one_graph(codec, oracle):
    """the coding call and the in-place deblock captured as one linear graph, replayed twice on fresh inputs: the eager results"""
    w, h, n = 128, 64, codec.ctu_count(128, 64)
    frames = [_coding_inputs(oracle, w, h, 910 + 10 * i) for i in range(3)]
    side = R.case("steps", w, h)[3]
    d_intra, d_mv, d_cls = dev(codec, side.intra), dev(codec, _records(side.mv)), dev(codec, np.full((n, 6), 3, np.uint8))
    dc, dp, dl, dn = codec.alloc(w * h * 2), codec.alloc(w * h * 2), codec.alloc(n * 12288), codec.alloc(n * 24)
    params = codec.deblock_params(d_cls.ptr, d_intra.ptr, dn.ptr, 0, d_mv.ptr, 34, 0, 0)
    st = codec.stream_create()
    try:
        def enqueue():
            codec.dct32_code_ctu_tiles_dev(dc.ptr, dp.ptr, w, h, 0, 34, 171, dl.ptr, dn.ptr, dp.ptr, stream=st)
            codec.deblock_dev(dp.ptr, w, h, params, dp.ptr, stream=st)

        def load(i):
            dc.upload(frames[i][0])
            dp.upload(frames[i][1])

        def results():
            codec.stream_sync(st)
            return dp.download(np.uint8, w * h * 2), dn.download(np.uint32, n * 6)

        eager = []
        for i in range(3):
            load(i)
            enqueue()
            eager.append(results())
        assert not np.array_equal(eager[1][0], eager[2][0])
        load(0)
        codec.graph_begin(st)
        enqueue()
        graph = codec.graph_end(st)
        try:
            for i in (1, 2):
                load(i)
                codec.graph_launch(graph, st)
                for x, y in zip(eager[i], results()):
                    assert np.array_equal(x, y), i
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 5. arguments and alignment ----------------------------------------------------------------------------------------------------------
PTRS = {"d_in": 16, "d_class": 1, "d_intra": 1, "d_nnz": 4, "d_qp": 1, "d_mv": 8, "d_out": 16}
AW, AH = 80, 48


@pytest.fixture(scope="module")
def arena_case(oracle):
    y, u, v, side = R.case("blocks", AW, AH)
    return _tiles(oracle, (y, u, v), 804), side


def _arena(codec, arena_case, planes, disp, guard_seed):
    tiles_, side = arena_case
    data = {"d_in": tiles_, "d_class": side.cls, "d_intra": side.intra, "d_nnz": side.nnz, "d_qp": side.qps, "d_mv": _records(side.mv)}
    return arena_slots(codec, PTRS, ("d_out",), data, disp, guard_seed, written={"d_out": tile_written(AW * AH // 256, planes)}, sizes={"d_out": tiles_.size})


def _call_arena(codec, name, s, side):
    params = DeblockParams(s["d_class"].ptr, s["d_intra"].ptr, s["d_nnz"].ptr, s["d_qp"].ptr, s["d_mv"].ptr, side.qp,
                           side.beta_offset_div2, side.tc_offset_div2)
    rc = getattr(codec.L, name)(codec.ctx, s["d_in"].ptr, AW, AH, ctypes.byref(params), s["d_out"].ptr, None)
    sync_or_exit(codec, rc)
    return rc


@gpu
@pytest.mark.parametrize("name", list(CALLS))
def test_minimum_alignment(codec, oracle, arena_case, name):
    tiles, side = arena_case
    results = []
    for guard_seed in (31, 51):
        a, s = _arena(codec, arena_case, CALLS[name], displacements(PTRS), guard_seed)
        assert _call_arena(codec, name, s, side) == 0, codec.L.xHipLastError(codec.ctx)
        got = a.check()["d_out"]                                            # guards, the planes the call does not own, inputs
        base = s["d_out"].image[s["d_out"].start:][:tiles.size]
        assert np.array_equal(got, R.deblock_tiles(oracle, tiles, AW, AH, side, base, CALLS[name]))
        results.append(got)
    assert np.array_equal(results[0], results[1])                           # the garbage around the inputs reaches no output byte


@gpu
@pytest.mark.parametrize("ptr", [p for p, align in PTRS.items() if align > 1])
@pytest.mark.parametrize("name", list(CALLS))
def test_half_alignment_is_rejected(codec, arena_case, name, ptr):
    a, s = _arena(codec, arena_case, CALLS[name], displacements(PTRS, halved=ptr), 33)
    assert _call_arena(codec, name, s, arena_case[1]) == EINVAL
    assert name.encode() in codec.L.xHipLastError(codec.ctx)
    a.check_untouched()


@gpu
@pytest.mark.parametrize("name", list(CALLS))
def test_argument_errors(codec, name):
    """one call per rule; nothing is launched by a refused call"""
    fn, ctx = getattr(codec.L, name), codec.ctx
    buf = codec.alloc(8 << 20)
    i, o = buf.ptr + (1 << 20), buf.ptr + (2 << 20)                          # two 64x64 tile arrays (8 KiB each)
    side = {"d_class": buf.ptr + (3 << 20), "d_intra": buf.ptr + (3 << 20) + 64, "d_nnz": buf.ptr + (4 << 20), "d_qp": buf.ptr + (3 << 20) + 128,
            "d_mv": buf.ptr + (5 << 20)}
    top = ctypes.c_void_p(2 ** 64 - 4096)                                   # aligned, and no frame (8 KiB) fits behind it
    top8, top4, top1 = 2 ** 64 - 8, 2 ** 64 - 4, 2 ** 64 - 1                # no 64 records, no 6 counts, no 6 bytes fit behind these

    def P(qp=30, bo=0, to=0, **kw):
        d = dict(side)
        d.update(kw)
        return DeblockParams(d["d_class"], d["d_intra"], d["d_nnz"], d["d_qp"], d["d_mv"], qp, bo, to)

    good = P()
    assert fn(None, i, 64, 64, ctypes.byref(good), o, None) == EINVAL
    cases = [(i, 64, 64, None, o),                                                                               # NULL p
             (None, 64, 64, good, o), (i, 64, 64, good, None), (i + 8, 64, 64, good, o), (i, 64, 64, good, o + 8),   # NULL / misaligned frame
             (i, 56, 64, good, o), (i, 64, 8, good, o), (i, 0, 64, good, o), (i, 64, -16, good, o),               # sizes
             (i, 64, 64, P(qp=-1, d_qp=None), o), (i, 64, 64, P(qp=52, d_qp=None), o),                           # scalar qp without d_qp
             (i, 64, 64, P(bo=-7), o), (i, 64, 64, P(bo=7), o), (i, 64, 64, P(to=-7), o), (i, 64, 64, P(to=7), o),   # offsets
             (i, 64, 64, P(d_mv=side["d_mv"] + 4), o), (i, 64, 64, P(d_nnz=side["d_nnz"] + 2), o),               # misaligned side arrays
             (top, 64, 64, good, o), (i, 64, 64, good, top), (i, 64, 64, P(d_mv=top8), o), (i, 64, 64, P(d_nnz=top4), o),
             (i, 64, 64, P(d_class=top1), o), (i, 64, 64, P(d_intra=top1), o), (i, 64, 64, P(d_qp=top1), o),     # spans past the address space
             (i, 64, 64, good, i + 4096), (i, 64, 64, good, i - 4096), (i, 64, 64, good, i + 16),                # partial overlap with d_in
             (i, 64, 64, P(d_class=o + 100), o), (i, 64, 64, P(d_intra=o + 8191), o), (i, 64, 64, P(d_nnz=o - 20), o),
             (i, 64, 64, P(d_qp=o - 1), o), (i, 64, 64, P(d_mv=o + 8184), o)]                                    # d_out over a side array
    for d_in, w, h, p, d_out in cases:
        assert fn(ctx, d_in, w, h, ctypes.byref(p) if p is not None else None, d_out, None) == EINVAL, (d_in, w, h, d_out)
        assert name.encode() in codec.L.xHipLastError(ctx)
    buf.upload(np.zeros(8 << 20, np.uint8))
    for p, d_out in ((good, o), (good, i), (P(qp=-1), o), (P(qp=51, d_qp=None), o), (DeblockParams(None, None, None, None, None, 0, -6, 6), o)):
        assert fn(ctx, i, 64, 64, ctypes.byref(p), d_out, None) == 0, codec.L.xHipLastError(ctx)
    codec.stream_sync()
