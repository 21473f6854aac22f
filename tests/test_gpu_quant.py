"""GPU (-m gpu): the quantiser over regions (xQuantRegionsGpu) and the fused CTU coding call (xDct32CodeCtuTilesGpu).  The reference
statement is tests/_quant_ref.py (the header's formulas in numpy int64, composed with the oracle's dct32 / dct32_inv /
conv_input_fmt); the fused call is also compared byte for byte with the four-call chain on the device.  Every comparison is
bit-exact."""
import ctypes

import numpy as np
import pytest

import _quant_ref as Q
from _quant_ref import EXTREMES, _bytes, _coefficients, _levels, _res_mix, _tiles_mix   # the data recipes, shared with tests/_frame_cases.py
from _dev import EINVAL, arena_slots, dev, displacements, sync_or_exit, tile_written
from _util import me_frames, splitmix64

pytestmark = pytest.mark.gpu

ROUNDINGS = [0, 171, 511]


# ---- 1. the region call against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("tables", ["none", "mixed"])
@pytest.mark.parametrize("n_regions", [1, 5, 18, 67])
def test_regions_forward_and_inverse(codec, n_regions, tables, rounding):
    """n_regions that are no multiple of the waves per workgroup (one of them past a whole workgroup); without tables (every region
    32x32, scalar qp 0 / 22 / 51) and with class bytes of all four sizes and qp bytes 0..63 (the clamp at 51)"""
    coef, lev = _coefficients(n_regions, 0x5100 + n_regions), _levels(n_regions, 0x5200 + n_regions)
    if tables == "none":
        runs = [dict(classes=None, qps=None, qp=qp) for qp in (0, 22, 51)]
    else:
        cls = _bytes(n_regions, 0x5300 + n_regions, 15)
        cls[:min(4, n_regions)] = np.arange(4, dtype=np.uint8)[:n_regions]              # every size is there
        runs = [dict(classes=cls, qps=_bytes(n_regions, 0x5400 + n_regions, 63), qp=0)]
    for kw in runs:
        got, nnz = codec.quant_regions(coef, False, rounding=rounding, **kw)
        want, want_nnz = Q.quant_regions(coef, False, rounding=rounding, **kw)
        assert np.array_equal(got, want), kw
        assert np.array_equal(nnz, want_nnz), kw
        if n_regions > 1:
            assert nnz[1] == 0
        if kw["qps"] is None and kw["qp"] == 0:
            assert nnz[0] > 512                                                          # qp 0: non-zero input stays non-zero
        back = codec.quant_regions(lev, True, rounding=rounding, **kw)
        want_back = Q.quant_regions(lev, True, **kw)
        assert np.array_equal(back, want_back), kw
        assert (want_back == 32767).any() and (want_back == -32768).any()              # the clip is reached


def test_all_zero_region_and_qp_zero(codec):
    z = np.zeros((1, 1024), np.int16)
    lv, nnz = codec.quant_regions(z, False, qp=0, rounding=511)
    assert not lv.any() and nnz.tolist() == [0]
    one = np.ones((1, 1024), np.int16)
    lv, nnz = codec.quant_regions(one, False, qp=0, rounding=511)
    want, want_nnz = Q.quant_regions(one, False, qp=0, rounding=511)
    assert np.array_equal(lv, want) and np.array_equal(nnz, want_nnz)


# ---- 2. in place, overlap ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [0, 1])
def test_in_place_equals_out_of_place(codec, inverse):
    n = 18
    x = _levels(n, 0x5500) if inverse else _coefficients(n, 0x5501)
    cls, qps = _bytes(n, 0x5502, 15), _bytes(n, 0x5503, 63)
    d_in, d_out, d_io, dk, dq = dev(codec, x), codec.alloc(x.nbytes), dev(codec, x), dev(codec, cls), dev(codec, qps)
    nnz = [None if inverse else codec.alloc(4 * n) for _ in range(2)]
    codec.quant_regions_dev(inverse, d_in.ptr, d_out.ptr, n, dk.ptr, dq.ptr, 0, 171, nnz[0].ptr if nnz[0] else 0)
    codec.quant_regions_dev(inverse, d_io.ptr, d_io.ptr, n, dk.ptr, dq.ptr, 0, 171, nnz[1].ptr if nnz[1] else 0)
    codec.stream_sync()
    want = Q.quant_regions(x, bool(inverse), cls, qps, 0, 171)
    out, io = d_out.download(np.int16, n * 1024), d_io.download(np.int16, n * 1024)
    assert np.array_equal(out, io)
    assert np.array_equal(out.reshape(n, 1024), want if inverse else want[0])
    assert np.array_equal(d_in.download(np.int16, n * 1024), x.ravel())
    if not inverse:
        assert np.array_equal(nnz[0].download(np.uint32, n), want[1]) and np.array_equal(nnz[1].download(np.uint32, n), want[1])


def test_partial_overlap_is_refused(codec):
    n = 3
    x = _coefficients(n + 1, 0x5510)
    d = dev(codec, x)
    for d_in, d_out in ((d.ptr, d.ptr + 2048), (d.ptr + 2048, d.ptr), (d.ptr, d.ptr + 16)):
        rc = codec.L.xQuantRegionsGpu(codec.ctx, 0, d_in, d_out, n, None, None, 22, 171, None, None)
        assert rc == EINVAL and b"xQuantRegionsGpu" in codec.L.xHipLastError(codec.ctx)
    out = codec.alloc(n * 2048)
    rc = codec.L.xQuantRegionsGpu(codec.ctx, 0, d.ptr, out.ptr, n, None, None, 22, 171, ctypes.c_void_p(d.ptr + 1024), None)    # nnz inside d_in
    assert rc == EINVAL
    codec.stream_sync()
    assert np.array_equal(d.download(np.int16, x.size), x.ravel())          # nothing was launched
    assert codec.L.xQuantRegionsGpu(codec.ctx, 0, None, None, 0, None, None, 22, 171, None, None) == 0   # an empty batch is no error


# ---- 3. the fused call -------------------------------------------------------------------------------------------------------------
def _qp_args(mode, n_ctus):
    if mode == "per-region":                                                # different luma and chroma values, some beyond the clamp
        q = np.empty((n_ctus, 6), np.uint8)
        q[:, :4] = 20 + (np.arange(n_ctus * 4).reshape(n_ctus, 4) % 13)
        q[:, 4], q[:, 5] = 27, 60
        return q.ravel(), 0
    return None, {"qp0": 0, "qp51": 51}[mode]


@pytest.fixture(scope="module")
def fused_frames():
    """cur / pred / the tile array d_recon starts from, per frame size: made once, never written"""
    return {(w, h): (_tiles_mix(w, h, 0x6000 + w + h), _tiles_mix(w, h, 0x6100 + w + h), _tiles_mix(w, h, 0x6200 + w + h))
            for w, h in ((64, 64), (192, 64), (192, 128))}


@pytest.mark.parametrize("mode", ["qp0", "qp51", "per-region"])
@pytest.mark.parametrize("w,h", [(64, 64), (192, 64), (192, 128)])
def test_fused_against_reference_and_chain(codec, oracle, fused_frames, w, h, mode):
    """one CTU, three, and six in two rows: levels, non-zero counts and the reconstruction against the reference and, byte for byte,
    against xDct32FwdCtuFromTilesDev -> xQuantRegionsGpu(0) -> xQuantRegionsGpu(1) -> xDct32InvCtuToTilesDev on the device"""
    cur, pred, base = fused_frames[(w, h)]
    n = codec.ctu_count(w, h)
    qps, qp = _qp_args(mode, n)
    rounding = 171
    want_level, want_nnz, want_recon = Q.code_ctu_tiles(oracle, cur, pred, w, h, qps, qp, rounding, base=base)
    if mode == "qp51":
        assert (want_level == 0).mean() > 0.5                               # most levels vanish
    if mode == "qp0":
        assert (want_nnz > 512).all()

    dc, dp, dr, dq = dev(codec, cur), dev(codec, pred), dev(codec, base), (dev(codec, qps) if qps is not None else None)
    dl, dn = codec.alloc(n * 12288), codec.alloc(max(n * 24, 16))
    q = dq.ptr if dq else 0
    codec.dct32_code_ctu_tiles_dev(dc.ptr, dp.ptr, w, h, q, qp, rounding, dl.ptr, dn.ptr, dr.ptr)
    codec.stream_sync()
    level, nnz, recon = dl.download(np.int16, n * 6144), dn.download(np.uint32, n * 6), dr.download(np.uint8, w * h * 2)
    assert np.array_equal(level.reshape(n, 6, 1024), want_level)
    assert np.array_equal(nnz.reshape(n, 6), want_nnz)
    assert np.array_equal(recon, want_recon)
    assert np.array_equal(recon.reshape(-1, 512)[:, 384:], base.reshape(-1, 512)[:, 384:])           # m_I is never written
    assert np.array_equal(dp.download(np.uint8, w * h * 2), pred) and np.array_equal(dc.download(np.uint8, w * h * 2), cur)

    # the four-call chain
    dz, dn2, dr2 = codec.alloc(n * 12288), codec.alloc(max(n * 24, 16)), dev(codec, base)
    codec.dct32_fwd_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dz.ptr)
    codec.quant_regions_dev(0, dz.ptr, dz.ptr, 6 * n, 0, q, qp, rounding, dn2.ptr)
    codec.stream_sync()
    assert np.array_equal(dz.download(np.int16, n * 6144), level)
    assert np.array_equal(dn2.download(np.uint32, n * 6), nnz)
    codec.quant_regions_dev(1, dz.ptr, dz.ptr, 6 * n, 0, q, qp, rounding)
    codec.dct32_inv_ctu_to_tiles_dev(dz.ptr, dp.ptr, w, h, dr2.ptr)
    codec.stream_sync()
    assert np.array_equal(dr2.download(np.uint8, w * h * 2), recon)

    # d_recon == d_pred; d_nnz left out
    dl3 = codec.alloc(n * 12288)
    codec.dct32_code_ctu_tiles_dev(dc.ptr, dp.ptr, w, h, q, qp, rounding, dl3.ptr, 0, dp.ptr)
    codec.stream_sync()
    in_place = dp.download(np.uint8, w * h * 2).reshape(-1, 512)
    assert np.array_equal(dl3.download(np.int16, n * 6144), level)
    assert np.array_equal(in_place[:, :384], recon.reshape(-1, 512)[:, :384])
    assert np.array_equal(in_place[:, 384:], pred.reshape(-1, 512)[:, 384:])


def test_fused_qp51_on_a_small_residual(codec, oracle):
    """pred = cur +- 2 at qp 51: every level vanishes, so the fused kernel writes nnz == 0 and all-zero level tiles for whole regions and
    the reconstruction is the prediction (the 0 / 255 / random recipe above leaves a third of the levels non-zero even at qp 51)"""
    w, h = 192, 128
    n = codec.ctu_count(w, h)
    cur = _tiles_mix(w, h, 0x6500).reshape(-1, 512)
    cur[:, :384] = 2 + (cur[:, :384].astype(np.int32) * 251 // 255).astype(np.uint8)          # 2 .. 253: room for the difference
    pred = cur.copy()
    step = (splitmix64(0x6501, 0, pred[:, :384].size) % np.uint64(5)).astype(np.int16).reshape(-1, 384) - 2
    pred[:, :384] = (cur[:, :384].astype(np.int16) + step).astype(np.uint8)
    cur, pred = cur.ravel(), pred.ravel()
    want_level, want_nnz, want_recon = Q.code_ctu_tiles(oracle, cur, pred, w, h, None, 51, 171)
    assert not want_nnz.any() and np.array_equal(want_recon, pred)       # what the data is for
    level, nnz, recon = codec.code_ctu_tiles(cur, pred, w, h, qp=51, rounding=171)
    assert not nnz.any() and not level.any()
    assert np.array_equal(recon, pred)
    level0, nnz0, recon0 = codec.code_ctu_tiles(cur, pred, w, h, qp=0, rounding=171)       # the same frames are not trivially zero
    want0 = Q.code_ctu_tiles(oracle, cur, pred, w, h, None, 0, 171)
    assert nnz0.all() and np.array_equal(level0, want0[0]) and np.array_equal(nnz0, want0[1]) and np.array_equal(recon0, want0[2])


def test_numpy_conveniences(codec, oracle, fused_frames):
    cur, pred, base = fused_frames[(192, 64)]
    got = codec.code_ctu_tiles(cur, pred, 192, 64, qp=22, rounding=171, base=base)
    want = Q.code_ctu_tiles(oracle, cur, pred, 192, 64, None, 22, 171, base=base)
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_)


# ---- 4. minimum alignment inside guard bands -------------------------------------------------------------------------------------
REGION_PTRS = {"d_in": 16, "d_out": 16, "d_class": 1, "d_qp": 1, "d_nnz": 4}
FUSED_PTRS = {"d_cur": 16, "d_pred": 16, "d_qp": 1, "d_level": 16, "d_nnz": 4, "d_recon": 16}


def _region_case(codec, inverse, disp, guard_seed):
    n = 7
    x = _levels(n, 0x5600) if inverse else _coefficients(n, 0x5601)
    cls, qps = _bytes(n, 0x5602, 15), _bytes(n, 0x5603, 63)
    placed = ("d_in", "d_class", "d_qp", "d_out") + (() if inverse else ("d_nnz",))   # the inputs first; no counts behind an inverse call
    a, s = arena_slots(codec, placed, ("d_out", "d_nnz"), {"d_in": x, "d_class": cls, "d_qp": qps}, disp, guard_seed, sizes={"d_out": n * 2048, "d_nnz": 4 * n})
    want = Q.quant_regions(x, bool(inverse), cls, qps, 0, 171)
    return a, s, n, want


def _call_region(codec, inverse, s, n, qp=0, rounding=171, nnz="own"):
    d_nnz = s["d_nnz"].ptr if nnz == "own" and "d_nnz" in s else nnz if isinstance(nnz, int) else None
    rc = codec.L.xQuantRegionsGpu(codec.ctx, inverse, s["d_in"].ptr, s["d_out"].ptr, n, s["d_class"].ptr, s["d_qp"].ptr, qp, rounding, d_nnz, None)
    sync_or_exit(codec, rc)
    return rc


@pytest.mark.parametrize("inverse", [0, 1])
def test_regions_at_minimum_alignment(codec, inverse):
    results = []
    for guard_seed in (11, 12):
        a, s, n, want = _region_case(codec, inverse, displacements(REGION_PTRS), guard_seed)
        assert _call_region(codec, inverse, s, n) == 0, codec.L.xHipLastError(codec.ctx)
        got = a.check()                                                     # guards intact, inputs unchanged
        out = got["d_out"].view(np.int16).reshape(n, 1024)
        assert np.array_equal(out, want if inverse else want[0])
        if not inverse:
            assert np.array_equal(got["d_nnz"].view(np.uint32), want[1])
        results.append(got["d_out"])
    assert np.array_equal(results[0], results[1])                           # the garbage around the inputs reaches no output byte


@pytest.mark.parametrize("ptr", [k for k, v in REGION_PTRS.items() if v > 1])
def test_regions_half_alignment_is_rejected(codec, ptr):
    a, s, n, _ = _region_case(codec, 0, displacements(REGION_PTRS, halved=ptr), 13)
    assert _call_region(codec, 0, s, n) == EINVAL
    assert b"xQuantRegionsGpu" in codec.L.xHipLastError(codec.ctx)
    a.check_untouched()


@pytest.mark.parametrize("what", ["qp52", "rounding512", "nnz-with-inverse"])
def test_regions_argument_errors(codec, what):
    inverse = 1 if what == "nnz-with-inverse" else 0
    a, s, n, _ = _region_case(codec, 0, displacements(REGION_PTRS), 14)
    if what == "qp52":
        rc = codec.L.xQuantRegionsGpu(codec.ctx, 0, s["d_in"].ptr, s["d_out"].ptr, n, s["d_class"].ptr, None, 52, 171, s["d_nnz"].ptr, None)
        sync_or_exit(codec, rc)
    elif what == "rounding512":
        rc = _call_region(codec, 0, s, n, rounding=512)
    else:
        rc = _call_region(codec, inverse, s, n)
    assert rc == EINVAL and b"xQuantRegionsGpu" in codec.L.xHipLastError(codec.ctx)
    a.check_untouched()


def _fused_case(codec, fused_frames, disp, guard_seed):
    """the 192x128 frame (six CTUs) with per-region qp bytes, every buffer placed by `disp`"""
    cur, pred, base = fused_frames[(192, 128)]
    qps, _ = _qp_args("per-region", 6)
    a, s = arena_slots(codec, FUSED_PTRS, ("d_level", "d_nnz", "d_recon"), {"d_cur": cur, "d_pred": pred, "d_qp": qps}, disp, guard_seed,
                       written={"d_recon": tile_written(192 * 128 // 256, "both")},   # m_I is a hole
                       sizes={"d_level": 6 * 12288, "d_nnz": 6 * 24, "d_recon": base.size})
    return a, s, qps


def _call_fused(codec, s, w=192, h=128, qp=0, rounding=171, with_qp=True):
    rc = codec.L.xDct32CodeCtuTilesGpu(codec.ctx, s["d_cur"].ptr, s["d_pred"].ptr, w, h, s["d_qp"].ptr if with_qp else None, qp, rounding,
                                       s["d_level"].ptr, s["d_nnz"].ptr, s["d_recon"].ptr, None)
    sync_or_exit(codec, rc)
    return rc


def test_fused_at_minimum_alignment(codec, oracle, fused_frames):
    cur, pred, _ = fused_frames[(192, 128)]
    results = []
    for guard_seed in (21, 22):
        a, s, qps = _fused_case(codec, fused_frames, displacements(FUSED_PTRS), guard_seed)
        assert _call_fused(codec, s) == 0, codec.L.xHipLastError(codec.ctx)
        got = a.check()                                                     # guards, the m_I holes, inputs
        want_level, want_nnz, want_recon = Q.code_ctu_tiles(oracle, cur, pred, 192, 128, qps, 0, 171, base=s["d_recon"].image[s["d_recon"].start:][:cur.size])
        assert np.array_equal(got["d_level"].view(np.int16), want_level.ravel())
        assert np.array_equal(got["d_nnz"].view(np.uint32), want_nnz.ravel())
        assert np.array_equal(got["d_recon"], want_recon)
        results.append((got["d_level"], got["d_nnz"], got["d_recon"].reshape(-1, 512)[:, :384].copy()))
    for x, y in zip(*results):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("ptr", [k for k, v in FUSED_PTRS.items() if v > 1])
def test_fused_half_alignment_is_rejected(codec, fused_frames, ptr):
    a, s, _ = _fused_case(codec, fused_frames, displacements(FUSED_PTRS, halved=ptr), 23)
    assert _call_fused(codec, s) == EINVAL
    assert b"xDct32CodeCtuTilesGpu" in codec.L.xHipLastError(codec.ctx)
    a.check_untouched()


@pytest.mark.parametrize("what", ["qp52", "rounding512", "width96"])
def test_fused_argument_errors(codec, fused_frames, what):
    a, s, _ = _fused_case(codec, fused_frames, displacements(FUSED_PTRS), 24)
    if what == "qp52":
        rc = _call_fused(codec, s, qp=52, with_qp=False)
    elif what == "rounding512":
        rc = _call_fused(codec, s, rounding=512)
    else:
        rc = _call_fused(codec, s, w=96, h=128)
    assert rc == EINVAL and b"xDct32CodeCtuTilesGpu" in codec.L.xHipLastError(codec.ctx)
    a.check_untouched()


# ---- 5. in a graph -----------------------------------------------------------------------------------------------------------------
def test_inter_loop_in_a_graph(codec, oracle):
    """scratch reserved, then search from tiles -> xMotionCompDev -> xDct32CodeCtuTilesGpu(.., d_recon = d_pred) on a 128x128 frame:
    run eagerly and replayed from a graph, the same levels, counts and tiles"""
    w, h, rng = 128, 128, 8
    cur_y, ref_y = me_frames(w, h, 0, 908, mv=(-4, 2), noise=5)
    cur_u, ref_u = me_frames(w // 2, h // 2, 0, 909, mv=(-2, 1), noise=5)
    cur_v, ref_v = me_frames(w // 2, h // 2, 0, 911, mv=(-2, 1), noise=5)
    ct, rt = oracle.conv_input_fmt(cur_y, cur_u, cur_v), oracle.conv_input_fmt(ref_y, ref_u, ref_v)
    nb, n = (w // 8) * (h // 8), codec.ctu_count(w, h)
    start = _tiles_mix(w, h, 0x6300)
    qps, _ = _qp_args("per-region", n)
    dc, dr, dq = dev(codec, ct), dev(codec, rt), dev(codec, qps)
    db, dp, dl, dn = codec.alloc(nb * 8), dev(codec, start), codec.alloc(n * 12288), codec.alloc(n * 24)
    st = codec.stream_create()
    try:
        codec._check(codec.L.xHipMeScratchReserve(codec.ctx, st, w, h), "xHipMeScratchReserve")

        def enqueue():
            codec.satd_search_from_tiles_dev(dc.ptr, dr.ptr, w, h, rng, db.ptr, stream=st)
            codec.motion_comp_dev(dr.ptr, db.ptr, w, h, dp.ptr, stream=st)
            codec.dct32_code_ctu_tiles_dev(dc.ptr, dp.ptr, w, h, dq.ptr, 0, 171, dl.ptr, dn.ptr, dp.ptr, stream=st)

        def results():
            codec.stream_sync(st)
            return db.download(np.uint8, nb * 8), dp.download(np.uint8, w * h * 2), dl.download(np.int16, n * 6144), dn.download(np.uint32, n * 6)

        codec.graph_begin(st)
        enqueue()
        graph = codec.graph_end(st)
        try:
            enqueue()
            eager = results()
            mv = eager[0].view(np.int16).reshape(nb, 4)[:, :2]
            pred = codec.motion_comp(rt, mv, w, h, base=start)
            want_level, want_nnz, want_recon = Q.code_ctu_tiles(oracle, ct, pred, w, h, qps, 0, 171)
            assert np.array_equal(eager[2].reshape(n, 6, 1024), want_level) and np.array_equal(eager[3].reshape(n, 6), want_nnz)
            assert np.array_equal(eager[1], want_recon)
            for buf in (db, dl, dn):
                buf.upload(np.zeros(buf.nbytes, np.uint8))
            dp.upload(start)
            codec.graph_launch(graph, st)
            for x, y in zip(eager, results()):
                assert np.array_equal(x, y)
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 6. the mixed-set loop of INTEGRATION.md ---------------------------------------------------------------------------------------
def test_mixed_set_loop_with_the_quantiser_in_place(codec, oracle):
    """xTransformCtuFromTilesDev -> xQuantRegionsGpu(0, in place) -> xQuantRegionsGpu(1, in place) -> xTransformCtuToTilesDev on a
    small frame with cut CTUs and every class: the class bytes of the transform calls are the quantiser's"""
    from test_gpu_transform_ctu_tiles import ref_forward, ref_inverse
    w, h = 144, 80
    n = codec.ctu_count(w, h)
    cur, pred, base = _tiles_mix(w, h, 0x6400), _tiles_mix(w, h, 0x6401), _tiles_mix(w, h, 0x6402)
    cls = _bytes(6 * n, 0x6403, 15)
    qps = _bytes(6 * n, 0x6404, 63)
    dc, dp, dr, dk, dq = dev(codec, cur), dev(codec, pred), dev(codec, base), dev(codec, cls), dev(codec, qps)
    dz, dn = codec.alloc(n * 12288), codec.alloc(n * 24)
    codec.transform_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dk.ptr, dz.ptr)
    codec.quant_regions_dev(0, dz.ptr, dz.ptr, 6 * n, dk.ptr, dq.ptr, 0, 171, dn.ptr)
    codec.stream_sync()
    level, nnz = dz.download(np.int16, n * 6144), dn.download(np.uint32, 6 * n)
    codec.quant_regions_dev(1, dz.ptr, dz.ptr, 6 * n, dk.ptr, dq.ptr, 0, 171)
    codec.transform_ctu_to_tiles_dev(dz.ptr, dk.ptr, dp.ptr, w, h, dr.ptr)
    codec.stream_sync()
    coef = ref_forward(oracle, cur, pred, w, h, cls)
    want_level, want_nnz = Q.quant_regions(coef, False, cls, qps, 0, 171)
    assert np.array_equal(level.reshape(-1, 1024), want_level) and np.array_equal(nnz, want_nnz)
    want = ref_inverse(oracle, Q.quant_regions(want_level, True, cls, qps), cls, pred, w, h, base)
    assert np.array_equal(dr.download(np.uint8, w * h * 2), want)
