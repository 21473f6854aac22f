"""Quarter-sample inter prediction on tiled frames: fractional motion compensation (xMotionCompQpelLumaGpu / ChromaGpu / Gpu) and
the quarter-sample SATD refinement (xSatd8x8RefineQpelFromTilesGpu).  The reference statement is tests/_subpel_ref.py (the
header's arithmetic in numpy int64, checked against plain loops by tests/test_subpel_ref.py); every comparison is bit-exact.
Only assert_coverage needs no GPU; every test here is marked gpu."""
import ctypes

import numpy as np
import pytest

import _quant_ref as Q
import _subpel_ref as R
from _dev import EINVAL, arena_slots, dev, displacements, records, sentinels, sync_or_exit, tile_written, tiles
from _util import me_frames
from test_gpu_mc_chroma import _mv_mix

gpu = pytest.mark.gpu
LARGER = [(48, 32), (144, 80), (272, 208)]


# ---- data -------------------------------------------------------------------------------------------------------------------------------
def _unpack(raw, nb):
    raw = np.ascontiguousarray(raw).view(np.uint8)
    return raw.view(np.int16).reshape(nb, 4)[:, :2].copy(), raw.view(np.uint32).reshape(nb, 2)[:, 1].copy()


def assert_coverage(w, h, luma, chroma):
    """what a size's case must have exercised, summed over its plane kinds (also run on the statement alone, without a GPU, by
    tests/test_subpel_ref.py)"""
    kinds = lambda s: [s[0, 0] > 0, s[1:, 0].sum() > 0, s[0, 1:].sum() > 0, s[1:, 1:].sum() > 0]   # copy, horizontal, vertical, 2-D
    if (w, h) == (16, 16):
        for c in (luma, chroma):
            assert sorted(zip(*np.nonzero(c.samples))) == [(0, 2), (1, 0), (3, 1)], c
    else:                                                                   # 32x32 is the luma phases' case: its chroma has no copy class
        assert all(kinds(luma.samples)) and ((w, h) == (32, 32) or all(kinds(chroma.samples))), (luma, chroma)
    if (w, h) in ((32, 32), (64, 64)):
        assert (luma.samples > 0).all(), luma
    if (w, h) == (64, 64):
        assert (chroma.samples > 0).all(), chroma
    for c in (luma, chroma):
        assert c.below.sum() > 0 and c.above.sum() > 0 and c.negative_v.sum() > 0, c


# ---- 1. motion compensation against the statement --------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", R.SIZES)
def test_mc_against_the_statement(codec, oracle, w, h):
    """each call on random and on {0, 255} planes: the plane it owns equals the statement, everything else (m_I, the other plane)
    is the random pre-fill byte for byte; the fused call equals the statement of both planes"""
    mv = R.vectors(w, h, w * h)
    luma, chroma = R.Counts(4), R.Counts(8)
    base = sentinels(w, h)
    for n, kind in enumerate(R.KINDS):
        y, u, v = R.planes(kind, w, h, 31 + w + 7 * n)
        rt = tiles(oracle, (y, u, v), 40 + h)
        luma += R.mc_luma(y, mv)[1]
        chroma += R.mc_chroma(u, v, mv)[2]
        for planes in ("luma", "chroma", "both"):
            got = codec.motion_comp_qpel(rt, mv, w, h, base=base, planes=planes)
            assert np.array_equal(got, R.mc_tiles(oracle, rt, mv, w, h, base, planes)), (kind, planes)
    print("%dx%d luma %r\n%dx%d chroma %r" % (w, h, luma, w, h, chroma))
    assert_coverage(w, h, luma, chroma)


@gpu
@pytest.mark.parametrize("w,h", LARGER)
def test_fused_call_is_luma_then_chroma(codec, oracle, w, h):
    y, u, v = R.planes("random", w, h, 300 + w)
    rt = tiles(oracle, (y, R.plane("extreme", w // 2, h // 2, 301), v), 302)
    mv = R.mv_mix_q((w // 8) * (h // 8), w, h, 303 + h)
    base = sentinels(w, h, 78)
    dr, dm, d_two, d_one = dev(codec, rt), dev(codec, records(mv, 0xFFFFFFFF)), dev(codec, base), dev(codec, base)   # the cost field is ignored
    codec.motion_comp_qpel_luma_dev(dr.ptr, dm.ptr, w, h, d_two.ptr)
    codec.motion_comp_qpel_chroma_dev(dr.ptr, dm.ptr, w, h, d_two.ptr)
    codec.motion_comp_qpel_dev(dr.ptr, dm.ptr, w, h, d_one.ptr)
    codec.stream_sync()
    two, one = d_two.download(np.uint8, w * h * 2), d_one.download(np.uint8, w * h * 2)
    assert np.array_equal(one, two)
    assert np.array_equal(one, R.mc_tiles(oracle, rt, mv, w, h, base))
    assert np.array_equal(dr.download(np.uint8, w * h * 2), rt)


@gpu
@pytest.mark.parametrize("w,h", LARGER)
def test_vectors_4m_reproduce_the_integer_calls(codec, oracle, w, h):
    nb = (w // 8) * (h // 8)
    y, u, v = R.planes("random", w, h, 400 + w)
    rt = tiles(oracle, (y, u, v), 401)
    m = np.clip(_mv_mix(nb, w, h, 402 + h), -8191, 8191).astype(np.int16)
    assert np.abs(m).max() == 8191 and (m & 1).any()
    base = sentinels(w, h, 79)
    assert np.array_equal(codec.motion_comp_qpel(rt, 4 * m, w, h, base=base), codec.motion_comp(rt, m, w, h, base=base))
    assert np.array_equal(codec.motion_comp_qpel(rt, 4 * m, w, h, base=base, planes="luma"), codec.motion_comp_luma(rt, m, w, h, base=base))
    assert np.array_equal(codec.motion_comp_qpel(rt, 4 * m, w, h, base=base, planes="chroma"),
                          codec.motion_comp(rt, m, w, h, base=base, planes="chroma"))


@gpu
def test_zero_vectors_copy_and_a_constant_frame_stays_constant(codec, oracle):
    w, h = 96, 64
    nb = (w // 8) * (h // 8)
    y, u, v = R.planes("random", w, h, 500)
    rt = tiles(oracle, (y, u, v), 501)
    for planes in ("luma", "chroma", "both"):
        assert np.array_equal(codec.motion_comp_qpel(rt, np.zeros((nb, 2), np.int16), w, h, base=rt, planes=planes), rt)
    flat = tiles(oracle, (np.full_like(y, 201), np.full_like(u, 255), np.full_like(v, 1)), 502)
    got = codec.motion_comp_qpel(flat, R.mv_mix_q(nb, w, h, 503), w, h).reshape(-1, 512)
    assert (got[:, :256] == 201).all()
    assert (got[:, 256:384:2] == 255).all() and (got[:, 257:384:2] == 1).all()


# ---- 2. the refinement -----------------------------------------------------------------------------------------------------------------
def _refine_case(oracle, w, h, source):
    """(cur plane, ref plane, integer vectors): me_frames content searched by the oracle, or a {0, 255} reference under _mv_mix
    vectors (far out and int16 extremes: the clamp to +-8191)"""
    nb = (w // 8) * (h // 8)
    cur, ref = me_frames(w, h, 0, 600 + w, mv=(2, -1), noise=4)
    if source == "search":
        mv_int = oracle.satd_search(cur, np.pad(ref, 4, mode="edge"), 4, 4)[0]
    else:
        ref = R.plane("extreme", w, h, 601 + w)
        mv_int = _mv_mix(nb, w, h, 602 + h)
        if nb >= 24:
            assert (np.abs(mv_int.astype(np.int64)) > 8191).any()
    return cur, ref, mv_int


@pytest.fixture(scope="module")
def refine_refs(oracle):
    """the reference's answers, computed once per case"""
    cache = {}

    def get(w, h, source):
        if (w, h, source) not in cache:
            cur, ref, mv_int = _refine_case(oracle, w, h, source)
            cache[(w, h, source)] = (cur, ref, mv_int) + R.refine(oracle, cur, ref, mv_int)
        return cache[(w, h, source)]
    return get


def _chroma_for(w, h, seed):
    return R.plane("random", w // 2, h // 2, seed), R.plane("random", w // 2, h // 2, seed + 1)


@gpu
@pytest.mark.parametrize("source", ["search", "mix"])
@pytest.mark.parametrize("w,h", [(16, 16), (48, 32), (144, 80)])
def test_refinement_against_the_reference(codec, oracle, refine_refs, w, h, source):
    cur, ref, mv_int, want_mv, want_cost, want_costs = refine_refs(w, h, source)
    ct, rt = tiles(oracle, (cur, *_chroma_for(w, h, 610)), 612), tiles(oracle, (ref, *_chroma_for(w, h, 613)), 615)
    mv, cost, costs = codec.refine_qpel_tiles(ct, rt, w, h, mv_int, want_costs=True)
    assert np.array_equal(costs, want_costs)
    assert np.array_equal(mv, want_mv) and np.array_equal(cost, want_cost)


@gpu
def test_refinement_of_constant_frames_returns_the_centre(codec, oracle):
    """every candidate of every block costs the same: the tie rule picks (0, 0), so d_best = 4 clamp(m)"""
    w, h = 48, 32
    nb = (w // 8) * (h // 8)
    u, v = _chroma_for(w, h, 620)
    ct, rt = tiles(oracle, (np.full((h, w), 90, np.uint8), u, v), 622), tiles(oracle, (np.full((h, w), 101, np.uint8), u, v), 623)
    m = _mv_mix(nb, w, h, 624)
    mv, cost, costs = codec.refine_qpel_tiles(ct, rt, w, h, m, want_costs=True)
    assert np.array_equal(mv, 4 * np.clip(m, -8191, 8191))
    centre = oracle.satd8x8(np.full((1, 64), 90 - 101, np.int16))[0]
    assert (costs == centre).all() and (cost == centre).all()


@gpu
def test_refinement_recovers_a_fractional_displacement(codec, oracle):
    """cur = the prediction of ref under (13, -10); from the integer vector (3, -2) every block finds cost 0"""
    w, h = 48, 32
    nb = (w // 8) * (h // 8)
    ref = me_frames(w, h, 0, 630)[0]
    u, v = _chroma_for(w, h, 631)
    rt = tiles(oracle, (ref, u, v), 633)
    ct = codec.motion_comp_qpel(rt, np.tile(np.int16([[13, -10]]), (nb, 1)), w, h, base=rt, planes="luma")
    cur = oracle.conv_output_420(ct, w, h)[0]
    assert np.array_equal(cur, R.mc_luma(ref, np.tile(np.int16([[13, -10]]), (nb, 1)))[0])
    m = np.tile(np.int16([[3, -2]]), (nb, 1))
    mv, cost, _ = codec.refine_qpel_tiles(ct, rt, w, h, m)
    want_mv, want_cost, _ = R.refine(oracle, cur, ref, m)
    assert not cost.any() and not want_cost.any()
    assert np.array_equal(mv, want_mv)
    assert (mv == [13, -10]).all(axis=1).any()


@gpu
def test_refinement_is_consistent_with_the_search(codec, oracle):
    """after xSatd8x8SearchFromTilesDev: the centre of d_costs is the search's cost, the refined cost is no larger, d_best is the
    winner of d_costs under the tie rule; without d_costs and in place (d_best == d_int) the records are the same"""
    w, h, rng = 144, 80, 8
    nb = (w // 8) * (h // 8)
    cur, ref = me_frames(w, h, 0, 640, mv=(-3, 2), noise=5)
    ct, rt = tiles(oracle, (cur, *_chroma_for(w, h, 641)), 643), tiles(oracle, (ref, *_chroma_for(w, h, 644)), 646)
    dc, dr = dev(codec, ct), dev(codec, rt)
    d_int, d_best, d_best2, d_costs = codec.alloc(nb * 8), codec.alloc(nb * 8), codec.alloc(nb * 8), codec.alloc(nb * 196)
    codec.satd_search_from_tiles_dev(dc.ptr, dr.ptr, w, h, rng, d_int.ptr)
    codec.satd_refine_qpel_from_tiles_dev(dc.ptr, dr.ptr, w, h, d_int.ptr, d_best.ptr, d_costs.ptr)
    codec.satd_refine_qpel_from_tiles_dev(dc.ptr, dr.ptr, w, h, d_int.ptr, d_best2.ptr)
    codec.stream_sync()
    (m, int_cost), (mv, cost) = _unpack(d_int.download(np.uint8, nb * 8), nb), _unpack(d_best.download(np.uint8, nb * 8), nb)
    costs = d_costs.download(np.uint32, nb * 49).reshape(nb, 49)
    assert np.array_equal(costs[:, 24], int_cost)
    assert (cost <= int_cost).all()
    win = R.winner(costs)
    assert np.array_equal(mv, 4 * m.astype(np.int64) + np.stack([win % 7 - 3, win // 7 - 3], axis=1))
    assert np.array_equal(cost, costs[np.arange(nb), win])
    assert np.array_equal(d_best2.download(np.uint8, nb * 8), d_best.download(np.uint8, nb * 8))
    codec.satd_refine_qpel_from_tiles_dev(dc.ptr, dr.ptr, w, h, d_int.ptr, d_int.ptr)          # in place
    codec.stream_sync()
    assert np.array_equal(d_int.download(np.uint8, nb * 8), d_best.download(np.uint8, nb * 8))
    assert np.array_equal(dc.download(np.uint8, w * h * 2), ct) and np.array_equal(dr.download(np.uint8, w * h * 2), rt)


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_inter_loop_eagerly_and_in_a_graph(codec, oracle):
    """search -> refine -> xMotionCompQpelGpu -> xDct32CodeCtuTilesGpu(.., d_recon = d_pred) on a 192x128 frame, eagerly and replayed
    from a graph: the reconstruction of the same chain composed from the numpy references; the quarter-sample prediction costs no
    more luma SATD than the integer one"""
    w, h, rng, qp, rounding = 192, 128, 8, 27, 171
    nb, nt, n = (w // 8) * (h // 8), (w // 16) * (h // 16), codec.ctu_count(w, h)
    cur_y, ref_y = me_frames(w, h, 0, 700, mv=(-4, 2), noise=5)
    cur_u, ref_u = me_frames(w // 2, h // 2, 0, 701, mv=(-2, 1), noise=5)
    cur_v, ref_v = me_frames(w // 2, h // 2, 0, 703, mv=(-2, 1), noise=5)
    ct, rt = tiles(oracle, (cur_y, cur_u, cur_v), 704), tiles(oracle, (ref_y, ref_u, ref_v), 705)
    start = sentinels(w, h, 80)
    # the chain from the references
    m = oracle.satd_search(cur_y, np.pad(ref_y, rng, mode="edge"), rng, rng)[0]
    q, q_cost, _ = R.refine(oracle, cur_y, ref_y, m)
    pred = R.mc_tiles(oracle, rt, q, w, h, start)
    want_level, want_nnz, want_recon = Q.code_ctu_tiles(oracle, ct, pred, w, h, None, qp, rounding)

    dc, dr = dev(codec, ct), dev(codec, rt)
    d_int, d_best, dp, dl, dn = codec.alloc(nb * 8), codec.alloc(nb * 8), dev(codec, start), codec.alloc(n * 12288), codec.alloc(n * 24)
    st = codec.stream_create()
    try:
        codec._check(codec.L.xHipMeScratchReserve(codec.ctx, st, w, h), "xHipMeScratchReserve")     # the search's; the refinement has none

        def enqueue():
            codec.satd_search_from_tiles_dev(dc.ptr, dr.ptr, w, h, rng, d_int.ptr, stream=st)
            codec.satd_refine_qpel_from_tiles_dev(dc.ptr, dr.ptr, w, h, d_int.ptr, d_best.ptr, stream=st)
            codec.motion_comp_qpel_dev(dr.ptr, d_best.ptr, w, h, dp.ptr, stream=st)
            codec.dct32_code_ctu_tiles_dev(dc.ptr, dp.ptr, w, h, 0, qp, rounding, dl.ptr, dn.ptr, dp.ptr, stream=st)

        def results():
            codec.stream_sync(st)
            return d_best.download(np.uint8, nb * 8), dp.download(np.uint8, w * h * 2), dl.download(np.int16, n * 6144), dn.download(np.uint32, n * 6)

        codec.graph_begin(st)
        enqueue()
        graph = codec.graph_end(st)
        try:
            enqueue()
            eager = results()
            mv, cost = _unpack(eager[0], nb)
            assert np.array_equal(mv, q) and np.array_equal(cost, q_cost)
            assert np.array_equal(eager[2].reshape(n, 6, 1024), want_level) and np.array_equal(eager[3].reshape(n, 6), want_nnz)
            assert np.array_equal(eager[1], want_recon)
            for buf in (d_int, d_best, dl, dn):
                buf.upload(np.zeros(buf.nbytes, np.uint8))
            dp.upload(start)
            codec.graph_launch(graph, st)
            for x, y in zip(eager, results()):
                assert np.array_equal(x, y)
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)
    # luma SATD from tiles of (cur, quarter-sample pred) against (cur, integer pred)
    d_q, d_i, ds = dev(codec, pred), dev(codec, codec.motion_comp(rt, m, w, h, base=start)), [codec.alloc(nb * 4), codec.alloc(nb * 4)]
    codec.satd8x8_from_tiles_dev(dc.ptr, d_q.ptr, w, h, ds[0].ptr)
    codec.satd8x8_from_tiles_dev(dc.ptr, d_i.ptr, w, h, ds[1].ptr)
    codec.stream_sync()
    sq, si = ds[0].download(np.uint32, nb).astype(np.int64), ds[1].download(np.uint32, nb).astype(np.int64)
    assert np.array_equal(sq, q_cost)
    assert sq.sum() <= si.sum()
    assert nt * 4 == nb


# ---- 4. arguments and alignment ------------------------------------------------------------------------------------------------------
MC_CALLS = {"xMotionCompQpelLumaGpu": "luma", "xMotionCompQpelChromaGpu": "chroma", "xMotionCompQpelGpu": "both"}
MC_PTRS = {"d_ref": 16, "d_mv": 8, "d_pred": 16}
REFINE_PTRS = {"d_cur": 16, "d_ref": 16, "d_int": 8, "d_best": 8, "d_costs": 4}
AW, AH = 48, 32


@pytest.fixture(scope="module")
def arena_frames(oracle):
    y, u, v = R.planes("random", AW, AH, 800)
    cur = me_frames(AW, AH, 0, 803)[0]
    return tiles(oracle, (cur, u, v), 804), tiles(oracle, (y, u, v), 805), R.mv_mix_q((AW // 8) * (AH // 8), AW, AH, 806)


def _mc_case(codec, arena_frames, planes, disp, guard_seed):
    _, rt, mv = arena_frames
    return arena_slots(codec, MC_PTRS, ("d_pred",), {"d_ref": rt, "d_mv": records(mv)}, disp, guard_seed,
                       written={"d_pred": tile_written(AW * AH // 256, planes)}, sizes={"d_pred": rt.size})


def _call_mc(codec, name, s, w=AW, h=AH):
    rc = getattr(codec.L, name)(codec.ctx, s["d_ref"].ptr, s["d_mv"].ptr, w, h, s["d_pred"].ptr, None)
    sync_or_exit(codec, rc)
    return rc


@gpu
@pytest.mark.parametrize("name", list(MC_CALLS))
def test_mc_at_minimum_alignment(codec, oracle, arena_frames, name):
    _, rt, mv = arena_frames
    results = []
    for guard_seed in (31, 32):
        a, s = _mc_case(codec, arena_frames, MC_CALLS[name], displacements(MC_PTRS), guard_seed)
        assert _call_mc(codec, name, s) == 0, codec.L.xHipLastError(codec.ctx)
        got = a.check()["d_pred"]                                           # guards, the planes the call does not own, inputs
        base = s["d_pred"].image[s["d_pred"].start:][:rt.size]
        assert np.array_equal(got, R.mc_tiles(oracle, rt, mv, AW, AH, base, MC_CALLS[name]))
        results.append(got)
    assert np.array_equal(results[0], results[1])                           # the garbage around the inputs reaches no output byte


@gpu
@pytest.mark.parametrize("ptr", list(MC_PTRS))
@pytest.mark.parametrize("name", list(MC_CALLS))
def test_mc_half_alignment_is_rejected(codec, arena_frames, name, ptr):
    a, s = _mc_case(codec, arena_frames, MC_CALLS[name], displacements(MC_PTRS, halved=ptr), 33)
    assert _call_mc(codec, name, s) == EINVAL
    assert name.encode() in codec.L.xHipLastError(codec.ctx)
    a.check_untouched()


def _refine_arena(codec, arena_frames, disp, guard_seed):
    ct, rt, mv = arena_frames
    nb = (AW // 8) * (AH // 8)
    return arena_slots(codec, REFINE_PTRS, ("d_best", "d_costs"), {"d_cur": ct, "d_ref": rt, "d_int": records(mv)}, disp, guard_seed,
                       sizes={"d_best": nb * 8, "d_costs": nb * 196})


def _call_refine(codec, s, w=AW, h=AH):
    rc = codec.L.xSatd8x8RefineQpelFromTilesGpu(codec.ctx, s["d_cur"].ptr, s["d_ref"].ptr, w, h, s["d_int"].ptr, s["d_best"].ptr, s["d_costs"].ptr, None)
    sync_or_exit(codec, rc)
    return rc


@gpu
def test_refinement_at_minimum_alignment(codec, oracle, arena_frames):
    ct, rt, mv = arena_frames
    nb = (AW // 8) * (AH // 8)
    want_mv, want_cost, want_costs = R.refine(oracle, oracle.conv_output_420(ct, AW, AH)[0], oracle.conv_output_420(rt, AW, AH)[0], mv)
    results = []
    for guard_seed in (41, 42):
        a, s = _refine_arena(codec, arena_frames, displacements(REFINE_PTRS), guard_seed)
        assert _call_refine(codec, s) == 0, codec.L.xHipLastError(codec.ctx)
        got = a.check()
        got_mv, got_cost = _unpack(got["d_best"], nb)
        assert np.array_equal(got["d_costs"].view(np.uint32).reshape(nb, 49), want_costs)
        assert np.array_equal(got_mv, want_mv) and np.array_equal(got_cost, want_cost)
        results.append((got["d_best"], got["d_costs"]))
    for x, y in zip(*results):
        assert np.array_equal(x, y)


@gpu
@pytest.mark.parametrize("ptr", list(REFINE_PTRS))
def test_refinement_half_alignment_is_rejected(codec, arena_frames, ptr):
    a, s = _refine_arena(codec, arena_frames, displacements(REFINE_PTRS, halved=ptr), 43)
    assert _call_refine(codec, s) == EINVAL
    assert b"xSatd8x8RefineQpelFromTilesGpu" in codec.L.xHipLastError(codec.ctx)
    a.check_untouched()


@gpu
@pytest.mark.parametrize("name", list(MC_CALLS))
def test_mc_argument_errors(codec, name):
    """one call per rule; nothing is launched by a refused call"""
    fn, ctx = getattr(codec.L, name), codec.ctx
    buf = codec.alloc(1 << 22)
    r = buf.ptr + (1 << 20)                          # a 64x64 tile array (8 KiB)
    b, m = buf.ptr + (2 << 20), buf.ptr + (3 << 20)  # records, and a prediction tile array
    top = ctypes.c_void_p(2 ** 64 - 4096)            # aligned, and no frame (8 KiB) fits behind it
    top8 = ctypes.c_void_p(2 ** 64 - 8)              # aligned for records, and the 64 records (512 bytes) do not fit behind it
    assert fn(None, r, b, 64, 64, m, None) == EINVAL
    for args in ((r, b, 56, 64, m), (r, b, 64, 8, m), (r, b, 0, 64, m), (r, b, 64, -16, m),                       # sizes
                 (None, b, 64, 64, m), (r, None, 64, 64, m), (r, b, 64, 64, None),                                # NULL
                 (r + 8, b, 64, 64, m), (r, b + 4, 64, 64, m), (r, b, 64, 64, m + 8),                             # alignment
                 (top, b, 64, 64, m), (r, top8, 64, 64, m), (r, b, 64, 64, top),                                   # spans past the address space
                 (r, b, 64, 64, r), (r, b, 64, 64, r + 4096), (r, b, 64, 64, r - 4096),                           # pred over ref
                 (r, b, 64, 64, b - 8192 + 16), (r, m - 256, 64, 64, m)):                                         # pred over the records
        assert fn(ctx, *args, None) == EINVAL, args
        assert name.encode() in codec.L.xHipLastError(ctx)
    assert fn(ctx, r, b, 64, 64, m, None) == 0
    codec.stream_sync()


@gpu
def test_refinement_argument_errors(codec):
    fn, ctx = codec.L.xSatd8x8RefineQpelFromTilesGpu, codec.ctx
    buf = codec.alloc(6 << 20)
    c, r = buf.ptr + (1 << 20), buf.ptr + (2 << 20)                          # two 64x64 tile arrays (8 KiB each)
    i, b, k = buf.ptr + (3 << 20), buf.ptr + (4 << 20), buf.ptr + (5 << 20)  # 64 records in, 64 out, 64 * 49 costs
    top, top8 = ctypes.c_void_p(2 ** 64 - 4096), ctypes.c_void_p(2 ** 64 - 8)   # no frame / cost map fits behind top, no 64 records behind top8
    assert fn(None, c, r, 64, 64, i, b, k, None) == EINVAL
    for args in ((c, r, 56, 64, i, b, k), (c, r, 64, 8, i, b, k), (c, r, 0, 64, i, b, k),                         # sizes
                 (None, r, 64, 64, i, b, k), (c, None, 64, 64, i, b, k), (c, r, 64, 64, None, b, k), (c, r, 64, 64, i, None, k),   # NULL
                 (c + 8, r, 64, 64, i, b, k), (c, r + 8, 64, 64, i, b, k), (c, r, 64, 64, i + 4, b, k), (c, r, 64, 64, i, b + 4, k),
                 (c, r, 64, 64, i, b, k + 2),                                                                     # alignment
                 (top, r, 64, 64, i, b, k), (c, top, 64, 64, i, b, k), (c, r, 64, 64, top8, b, k), (c, r, 64, 64, i, top8, k),
                 (c, r, 64, 64, i, b, top),                                                                       # spans past the address space
                 (c, r, 64, 64, i, c + 4096, k), (c, r, 64, 64, i, r - 256, k), (c, r, 64, 64, i, i + 8, k),      # d_best over an input
                 (c, r, 64, 64, i, b, c + 8188), (c, r, 64, 64, i, b, r - 4), (c, r, 64, 64, i, b, i + 256), (c, r, 64, 64, i, b, b - 12540)):
        assert fn(ctx, *args, None) == EINVAL, args
        assert b"xSatd8x8RefineQpelFromTilesGpu" in codec.L.xHipLastError(ctx)
    for args in ((c, r, 64, 64, i, b, k), (c, r, 64, 64, i, b, None), (c, c, 64, 64, i, b, k), (c, r, 64, 64, i, i, k)):
        assert fn(ctx, *args, None) == 0, args
    codec.stream_sync()
