"""GPU (-m gpu): inter prediction on tiled frames -- full-search motion estimation straight from ref_block_t tiles
(xSatd8x8SearchFromTilesDev, xSad8x8SearchFromTilesDev) and integer-pel luma motion compensation into tiles (xMotionCompLumaDev).
Edge convention of all three: a reference sample outside the frame takes the nearest in-frame one.  The reference statements are
the oracle's brute-force search on np.pad(ref, R, mode="edge") (planes from oracle.conv_output_420 of the tiles) and a numpy
gather with clamped coordinates."""
import numpy as np
import pytest

from _dev import dev, records, tiles
from _util import me_frames, splitmix64

pytestmark = pytest.mark.gpu


# ---- data and numpy statements -----------------------------------------------------------------------------------------------
def _tiles(oracle, y, seed):
    """a tile array whose m_Y is the plane y, with random chroma and random m_I bytes (which no call may read)"""
    h, w = y.shape
    r = splitmix64(seed, 0, (h // 2) * (w // 2) * 2)
    u = (r[: (h // 2) * (w // 2)] & np.uint64(255)).astype(np.uint8).reshape(h // 2, w // 2)
    v = ((r[(h // 2) * (w // 2):] >> np.uint64(8)) & np.uint64(255)).astype(np.uint8).reshape(h // 2, w // 2)
    return tiles(oracle, (y, u, v), seed + 1)


def _luma(oracle, tiles, w, h):
    return oracle.conv_output_420(tiles, w, h)[0]


def _mc_np(ref, mv, w, h):
    """pred[8by+y][8bx+x] = ref[clamp(8by+y+mvy, 0, H-1)][clamp(8bx+x+mvx, 0, W-1)]"""
    m = np.asarray(mv, np.int64).reshape(h // 8, w // 8, 2)
    mvx = np.repeat(np.repeat(m[..., 0], 8, 0), 8, 1)
    mvy = np.repeat(np.repeat(m[..., 1], 8, 0), 8, 1)
    yy, xx = np.mgrid[0:h, 0:w]
    return ref[np.clip(yy + mvy, 0, h - 1), np.clip(xx + mvx, 0, w - 1)]


def _block_sad(cur, pred, w, h):
    d = np.abs(cur.astype(np.int32) - pred.astype(np.int32)).reshape(h // 8, 8, w // 8, 8)
    return d.sum(axis=(1, 3)).astype(np.uint32).ravel()


def _mv_mix(nb, w, h, seed):
    """int16 vectors: small ones, the int16 extremes, vectors pointing wholly outside the frame, and zero"""
    r = splitmix64(seed, 0, 2 * nb).reshape(nb, 2)
    kind = (r >> np.uint64(60)).astype(np.int64)
    small = (r & np.uint64(63)).astype(np.int64) - 32
    ext = np.array([32767, -32768, -32767, 32766], np.int64)[((r >> np.uint64(20)) & np.uint64(3)).astype(np.int64)]
    far = np.where((r >> np.uint64(30)) & np.uint64(1), 1, -1) * (np.array([w, h], np.int64) + 8 + (r >> np.uint64(40) & np.uint64(255)).astype(np.int64))
    mv = np.select([kind < 8, kind < 11, kind < 14], [small, ext, far], 0)
    return np.clip(mv, -32768, 32767).astype(np.int16)


def _with_rows(codec, option, value, fn):
    saved = codec.get_option(option)
    codec.set_option(option, value)
    try:
        return fn()
    finally:
        codec.set_option(option, saved)


# ---- 1. every cost, every winner, both metrics --------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,rng,tile_rows", [
    (16, 16, 1, 2), (16, 16, 64, 8), (16, 16, 31, 4), (48, 16, 2, 4), (48, 16, 33, 2), (48, 16, 5, 8), (80, 48, 3, 8),
    (80, 48, 31, 4), (80, 48, 1, 8), (144, 80, 5, 2), (144, 80, 16, 8), (144, 80, 64, 2), (272, 208, 16, 2), (272, 208, 3, 8),
    (272, 208, 64, 4), (272, 208, 33, 8)])
@pytest.mark.parametrize("metric", ["satd", "sad"])
def test_every_candidate_cost_and_winner(codec, oracle, w, h, rng, tile_rows, metric):
    cur, ref = me_frames(w, h, 0, 7 * w + h + rng, mv=(min(rng, 3), -min(rng, 2)))
    ct, rt = _tiles(oracle, cur, w + rng), _tiles(oracle, ref, h + rng)
    assert np.array_equal(_luma(oracle, rt, w, h), ref)
    refp = np.pad(ref, rng, mode="edge")
    mv, cost, costs = _with_rows(codec, "me_tile_rows", tile_rows, lambda: codec.search_tiles(ct, rt, w, h, rng, want_costs=True, metric=metric))
    mv2, cost2, _ = _with_rows(codec, "me_tile_rows", tile_rows, lambda: codec.search_tiles(ct, rt, w, h, rng, metric=metric))
    omv, ocost, ocosts = oracle.satd_search(cur, refp, rng, rng, threads=8, want_costs=True, metric=metric)
    assert np.array_equal(costs, ocosts)                                 # all (2R+1)^2 costs of every block
    assert np.array_equal(cost, ocost) and np.array_equal(mv, omv)      # same winner => same tie-break
    assert np.array_equal(cost2, ocost) and np.array_equal(mv2, omv)    # the search-only kernel
    # the planar GPU search on the edge-padded plane: bit-identical records and maps
    pmv, pcost, pcosts = _with_rows(codec, "me_tile_rows", tile_rows, lambda: codec.satd_search(cur, refp, rng, rng, want_costs=True, metric=metric))
    assert np.array_equal(pmv, mv) and np.array_equal(pcost, cost) and np.array_equal(pcosts, costs)


@pytest.mark.parametrize("rng", [5, 13, 64])
@pytest.mark.parametrize("metric", ["satd", "sad"])
def test_extreme_pixels(codec, oracle, rng, metric):
    """0/255 checkerboard against random 0/255 samples: the largest costs, with windows reaching past every edge"""
    w, h = 64, 32
    yy, xx = np.mgrid[0:h, 0:w]
    cur = np.where((xx + yy) % 2 == 0, 255, 0).astype(np.uint8)
    ref = np.where((splitmix64(9 + rng, 0, h * w) >> np.uint64(13)) & np.uint64(1), 255, 0).astype(np.uint8).reshape(h, w)
    mv, cost, costs = codec.search_tiles(_tiles(oracle, cur, 1), _tiles(oracle, ref, 2), w, h, rng, want_costs=True, metric=metric)
    omv, ocost, ocosts = oracle.satd_search(cur, np.pad(ref, rng, mode="edge"), rng, rng, threads=8, want_costs=True, metric=metric)
    assert np.array_equal(costs, ocosts) and np.array_equal(mv, omv) and np.array_equal(cost, ocost)
    assert costs.max() <= (32640 if metric == "satd" else 64 * 255)


def test_same_frame_as_cur_and_ref(codec, oracle):
    """d_cur == d_ref is allowed: both are read-only"""
    w, h, rng = 80, 48, 7
    cur, _ = me_frames(w, h, 0, 55)
    ct = _tiles(oracle, cur, 3)
    d = dev(codec, ct)
    nb = (w // 8) * (h // 8)
    for metric, fn in (("satd", codec.satd_search_from_tiles_dev), ("sad", codec.sad_search_from_tiles_dev)):
        db = codec.alloc(nb * 8)
        fn(d.ptr, d.ptr, w, h, rng, db.ptr)
        codec.stream_sync()
        raw = db.download(np.uint8, nb * 8)
        omv, ocost, _ = oracle.satd_search(cur, np.pad(cur, rng, mode="edge"), rng, rng, metric=metric)
        assert np.array_equal(raw.view(np.int16).reshape(nb, 4)[:, :2], omv) and np.array_equal(raw.view(np.uint32).reshape(nb, 2)[:, 1], ocost)
        assert (ocost == 0).all()


# ---- 2. the whole 4K frame ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame_4k(oracle):
    w, h = 3840, 2160
    cur, ref = me_frames(w, h, 0, 2160, mv=(5, -3), noise=4)
    return w, h, cur, ref, _tiles(oracle, cur, 11), _tiles(oracle, ref, 12)


def test_full_frame_4k_every_block(codec, oracle, frame_4k):
    """3840x2160, +-64: all 129 600 SATD records against the oracle's brute force on the edge-padded plane; the SAD records against
    the planar GPU search on the same padded plane (itself checked against the oracle by tests/test_gpu_sad_search.py)."""
    w, h, cur, ref, ct, rt = frame_4k
    rng = 64
    refp = np.pad(ref, rng, mode="edge")
    mv, cost, _ = codec.search_tiles(ct, rt, w, h, rng)
    assert mv.shape == (129600, 2) and (mv == [5, -3]).all(axis=1).mean() > 0.9
    omv, ocost, _ = oracle.satd_search(cur, refp, rng, rng, threads=min(270, oracle.hw_threads()))
    assert np.array_equal(cost, ocost) and np.array_equal(mv, omv)
    smv, scost, _ = codec.search_tiles(ct, rt, w, h, rng, metric="sad")
    pmv, pcost, _ = codec.satd_search(cur, refp, rng, rng, metric="sad")
    assert np.array_equal(smv, pmv) and np.array_equal(scost, pcost)


# ---- 3. motion compensation against numpy -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(16, 16), (48, 16), (80, 48), (272, 208), (3840, 2160)])
def test_motion_comp_against_numpy(codec, oracle, w, h):
    ref, _ = me_frames(w, h, 0, 31 + w)
    rt = _tiles(oracle, ref, 40 + h)
    nb = (w // 8) * (h // 8)
    mv = _mv_mix(nb, w, h, w * h)
    base = (splitmix64(77, 0, w * h * 2) & np.uint64(255)).astype(np.uint8)      # sentinels: m_C and m_I must survive
    pred = codec.motion_comp_luma(rt, mv, w, h, base=base)
    assert np.array_equal(_luma(oracle, pred, w, h), _mc_np(ref, mv, w, h))
    assert np.array_equal(pred.reshape(-1, 512)[:, 256:], base.reshape(-1, 512)[:, 256:])
    # the cost field of a record is ignored
    rec = records(mv, np.full(nb, 0xFFFFFFFF, np.uint32))
    dr, dm, dp = dev(codec, rt), dev(codec, rec), dev(codec, base)
    codec.motion_comp_luma_dev(dr.ptr, dm.ptr, w, h, dp.ptr)
    codec.stream_sync()
    assert np.array_equal(dp.download(np.uint8, w * h * 2), pred)


def test_motion_comp_zero_and_whole_tile_vectors(codec, oracle):
    """mv 0 copies m_Y; a vector of whole tiles moves tiles' m_Y bytes unchanged"""
    w, h = 96, 64
    ref, _ = me_frames(w, h, 0, 5)
    rt = _tiles(oracle, ref, 6)
    nb = (w // 8) * (h // 8)
    pred = codec.motion_comp_luma(rt, np.zeros((nb, 2), np.int16), w, h, base=rt)
    assert np.array_equal(pred, rt)
    pred = codec.motion_comp_luma(rt, np.tile(np.array([[16, 16]], np.int16), (nb, 1)), w, h)
    t, p = rt.reshape(h // 16, w // 16, 512), pred.reshape(h // 16, w // 16, 512)
    assert np.array_equal(p[:-1, :-1, :256], t[1:, 1:, :256])


def test_motion_comp_beyond_4_gib(codec):
    """A 65568 x 32768 frame (8 392 704 tiles = 4.3 GB per tile array): random references and int16 vectors, 32x32 regions at the
    start, around the tile whose byte offset is 2^32 and at the far corners, against a gather over the tiles each block reads."""
    w, h = 65536 + 32, 32768
    tiles_x, nt, bw, nb = w // 16, (w // 16) * (h // 16), w // 8, (w // 8) * (h // 8)
    assert nt * 512 > (1 << 32)
    d_ref, d_pred = codec.alloc(nt * 512), codec.alloc(nt * 512)
    codec.fill_residual_dev(d_ref.ptr, nt * 256, 0xE0)
    codec.fill_residual_dev(d_pred.ptr, nt * 256, 0xE1)
    mv = _mv_mix(nb, w, h, 0xE2)
    d_mv = dev(codec, records(mv))

    def fetch(buf, byte_off, count):
        out = np.empty(count, np.uint8)
        codec._check(codec.L.xHipMemcpyD2H(codec.ctx, out.ctypes.data, buf.ptr + byte_off, count), "D2H")
        return out

    t_edge = (1 << 32) // 512
    regions = [(0, 0), (t_edge // tiles_x // 2, (t_edge % tiles_x) // 2), (h // 32 - 1, w // 32 - 1), (h // 32 - 1, 0), (0, w // 32 - 1)]
    tile_ids = lambda by, bx: [(2 * by + j) * tiles_x + 2 * bx + i for j in (0, 1) for i in (0, 1)]
    before = {(by, bx): [fetch(d_pred, t * 512, 512) for t in tile_ids(by, bx)] for by, bx in regions}
    codec.motion_comp_luma_dev(d_ref.ptr, d_mv.ptr, w, h, d_pred.ptr)
    codec.stream_sync()
    cache = {}

    def ref_at(y, x):
        t = (y >> 4) * tiles_x + (x >> 4)
        if t not in cache:
            cache[t] = fetch(d_ref, t * 512, 512)
        return cache[t][(y & 15) * 16 + (x & 15)]

    for by, bx in regions:
        got = [fetch(d_pred, t * 512, 512) for t in tile_ids(by, bx)]
        for k, (g, b) in enumerate(zip(got, before[(by, bx)])):
            assert np.array_equal(g[256:], b[256:]), (by, bx)                      # m_C / m_I untouched
            ty, tx = 2 * by + k // 2, 2 * bx + k % 2
            for y in range(16):
                for x in range(16):
                    gy, gx = 16 * ty + y, 16 * tx + x
                    mvx, mvy = (int(v) for v in mv[(gy // 8) * bw + gx // 8])
                    want = ref_at(min(max(gy + mvy, 0), h - 1), min(max(gx + mvx, 0), w - 1))
                    assert g[16 * y + x] == want, (by, bx, gy, gx)


# ---- 4. search and compensation agree with the tile stage --------------------------------------------------------------------------
def test_search_then_mc_agrees_with_the_tile_stage(codec, frame_4k):
    """pred = MC(ref, best): the from-tiles SATD of (cur, pred) is every block's SATD search cost; numpy's per-block
    sum |cur - pred| is every block's SAD search cost"""
    w, h, cur, ref, ct, rt = frame_4k
    rng, nb = 64, (w // 8) * (h // 8)
    dc, dr = dev(codec, ct), dev(codec, rt)
    db, dp, dcost = codec.alloc(nb * 8), codec.alloc(w * h * 2), codec.alloc(nb * 4)
    for metric, fn in (("satd", codec.satd_search_from_tiles_dev), ("sad", codec.sad_search_from_tiles_dev)):
        fn(dc.ptr, dr.ptr, w, h, rng, db.ptr)
        codec.motion_comp_luma_dev(dr.ptr, db.ptr, w, h, dp.ptr)
        codec.satd8x8_from_tiles_dev(dc.ptr, dp.ptr, w, h, dcost.ptr)
        codec.stream_sync()
        raw = db.download(np.uint8, nb * 8)
        mv, cost = raw.view(np.int16).reshape(nb, 4)[:, :2], raw.view(np.uint32).reshape(nb, 2)[:, 1]
        pred_tiles = dp.download(np.uint8, w * h * 2)
        pred = pred_tiles.reshape(h // 16, w // 16, 512)[:, :, :256].reshape(h // 16, w // 16, 16, 16).transpose(0, 2, 1, 3).reshape(h, w)
        assert np.array_equal(pred, _mc_np(ref, mv, w, h))
        if metric == "satd":
            assert np.array_equal(dcost.download(np.uint32, nb), cost)
        else:
            assert np.array_equal(_block_sad(cur, pred, w, h), cost)


# ---- 5. the loop in a graph --------------------------------------------------------------------------------------------------------
def test_inter_loop_in_a_graph(codec, oracle):
    """reserve scratch -> search from tiles -> MC -> xDct32FwdFromTilesDev -> xDct32InvToTilesDev(coef, pred, .., pred), recorded
    once and replayed twice: the same bytes as the eager calls"""
    w, h, rng = 256, 128, 16
    cur, ref = me_frames(w, h, 0, 808, mv=(-4, 6), noise=5)
    ct, rt = _tiles(oracle, cur, 8), _tiles(oracle, ref, 9)
    nb = (w // 8) * (h // 8)
    dc, dr = dev(codec, ct), dev(codec, rt)
    db, dp, dcoef = codec.alloc(nb * 8), dev(codec, rt), codec.alloc(w * h * 2)
    st = codec.stream_create()
    try:
        codec._check(codec.L.xHipMeScratchReserve(codec.ctx, st, w, h), "xHipMeScratchReserve")

        def enqueue():
            codec.satd_search_from_tiles_dev(dc.ptr, dr.ptr, w, h, rng, db.ptr, stream=st)
            codec.motion_comp_luma_dev(dr.ptr, db.ptr, w, h, dp.ptr, stream=st)
            codec.dct32_fwd_from_tiles_dev(dc.ptr, dp.ptr, w, h, dcoef.ptr, stream=st)
            codec.dct32_inv_to_tiles_dev(dcoef.ptr, dp.ptr, w, h, dp.ptr, stream=st)

        def results():
            codec.stream_sync(st)
            return db.download(np.uint8, nb * 8), dp.download(np.uint8, w * h * 2), dcoef.download(np.uint8, w * h * 2)

        codec.graph_begin(st)
        enqueue()
        graph = codec.graph_end(st)
        try:
            enqueue()
            eager = results()
            mv = eager[0].view(np.int16).reshape(nb, 4)[:, :2]
            omv, _, _ = oracle.satd_search(cur, np.pad(ref, rng, mode="edge"), rng, rng, threads=8)
            assert np.array_equal(mv, omv)
            assert np.array_equal(eager[1].reshape(-1, 512)[:, 256:], rt.reshape(-1, 512)[:, 256:])
            for _ in range(2):
                for buf in (db, dcoef):
                    buf.upload(np.zeros(buf.nbytes, np.uint8))
                dp.upload(rt)
                codec.graph_launch(graph, st)
                for a, b in zip(eager, results()):
                    assert np.array_equal(a, b)
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors(codec):
    L, ctx = codec.L, codec.ctx
    buf = codec.alloc(1 << 22)
    p = buf.ptr
    c, r = p, p + (1 << 20)                          # two 64x64 tile arrays (8 KiB each)
    b, m = p + (2 << 20), p + (3 << 20)              # records / cost map, and a prediction tile array
    E = -1                                           # X266HIP_EINVAL
    for fn in (L.xSatd8x8SearchFromTilesDev, L.xSad8x8SearchFromTilesDev):
        assert fn(ctx, c, r, 56, 64, 8, b, None, None) == E            # 56 % 16
        assert fn(ctx, c, r, 64, 24, 8, b, None, None) == E
        assert fn(ctx, c, r, 0, 64, 8, b, None, None) == E
        assert fn(ctx, c, r, 64, 64, 0, b, None, None) == E            # range 0
        assert fn(ctx, c, r, 64, 64, 65, b, None, None) == E           # range 65
        assert fn(ctx, None, r, 64, 64, 8, b, None, None) == E
        assert fn(ctx, c, None, 64, 64, 8, b, None, None) == E
        assert fn(ctx, c, r, 64, 64, 8, None, None, None) == E
        assert fn(ctx, c + 8, r, 64, 64, 8, b, None, None) == E        # unaligned tiles
        assert fn(ctx, c, r + 4, 64, 64, 8, b, None, None) == E
        assert fn(ctx, c, r, 64, 64, 8, b + 4, None, None) == E        # unaligned records
        assert fn(ctx, c, r, 64, 64, 8, b, b + 4098, None) == E        # unaligned cost map
        assert fn(ctx, c, r, 64, 64, 8, c + 4096, None, None) == E     # d_best inside cur
        assert fn(ctx, c, r, 64, 64, 8, r - 64, None, None) == E       # d_best runs into ref
        assert fn(ctx, c, r, 64, 64, 8, b, c + 512, None) == E         # d_costs inside cur
        assert fn(ctx, c, r, 64, 64, 8, b, r - 4096, None) == E        # d_costs (64 blocks x 289 costs) runs into ref
        assert fn(ctx, c, r, 64, 64, 8, b, (1 << 64) - 4096, None) == E   # a cost map past the end of the address space
        assert fn(ctx, c, c, 64, 64, 8, b, None, None) == 0            # d_cur == d_ref
        assert fn(ctx, c, r, 64, 64, 8, b, b + 512, None) == 0
    assert L.xMotionCompLumaDev(ctx, r, b, 56, 64, m, None) == E
    assert L.xMotionCompLumaDev(ctx, r, b, 64, 8, m, None) == E
    assert L.xMotionCompLumaDev(ctx, None, b, 64, 64, m, None) == E
    assert L.xMotionCompLumaDev(ctx, r, None, 64, 64, m, None) == E
    assert L.xMotionCompLumaDev(ctx, r, b, 64, 64, None, None) == E
    assert L.xMotionCompLumaDev(ctx, r + 8, b, 64, 64, m, None) == E
    assert L.xMotionCompLumaDev(ctx, r, b + 4, 64, 64, m, None) == E
    assert L.xMotionCompLumaDev(ctx, r, b, 64, 64, m + 8, None) == E
    assert L.xMotionCompLumaDev(ctx, r, b, 64, 64, r, None) == E        # in place
    assert L.xMotionCompLumaDev(ctx, r, b, 64, 64, r + 4096, None) == E  # partial overlap with ref
    assert L.xMotionCompLumaDev(ctx, r, b, 64, 64, r - 4096, None) == E
    assert L.xMotionCompLumaDev(ctx, r, b, 64, 64, b - 8192 + 16, None) == E   # pred runs into the records
    assert L.xMotionCompLumaDev(ctx, r, m - 256, 64, 64, m, None) == E   # records run into pred
    assert L.xMotionCompLumaDev(ctx, r, b, 64, 64, m, None) == 0
    codec.stream_sync()
