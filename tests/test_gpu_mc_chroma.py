"""4:2:0 chroma motion compensation on tiled frames (xMotionCompChromaDev) and the fused luma + chroma call (xMotionCompDev).
The reference statement is numpy in this file: a direct transcription of the convention of include/x266hip.h (half-sample
filter -4, 36, 36, -4, edge replication on the chroma plane, arithmetic shifts) in int64 over the U and V planes that
oracle.conv_output_420 unpacks.  It also counts what it exercised -- outputs below 0 and above 255 before the clip, 2-D cases
with a negative intermediate, samples per (fx, fy) class -- so that no case silently covers only the copy path.  The statement
itself is checked against a plain Python loop by the one test here that needs no GPU; every other test is marked gpu."""
import numpy as np
import pytest

from _subpel_ref import _mv_mix                                          # the vector mix, shared with tests/_frame_cases.py
from _dev import dev, records, sentinels, tiles
from _util import me_frames, splitmix64

gpu = pytest.mark.gpu
TAPS = (-4, 36, 36, -4)


# ---- the statement ----------------------------------------------------------------------------------------------------------------
def _mcc_plane_np(plane, mv, w, h):
    """one chroma plane [h/2, w/2] uint8, mv [nb, 2] int16 per 8x8 luma block -> (uint8 plane, counts).
    counts = [below 0 before the clip, above 255 before the clip, 2-D cases with v < 0, samples of class (fx, fy) =
    (0, 0), (1, 0), (0, 1), (1, 1)]"""
    cw, ch = w // 2, h // 2
    m = np.asarray(mv, np.int64).reshape(h // 8, w // 8, 2)
    mvx = np.repeat(np.repeat(m[..., 0], 4, 0), 4, 1)
    mvy = np.repeat(np.repeat(m[..., 1], 4, 0), 4, 1)
    ix, fx, iy, fy = mvx >> 1, mvx & 1, mvy >> 1, mvy & 1                # numpy's >> on int64 is arithmetic
    yy, xx = np.mgrid[0:ch, 0:cw]
    p = np.asarray(plane, np.int64)
    S = lambda y, x: p[np.clip(y, 0, ch - 1), np.clip(x, 0, cw - 1)]
    hsum = lambda r: sum(TAPS[k] * S(r, xx + ix + k - 1) for k in range(4))
    gather = S(yy + iy, xx + ix)
    hor = (hsum(yy + iy) + 32) >> 6
    ver = (sum(TAPS[k] * S(yy + iy + k - 1, xx + ix) for k in range(4)) + 32) >> 6
    v = sum(TAPS[k] * hsum(yy + iy + k - 1) for k in range(4)) >> 6
    both = (v + 32) >> 6
    cls = [(fx == a) & (fy == b) for a, b in ((0, 0), (1, 0), (0, 1), (1, 1))]
    pre = np.select(cls[:3], [gather, hor, ver], both)
    counts = np.array([(pre < 0).sum(), (pre > 255).sum(), (cls[3] & (v < 0)).sum()] + [c.sum() for c in cls], np.int64)
    return np.clip(pre, 0, 255).astype(np.uint8), counts


def _mcc_np(u, v, mv, w, h):
    pu, cu = _mcc_plane_np(u, mv, w, h)
    pv, cv = _mcc_plane_np(v, mv, w, h)
    return pu, pv, cu + cv


def _mcc_sample(S, x, y, mvx, mvy):
    """the convention for ONE sample in plain Python integers, S(y, x) the clamped plane -> (value before the clip, v or None)"""
    ix, fx, iy, fy = mvx >> 1, mvx & 1, mvy >> 1, mvy & 1
    if not fx and not fy:
        return S(y + iy, x + ix), None
    if fx and not fy:
        return (sum(TAPS[k] * S(y + iy, x + ix + k - 1) for k in range(4)) + 32) >> 6, None
    if fy and not fx:
        return (sum(TAPS[k] * S(y + iy + k - 1, x + ix) for k in range(4)) + 32) >> 6, None
    hs = [sum(TAPS[k] * S(y + iy + r - 1, x + ix + k - 1) for k in range(4)) for r in range(4)]
    assert all(-2040 <= t <= 18360 for t in hs)
    v = sum(TAPS[r] * hs[r] for r in range(4)) >> 6
    return (v + 32) >> 6, v


def _mcc_plane_loops(plane, mv, w, h):
    cw, ch = w // 2, h // 2
    out = np.zeros((ch, cw), np.uint8)
    counts = [0] * 7
    S = lambda y, x: int(plane[min(max(y, 0), ch - 1)][min(max(x, 0), cw - 1)])
    for y in range(ch):
        for x in range(cw):
            mvx, mvy = (int(t) for t in mv[(y // 4) * (w // 8) + x // 4])
            pre, v = _mcc_sample(S, x, y, mvx, mvy)
            counts[0] += pre < 0
            counts[1] += pre > 255
            counts[2] += v is not None and v < 0
            counts[3 + (mvx & 1) + 2 * (mvy & 1)] += 1
            out[y, x] = min(max(pre, 0), 255)
    return out, np.array(counts, np.int64)


# ---- data -------------------------------------------------------------------------------------------------------------------------
def _plane(kind, w, h, seed):
    """a chroma plane [h/2, w/2]: "random" 0..255 or "extreme" {0, 255} (the content that reaches both clips)"""
    r = splitmix64(seed, 0, (h // 2) * (w // 2)).reshape(h // 2, w // 2)
    if kind == "random":
        return (r & np.uint64(255)).astype(np.uint8)
    return np.where((r >> np.uint64(13)) & np.uint64(1), 255, 0).astype(np.uint8)


def _planes_of(kind, w, h, seed):
    ku, kv = ("random", "extreme") if kind == "split" else (kind, kind)
    return _plane(ku, w, h, seed), _plane(kv, w, h, seed + 1)


def _luma(w, h, seed):
    return (splitmix64(seed, 0, w * h) & np.uint64(255)).astype(np.uint8).reshape(h, w)


def _vectors(w, h, seed):
    nb = (w // 8) * (h // 8)
    if (w, h) == (16, 16):                                               # one tile, every tap clamps: the filtered classes explicitly
        return np.array([[1, 0], [0, 1], [1, 1], [-1, -3]], np.int16)
    return _mv_mix(nb, w, h, seed)


# ---- 7. the statement itself, no GPU ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(16, 16), (48, 32)])
@pytest.mark.parametrize("kind", ["random", "extreme"])
def test_statement_against_plain_loops(w, h, kind):
    u, v = _planes_of(kind, w, h, 3 * w + h)
    mv = _vectors(w, h, w * h)
    for plane in (u, v):
        got, counts = _mcc_plane_np(plane, mv, w, h)
        want, wcounts = _mcc_plane_loops(plane, mv, w, h)
        assert np.array_equal(got, want)
        assert np.array_equal(counts, wcounts), (counts, wcounts)
        assert counts[3:].sum() == (w // 2) * (h // 2)
    if (w, h) == (16, 16):
        assert np.array_equal(_mcc_plane_np(u, mv, w, h)[1][3:], [0, 16, 16, 32])   # (-1, -3) is the 2-D class again, negative
    # a zero vector copies, an even vector moves bytes, a constant plane stays constant
    nb = (w // 8) * (h // 8)
    assert np.array_equal(_mcc_plane_np(u, np.zeros((nb, 2), np.int16), w, h)[0], u)
    assert np.array_equal(_mcc_plane_np(u, np.tile(np.int16([[2, -4]]), (nb, 1)), w, h)[0][2:, :-1], u[:-2, 1:])
    assert (_mcc_plane_np(np.full_like(u, 201), mv, w, h)[0] == 201).all()


def test_vector_split_is_arithmetic():
    S = lambda y, x: 10 * y + x
    assert _mcc_sample(S, 20, 20, -32768, 32766) == (10 * (20 + 16383) + 20 - 16384, None)
    one = np.full((8, 8), 9, np.uint8)
    for mvx, want in ((-1, (-1, 1)), (-32768, (-16384, 0)), (32767, (16383, 1)), (-3, (-2, 1))):
        assert (np.int64(mvx) >> 1, np.int64(mvx) & 1) == want and (mvx >> 1, mvx & 1) == want
    assert (_mcc_plane_np(one, np.int16([[-32768, 32767], [32767, -32767], [-1, -1], [1, 1]]), 16, 16)[0] == 9).all()


# ---- 1. against numpy ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", [(16, 16), (48, 32), (144, 80), (272, 208), (3840, 2160)])
def test_chroma_against_numpy(codec, oracle, w, h):
    """both plane kinds per case (3840x2160 once: U random, V {0, 255}); the counts of the case, summed over its kinds, must all
    be non-zero from 48x32 upward -- the clips fire on the {0, 255} planes only"""
    nb = (w // 8) * (h // 8)
    mv = _vectors(w, h, w * h)
    total = np.zeros(7, np.int64)
    for n, kind in enumerate(("split",) if w == 3840 else ("random", "extreme")):
        u, v = _planes_of(kind, w, h, 31 + w + n)
        y = _luma(w, h, 5 + n)
        rt = tiles(oracle, (y, u, v), 40 + h)
        base = sentinels(w, h)                                          # m_Y and m_I must survive
        pred = codec.motion_comp(rt, mv, w, h, base=base, planes="chroma")
        wu, wv, counts = _mcc_np(u, v, mv, w, h)
        total += counts
        _, gu, gv = oracle.conv_output_420(pred, w, h)
        assert np.array_equal(gu, wu) and np.array_equal(gv, wv), kind
        p, b = pred.reshape(-1, 512), base.reshape(-1, 512)
        assert np.array_equal(p[:, :256], b[:, :256]) and np.array_equal(p[:, 384:], b[:, 384:])
        assert (counts[3:] > 0).all() or nb < 24, counts
        # raw device pointers; the cost field of a record is ignored
        rec = records(mv, np.full(nb, 0xFFFFFFFF, np.uint32))
        dr, dm, dp = dev(codec, rt), dev(codec, rec), dev(codec, base)
        codec.motion_comp_chroma_dev(dr.ptr, dm.ptr, w, h, dp.ptr)
        codec.stream_sync()
        assert np.array_equal(dp.download(np.uint8, w * h * 2), pred)
    print("counts %dx%d: below 0 %d, above 255 %d, negative v %d, classes %s" % (w, h, total[0], total[1], total[2], total[3:]))
    if (w, h) == (16, 16):
        assert np.array_equal(total[3:], [0, 64, 64, 128])               # two kinds x two planes x 16 samples per block
    else:
        assert (total > 0).all(), total


# ---- 2. identities ------------------------------------------------------------------------------------------------------------------
@gpu
def test_chroma_identities(codec, oracle):
    """mv 0 with base = ref returns ref; (32, 32) moves whole tiles' m_C unchanged; a constant chroma plane stays constant"""
    w, h = 96, 64
    nb = (w // 8) * (h // 8)
    u, v = _planes_of("split", w, h, 17)
    rt = tiles(oracle, (_luma(w, h, 3), u, v), 6)
    for planes in ("chroma", "both"):
        assert np.array_equal(codec.motion_comp(rt, np.zeros((nb, 2), np.int16), w, h, base=rt, planes=planes), rt)
        pred = codec.motion_comp(rt, np.tile(np.array([[32, 32]], np.int16), (nb, 1)), w, h, planes=planes)
        t, p = rt.reshape(h // 16, w // 16, 512), pred.reshape(h // 16, w // 16, 512)
        assert np.array_equal(p[:-2, :-2, 256:384], t[2:, 2:, 256:384])
        flat = tiles(oracle, (_luma(w, h, 4), np.full_like(u, 255), np.full_like(v, 1)), 7)
        got = codec.motion_comp(flat, _mv_mix(nb, w, h, 99), w, h, planes=planes).reshape(-1, 512)[:, 256:384].reshape(-1, 2)
        assert (got[:, 0] == 255).all() and (got[:, 1] == 1).all()


# ---- 3. the fused call ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", [(48, 32), (144, 80), (272, 208)])
def test_fused_call_is_luma_then_chroma(codec, oracle, w, h):
    nb = (w // 8) * (h // 8)
    u, v = _planes_of("split", w, h, 300 + w)
    y, _ = me_frames(w, h, 0, 301 + w)
    rt = tiles(oracle, (y, u, v), 302)
    mv = _mv_mix(nb, w, h, 303 + h)
    base = sentinels(w, h, 78)
    dr, dm, d_two, d_one = dev(codec, rt), dev(codec, records(mv)), dev(codec, base), dev(codec, base)
    codec.motion_comp_luma_dev(dr.ptr, dm.ptr, w, h, d_two.ptr)
    codec.motion_comp_chroma_dev(dr.ptr, dm.ptr, w, h, d_two.ptr)
    codec.motion_comp_dev(dr.ptr, dm.ptr, w, h, d_one.ptr)
    codec.stream_sync()
    two, one = d_two.download(np.uint8, w * h * 2), d_one.download(np.uint8, w * h * 2)
    assert np.array_equal(one, two)
    assert np.array_equal(one.reshape(-1, 512)[:, 384:], base.reshape(-1, 512)[:, 384:])
    assert np.array_equal(one, codec.motion_comp(rt, mv, w, h, base=base))
    wu, wv, _ = _mcc_np(u, v, mv, w, h)
    _, gu, gv = oracle.conv_output_420(one, w, h)
    assert np.array_equal(gu, wu) and np.array_equal(gv, wv)


# ---- 4. closing the loop ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_frames(oracle):
    w, h = 256, 128
    cur_y, ref_y = me_frames(w, h, 0, 808, mv=(-4, 6), noise=5)
    cur_u, ref_u = me_frames(w // 2, h // 2, 0, 809, mv=(-2, 3), noise=5)
    cur_v, ref_v = me_frames(w // 2, h // 2, 0, 811, mv=(-2, 3), noise=5)
    return w, h, (cur_y, cur_u, cur_v), (ref_y, ref_u, ref_v), tiles(oracle, (cur_y, cur_u, cur_v), 8), tiles(oracle, (ref_y, ref_u, ref_v), 9)


@gpu
def test_search_mc_residual_recon_and_satd(codec, oracle, loop_frames):
    """search from tiles -> xMotionCompDev -> chroma residual -> chroma recon gives back cur's m_C; the chroma SATD from tiles of
    (cur, pred) is satd8x8 of numpy's cur - pred"""
    w, h, cur, ref, ct, rt = loop_frames
    rng, nb, nt, npl = 16, (w // 8) * (h // 8), (w // 16) * (h // 16), (w // 2) * (h // 2)
    dc, dr = dev(codec, ct), dev(codec, rt)
    db, dp, drec = codec.alloc(nb * 8), dev(codec, sentinels(w, h, 79)), dev(codec, sentinels(w, h, 80))
    dru, drv, dsu, dsv = codec.alloc(npl * 2), codec.alloc(npl * 2), codec.alloc(nt * 4), codec.alloc(nt * 4)
    codec.satd_search_from_tiles_dev(dc.ptr, dr.ptr, w, h, rng, db.ptr)
    codec.motion_comp_dev(dr.ptr, db.ptr, w, h, dp.ptr)
    codec.residual_chroma_dev(dc.ptr, dp.ptr, w, h, 8, dru.ptr, drv.ptr)
    codec.recon_chroma_dev(dp.ptr, dru.ptr, drv.ptr, w, h, 8, drec.ptr)
    codec.satd8x8_chroma_from_tiles_dev(dc.ptr, dp.ptr, w, h, dsu.ptr, dsv.ptr)
    codec.stream_sync()
    mv = db.download(np.uint8, nb * 8).view(np.int16).reshape(nb, 4)[:, :2]
    assert (mv == [-4, 6]).all(axis=1).mean() > 0.5
    pred = dp.download(np.uint8, w * h * 2)
    _, pu, pv = oracle.conv_output_420(pred, w, h)
    wu, wv, _ = _mcc_np(ref[1], ref[2], mv, w, h)
    assert np.array_equal(pu, wu) and np.array_equal(pv, wv)
    rec = drec.download(np.uint8, w * h * 2).reshape(-1, 512)
    assert np.array_equal(rec[:, 256:384], ct.reshape(-1, 512)[:, 256:384])
    blocks = lambda d: d.reshape(h // 16, 8, w // 16, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    for got, c, p in ((dsu, cur[1], pu), (dsv, cur[2], pv)):
        res = (c.astype(np.int16) - p.astype(np.int16))
        assert np.array_equal(got.download(np.uint32, nt), oracle.satd8x8(blocks(res)))


@gpu
def test_inter_loop_in_a_graph(codec, oracle, loop_frames):
    """reserve scratch -> search from tiles -> xMotionCompDev -> xTransformCtuFromTilesDev -> xTransformCtuToTilesDev(.., pred, ..,
    pred), recorded once and replayed twice: the same bytes as the eager calls"""
    w, h, cur, ref, ct, rt = loop_frames
    rng, nb, n = 16, (w // 8) * (h // 8), codec.ctu_count(w, h)
    cls = (np.arange(6 * n) % 4).astype(np.uint8)                         # DCT-II of sizes 4, 8, 16, 32 in turn
    start = sentinels(w, h, 81)
    dc, dr, dk = dev(codec, ct), dev(codec, rt), dev(codec, cls)
    db, dp, dz = codec.alloc(nb * 8), dev(codec, start), codec.alloc(n * 12288)
    st = codec.stream_create()
    try:
        codec._check(codec.L.xHipMeScratchReserve(codec.ctx, st, w, h), "xHipMeScratchReserve")

        def enqueue():
            codec.satd_search_from_tiles_dev(dc.ptr, dr.ptr, w, h, rng, db.ptr, stream=st)
            codec.motion_comp_dev(dr.ptr, db.ptr, w, h, dp.ptr, stream=st)
            codec.transform_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dk.ptr, dz.ptr, stream=st)
            codec.transform_ctu_to_tiles_dev(dz.ptr, dk.ptr, dp.ptr, w, h, dp.ptr, stream=st)

        def results():
            codec.stream_sync(st)
            return db.download(np.uint8, nb * 8), dp.download(np.uint8, w * h * 2), dz.download(np.uint8, n * 12288)

        codec.graph_begin(st)
        enqueue()
        graph = codec.graph_end(st)
        try:
            enqueue()
            eager = results()
            mv = eager[0].view(np.int16).reshape(nb, 4)[:, :2]
            want = codec.motion_comp(rt, mv, w, h, base=start)
            coef = codec.transform_ctu_from_tiles(ct, want, w, h, cls)
            assert np.array_equal(eager[2].view(np.int16).reshape(n, 6, 1024), coef)
            assert np.array_equal(eager[1], codec.transform_ctu_to_tiles(coef, cls, want, w, h, base=start))
            assert np.array_equal(eager[1].reshape(-1, 512)[:, 384:], start.reshape(-1, 512)[:, 384:])
            for _ in range(2):
                for buf in (db, dz):
                    buf.upload(np.zeros(buf.nbytes, np.uint8))
                dp.upload(start)
                codec.graph_launch(graph, st)
                for a, b in zip(eager, results()):
                    assert np.array_equal(a, b)
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 5. beyond 4 GiB ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_chroma_beyond_4_gib(codec):
    """A 65568 x 32768 frame (8 392 704 tiles = 4.3 GB per tile array), device-filled (U bytes random, V bytes 0 / 255): 32x32
    regions at the start, around the tile whose byte offset is 2^32 and at the far corners, against the convention evaluated
    sample by sample over the tiles each block reads; m_Y and m_I untouched"""
    w, h = 65536 + 32, 32768
    cw, ch = w // 2, h // 2
    tiles_x, nt, bw, nb = w // 16, (w // 16) * (h // 16), w // 8, (w // 8) * (h // 8)
    assert nt * 512 > (1 << 32)
    d_ref, d_pred = codec.alloc(nt * 512), codec.alloc(nt * 512)
    codec.fill_residual_dev(d_ref.ptr, nt * 256, 0xE4)
    codec.fill_residual_dev(d_pred.ptr, nt * 256, 0xE5)
    mv = _mv_mix(nb, w, h, 0xE6)
    d_mv = dev(codec, records(mv))

    def fetch(buf, byte_off, count):
        out = np.empty(count, np.uint8)
        codec._check(codec.L.xHipMemcpyD2H(codec.ctx, out.ctypes.data, buf.ptr + byte_off, count), "D2H")
        return out

    t_edge = (1 << 32) // 512
    regions = [(0, 0), (t_edge // tiles_x // 2, (t_edge % tiles_x) // 2), (h // 32 - 1, w // 32 - 1), (h // 32 - 1, 0), (0, w // 32 - 1)]
    tile_ids = lambda by, bx: [(2 * by + j) * tiles_x + 2 * bx + i for j in (0, 1) for i in (0, 1)]
    before = {(by, bx): [fetch(d_pred, t * 512, 512) for t in tile_ids(by, bx)] for by, bx in regions}
    codec.motion_comp_chroma_dev(d_ref.ptr, d_mv.ptr, w, h, d_pred.ptr)
    codec.stream_sync()
    cache = {}

    def sampler(plane):
        def S(y, x):
            y, x = min(max(y, 0), ch - 1), min(max(x, 0), cw - 1)
            t = (y >> 3) * tiles_x + (x >> 3)
            if t not in cache:
                cache[t] = fetch(d_ref, t * 512 + 256, 128)
            return int(cache[t][(y & 7) * 16 + (x & 7) * 2 + plane])
        return S

    S = (sampler(0), sampler(1))
    classes = set()
    for by, bx in regions:
        got = [fetch(d_pred, t * 512, 512) for t in tile_ids(by, bx)]
        for k, (g, b) in enumerate(zip(got, before[(by, bx)])):
            assert np.array_equal(g[:256], b[:256]) and np.array_equal(g[384:], b[384:]), (by, bx)   # m_Y / m_I untouched
            ty, tx = 2 * by + k // 2, 2 * bx + k % 2
            for y in range(8):
                for x in range(8):
                    gy, gx = 8 * ty + y, 8 * tx + x
                    mvx, mvy = (int(v) for v in mv[(gy // 4) * bw + gx // 4])
                    classes.add((mvx & 1, mvy & 1))
                    for plane in (0, 1):
                        want = min(max(_mcc_sample(S[plane], gx, gy, mvx, mvy)[0], 0), 255)
                        assert g[256 + 16 * y + 2 * x + plane] == want, (by, bx, gy, gx, plane)
    assert len(classes) == 4


# ---- 6. argument errors ------------------------------------------------------------------------------------------------------------------
@gpu
def test_argument_errors(codec):
    L, ctx = codec.L, codec.ctx
    buf = codec.alloc(1 << 22)
    p = buf.ptr
    r = p + (1 << 20)                                # a 64x64 tile array (8 KiB)
    b, m = p + (2 << 20), p + (3 << 20)              # records, and a prediction tile array
    E = -1                                           # X266HIP_EINVAL
    for fn in (L.xMotionCompChromaDev, L.xMotionCompDev):
        assert fn(ctx, r, b, 56, 64, m, None) == E
        assert fn(ctx, r, b, 64, 8, m, None) == E
        assert fn(ctx, r, b, 0, 64, m, None) == E
        assert fn(ctx, None, b, 64, 64, m, None) == E
        assert fn(ctx, r, None, 64, 64, m, None) == E
        assert fn(ctx, r, b, 64, 64, None, None) == E
        assert fn(ctx, r + 8, b, 64, 64, m, None) == E
        assert fn(ctx, r, b + 4, 64, 64, m, None) == E
        assert fn(ctx, r, b, 64, 64, m + 8, None) == E
        assert fn(ctx, r, b, 64, 64, r, None) == E        # in place
        assert fn(ctx, r, b, 64, 64, r + 4096, None) == E  # partial overlap with ref
        assert fn(ctx, r, b, 64, 64, r - 4096, None) == E
        assert fn(ctx, r, b, 64, 64, b - 8192 + 16, None) == E   # pred runs into the records
        assert fn(ctx, r, m - 256, 64, 64, m, None) == E   # records run into pred
        assert fn(ctx, r, b, 64, 64, m, None) == 0
    codec.stream_sync()
