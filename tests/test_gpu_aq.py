"""GPU (-m gpu): source analysis (xAqStatsGpu, xAqDecideGpu, and xWeightsFromTotals behind them) against tests/_aq_ref.py, bit-exact.
Every buffer of every call sits between the guard bands of tests/_arena.py at exactly its documented alignment; the guards and the
inputs are checked after every call."""
import ctypes
import functools

import numpy as np
import pytest

import _aq_ref as R
import x266_amd
from _arena import Arena
from _dev import EINVAL, call_struct, dev, sync_or_exit

pytestmark = pytest.mark.gpu

try:
    CHUNK = x266_amd.aq_totals_chunk()                                      # the totals' step, as the implementation exposes it
except (x266_amd.X266Error, AttributeError):                                # collected without a built library: the GPU tests then fail on their own
    CHUNK = 1024
PTRS = {"d_src": 16, "d_tile": 16, "d_total": 8, "d_offset": 2, "d_qp": 1}
DISP = {name: align * (2 * i + 1) for i, (name, align) in enumerate(PTRS.items())}          # exactly the documented alignment, no more
SIZES = [(16, 16), (48, 80), (64, 64), (144, 80)]
TALL = [(16, 16 * n) for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)]


@functools.lru_cache(None)
def frame(kind, w, h):
    """(tiles, records, totals): the reference is computed once per frame and shared"""
    if kind == "zeros":
        t = R.constant_frame(w, h, 0)
    elif kind == "ones":
        t = R.constant_frame(w, h, 255)
    elif kind == "max":
        t = R.max_energy_frame(w, h)
    elif kind == "noise":
        t = R.noise_frame(w, h, 0xA0 + w + h)
    elif kind == "halves":
        t = R.halves_frame(w, h, 0xB0 + w + h)
    else:
        t = R.distinct_frame(w, h)
    rec = R.tile_stats(t)
    for a in (t, rec):
        a.setflags(write=False)
    return t, rec, R.totals(rec)


def stats(codec, tiles, w, h, want, stream=None, guard_seed=41):
    """the call inside an arena, held against the reference's records `want`: every record and the totals"""
    n = want.size
    a = Arena(codec)
    src = a.input("d_src", tiles, 16, DISP["d_src"], guard_seed)
    tile = a.output("d_tile", 32 * n, 16, DISP["d_tile"])
    total = a.output("d_total", 64, 8, DISP["d_total"])
    p = codec.aq_params(src.ptr, tile.ptr, total.ptr, 0, 0, w, h, mode=0, strength_q8=-1, qp=99, chroma_qp_offset=99)   # stats reads no scalar
    call_struct(codec, "xAqStatsGpu", p, stream)
    got = a.check()                                                         # guard bands and the input
    rec, tot = got["d_tile"].view(R.TILE_DTYPE), got["d_total"].view(np.int64)
    bad = np.flatnonzero(rec != want)
    assert bad.size == 0, (bad[:4], rec[bad[:4]], want[bad[:4]])
    assert tot.tolist() == R.totals(want).tolist(), (tot, R.totals(want))
    return rec, tot


def decide(codec, rec, tot, w, h, mode, strength, qp=30, chroma=0, offset=True, qps=True, stream=None, guard_seed=51):
    """the call inside an arena, held against the reference: the Q8 offsets and the qp bytes, whichever are asked for"""
    want_off, want_qp = R.decide(rec, tot, w, h, mode, strength, qp, chroma)
    a, s = Arena(codec), {}
    s["d_tile"] = a.input("d_tile", np.ascontiguousarray(rec).view(np.uint8), 16, DISP["d_tile"], guard_seed)
    s["d_total"] = a.input("d_total", np.ascontiguousarray(tot, np.int64), 8, DISP["d_total"], guard_seed + 1)
    if offset:
        s["d_offset"] = a.output("d_offset", want_off.nbytes, 2, DISP["d_offset"])
    if qps:
        s["d_qp"] = a.output("d_qp", want_qp.nbytes, 1, DISP["d_qp"])
    p = codec.aq_params(0, s["d_tile"].ptr, s["d_total"].ptr, s["d_offset"].ptr if offset else 0, s["d_qp"].ptr if qps else 0, w, h, mode, strength, qp, chroma)
    call_struct(codec, "xAqDecideGpu", p, stream)
    got = a.check()
    if offset:
        off = got["d_offset"].view(np.int16)
        bad = np.flatnonzero(off != want_off)
        assert bad.size == 0, (bad[:8], off[bad[:8]], want_off[bad[:8]])
    if qps:
        bad = np.flatnonzero(got["d_qp"] != want_qp)
        assert bad.size == 0, (bad[:8], got["d_qp"][bad[:8]], want_qp[bad[:8]])
    return want_off, want_qp


# ---- 1. frame sizes: one tile, tile counts off the wave's four, cut CTUs, tile counts around the totals' step -------------------------------
@pytest.mark.parametrize("w,h", SIZES + TALL)
def test_frame_sizes(codec, w, h):
    assert CHUNK == x266_amd.aq_totals_chunk() and codec.L.xAqTotalsChunk() == CHUNK
    tiles, want, _ = frame("noise", w, h)
    rec, tot = stats(codec, tiles, w, h, want)
    assert int(tot[7]) == (w // 16) * (h // 16)
    for mode in (1, 2):
        decide(codec, rec, tot, w, h, mode, 256)


# ---- 2. contents ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(48, 80), (144, 80)])
@pytest.mark.parametrize("kind", ["zeros", "ones", "max", "halves", "distinct"])
def test_contents(codec, kind, w, h):
    tiles, want, _ = frame(kind, w, h)
    for seed in (41, 77):                                                   # whatever lies around the frame must not reach a record
        rec, tot = stats(codec, tiles, w, h, want, guard_seed=seed)
    if kind in ("zeros", "ones"):
        assert not rec["energy"].any() and not rec["log2_q8"].any() and int(rec["sum_y"][0]) == (65280 if kind == "ones" else 0)
    if kind == "max":
        assert (rec["energy"] == R.MAX_ENERGY).all() and (rec["log2_q8"] == 5778).all()
    if kind == "distinct":                                                  # no sample of a neighbouring tile in any sum
        i = np.arange(rec.size)
        assert np.array_equal(rec["sum_y"], 256 * ((7 * i + 3) % 256)) and np.array_equal(rec["sum_u"], 64 * ((11 * i + 5) % 256))
        assert np.array_equal(rec["sum_v"], 64 * ((13 * i + 1) % 256)) and not rec["energy"].any()
    for mode in (1, 2):
        decide(codec, rec, tot, w, h, mode, 256)


@pytest.mark.parametrize("w,h", [(16, 16), (48, 80), (144, 80)])
def test_modes_strengths_and_clamps(codec, w, h):
    tiles, rec, tot = frame("halves", w, h)
    maps = {}
    for mode in (1, 2):
        for strength in (0, 256, 1024):
            off, qp = decide(codec, rec, tot, w, h, mode, strength, qp=30)
            maps[mode, strength] = qp
            if strength == 0:
                assert (qp == 30).all() and not off.any()                     # every qp is the base
        for base, chroma in ((0, -12), (0, 12), (51, -12), (51, 12)):
            off, qp = decide(codec, rec, tot, w, h, mode, 1024, qp=base, chroma=chroma)
            assert qp.min() >= 0 and qp.max() <= 51
    if w > 16:                                                               # the modes differ, the strengths differ, delta takes both signs
        assert not np.array_equal(maps[1, 256], maps[2, 256])
        assert not np.array_equal(maps[1, 256], maps[1, 1024]) and not np.array_equal(maps[2, 256], maps[2, 1024])
        d = maps[2, 256].astype(int) - 30
        assert d.min() < 0 < d.max()


def test_either_output_alone(codec):
    w, h = 144, 80
    tiles, rec, tot = frame("halves", w, h)
    decide(codec, rec, tot, w, h, 2, 256, offset=True, qps=False)
    decide(codec, rec, tot, w, h, 2, 256, offset=False, qps=True)
    decide(codec, rec, tot, w, h, 2, 256, offset=True, qps=True)
    for seed in (51, 91):                                                    # records behind the frame's last are not read
        decide(codec, rec, tot, w, h, 1, 1024, guard_seed=seed)


# ---- 3. the same bytes on every run -----------------------------------------------------------------------------------------------------------
def test_two_runs_on_two_streams_give_identical_bytes(codec):
    w, h = 144, 80
    tiles, want, _ = frame("noise", w, h)
    streams = [codec.stream_create(), codec.stream_create()]
    try:
        runs = [stats(codec, tiles, w, h, want, stream=st) for st in streams]
    finally:
        for st in streams:
            codec.stream_destroy(st)
    for a, b in zip(runs[0], runs[1]):
        assert a.tobytes() == b.tobytes()


def test_numpy_conveniences(codec):
    w, h = 48, 80
    tiles, want, want_tot = frame("halves", w, h)
    rec, tot = codec.aq_stats(tiles, w, h)
    assert np.array_equal(rec, want) and tot.tolist() == want_tot.tolist() and rec.dtype == x266_amd.AQ_TILE_DTYPE
    off, qp = codec.aq_decide(rec, tot, w, h, mode=2, strength_q8=300, qp=27, chroma_qp_offset=3)
    want_off, want_qp = R.decide(want, want_tot, w, h, 2, 300, 27, 3)
    assert np.array_equal(off, want_off) and np.array_equal(qp.ravel(), want_qp)


# ---- 4. one graph -------------------------------------------------------------------------------------------------------------------------------
def test_stats_and_decide_in_one_graph(codec):
    w, h = 144, 80
    n, n_ctu = 45, 6
    inputs = [frame("halves", w, h), frame("noise", w, h)]
    d_src, d_tile, d_tot, d_off, d_qp = codec.alloc(n * 512), codec.alloc(n * 32), codec.alloc(64), codec.alloc(n * 2), codec.alloc(n_ctu * 6)
    p = codec.aq_params(d_src.ptr, d_tile.ptr, d_tot.ptr, d_off.ptr, d_qp.ptr, w, h, 2, 256, 30, -1)
    st = codec.stream_create()
    try:
        d_src.upload(inputs[0][0])
        codec.graph_begin(st)
        codec.aq_stats_dev(p, stream=st)
        codec.aq_decide_dev(p, stream=st)                                   # reads the records and the totals on the device
        graph = codec.graph_end(st)
        try:
            for i in (1, 0):                                                 # replayed twice, on other data than it was captured with
                tiles, rec, tot = inputs[i]
                d_src.upload(tiles)
                d_tile.upload(np.full(n * 32, 0x5A, np.uint8))
                d_off.upload(np.full(n, 0x5A5A, np.int16))
                codec.graph_launch(graph, st)
                sync_or_exit(codec, 0, st)
                want_off, want_qp = R.decide(rec, tot, w, h, 2, 256, 30, -1)
                assert d_tot.download(np.int64, 8).tolist() == tot.tolist()
                assert np.array_equal(d_tile.download(np.uint8, n * 32).view(R.TILE_DTYPE), rec)
                assert np.array_equal(d_off.download(np.int16, n), want_off)
                assert np.array_equal(d_qp.download(np.uint8, n_ctu * 6), want_qp)
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 5. refusals through the ABI --------------------------------------------------------------------------------------------------------------
def test_argument_errors(codec):
    """every rule once per call: X266HIP_EINVAL, the call named in the error text, nothing launched, the buffers untouched"""
    L, ctx = codec.L, codec.ctx
    M = 1 << 20
    buf = codec.alloc(6 * M)
    fill = np.random.RandomState(9).randint(1, 255, 6 * M).astype(np.uint8)
    buf.upload(fill)
    w, h, n, n_ctu = 144, 80, 45, 6
    src, tile, tot, off, qp = (buf.ptr + i * M for i in range(1, 6))
    good = dict(d_src=src, d_tile=tile, d_total=tot, d_offset=off, d_qp=qp, width=w, height=h, mode=2, strength_q8=256, qp=30, chroma_qp_offset=0)
    extent = dict(d_src=n * 512, d_tile=n * 32, d_total=64, d_offset=n * 2, d_qp=n_ctu * 6)

    def refused(name, **change):
        p = codec.aq_params(**dict(good, **change))
        assert getattr(L, name)(ctx, ctypes.byref(p), None) == EINVAL, (name, change)
        assert name.encode() in L.xHipLastError(ctx), (name, change)

    for name in ("xAqStatsGpu", "xAqDecideGpu"):
        assert getattr(L, name)(ctx, None, None) == EINVAL and name.encode() in L.xHipLastError(ctx)    # NULL p
        assert getattr(L, name)(None, ctypes.byref(codec.aq_params(**good)), None) == EINVAL
        for field in ("d_tile", "d_total"):
            refused(name, **{field: 0})
            refused(name, **{field: good[field] + PTRS[field] // 2})
            refused(name, **{field: 2 ** 64 - PTRS[field]})                  # aligned, and the extent does not fit behind it
        for side in ("width", "height"):
            for v in (0, -16, 8, 152 if side == "width" else 88):
                refused(name, **{side: v})
    refused("xAqStatsGpu", d_src=0)
    refused("xAqStatsGpu", d_src=src + 8)
    refused("xAqStatsGpu", d_src=2 ** 64 - 16)
    for field, other in (("d_tile", "d_src"), ("d_total", "d_src"), ("d_total", "d_tile"), ("d_tile", "d_total")):
        refused("xAqStatsGpu", **{field: good[other] + (extent[other] - 1) // PTRS[field] * PTRS[field]})   # onto the other's last bytes
        refused("xAqStatsGpu", **{field: good[other]})
    refused("xAqDecideGpu", d_offset=0, d_qp=0)
    refused("xAqDecideGpu", d_offset=off + 1)
    refused("xAqDecideGpu", d_offset=2 ** 64 - 2)
    refused("xAqDecideGpu", d_qp=2 ** 64 - 1)
    for change in (dict(mode=0), dict(mode=3), dict(strength_q8=-1), dict(strength_q8=1025), dict(qp=-1), dict(qp=52), dict(chroma_qp_offset=-13),
                   dict(chroma_qp_offset=13)):
        refused("xAqDecideGpu", **change)
    for field, other in (("d_offset", "d_tile"), ("d_offset", "d_total"), ("d_offset", "d_qp"), ("d_qp", "d_tile"), ("d_qp", "d_total"), ("d_qp", "d_offset")):
        refused("xAqDecideGpu", **{field: good[other] + (extent[other] - 1) // PTRS[field] * PTRS[field]})
        refused("xAqDecideGpu", **{field: good[other]})
    sync_or_exit(codec, 0)
    assert np.array_equal(buf.download(np.uint8, 6 * M), fill)             # nothing was launched
    # the edges of what is accepted: decide without d_src and with one output, every scalar at either end of its range
    tiles, rec, total = frame("halves", w, h)
    buf.upload(np.concatenate([fill[:M], tiles.ravel()]))
    for p in (codec.aq_params(**dict(good, d_offset=0, d_qp=0, mode=7)), ):
        rc = L.xAqStatsGpu(ctx, ctypes.byref(p), None)
        sync_or_exit(codec, rc)
        assert rc == 0, L.xHipLastError(ctx)
    for change in (dict(d_src=0, d_qp=0, mode=1, strength_q8=0, qp=0, chroma_qp_offset=-12), dict(d_src=3, d_offset=0, mode=2, strength_q8=1024, qp=51, chroma_qp_offset=12)):
        p = codec.aq_params(**dict(good, **change))
        rc = L.xAqDecideGpu(ctx, ctypes.byref(p), None)
        sync_or_exit(codec, rc)
        assert rc == 0, (change, L.xHipLastError(ctx))
    now = buf.download(np.uint8, 6 * M)
    assert np.array_equal(now[2 * M:2 * M + n * 32].view(R.TILE_DTYPE), rec) and now[3 * M:3 * M + 64].view(np.int64).tolist() == total.tolist()
    assert np.array_equal(now[4 * M:4 * M + 2 * n].view(np.int16), R.decide(rec, total, w, h, 1, 0, 0, -12)[0])
    assert np.array_equal(now[5 * M:5 * M + 6 * n_ctu], R.decide(rec, total, w, h, 2, 1024, 51, 12)[1])
    for lo, size in ((2 * M, n * 32), (3 * M, 64), (4 * M, 2 * n), (5 * M, 6 * n_ctu), (M, n * 512)):
        now[lo:lo + size] = fill[lo:lo + size]
    assert np.array_equal(now, fill)                                        # ... and nothing else was written


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------------
def test_the_qp_map_feeds_the_fused_coding_call(codec):
    """aq_decide's d_qp goes into xDct32CodeCtuTilesGpu without leaving the device; the result is that of the reference's qp bytes"""
    from test_gpu_quant import _tiles_mix
    w, h = 128, 64
    n, n_ctu = 32, 2
    cur, _, _ = frame("halves", w, h)
    pred, base = _tiles_mix(w, h, 0x7A00), _tiles_mix(w, h, 0x7A01)
    dc, dp, dr = dev(codec, cur), dev(codec, pred), dev(codec, base)
    d_tile, d_tot, d_qp = codec.alloc(n * 32), codec.alloc(64), codec.alloc(16)
    dl, dn = codec.alloc(n_ctu * 12288), codec.alloc(n_ctu * 24)
    p = codec.aq_params(dc.ptr, d_tile.ptr, d_tot.ptr, 0, d_qp.ptr, w, h, 2, 256, 30, 2)
    codec.aq_stats_dev(p)
    codec.aq_decide_dev(p)
    codec.dct32_code_ctu_tiles_dev(dc.ptr, dp.ptr, w, h, d_qp.ptr, 0, 171, dl.ptr, dn.ptr, dr.ptr)
    sync_or_exit(codec, 0)
    rec = R.tile_stats(cur)
    want_qp = R.decide(rec, R.totals(rec), w, h, 2, 256, 30, 2)[1]
    assert len(set(want_qp.tolist())) > 2                                    # a map, not a flat qp
    assert np.array_equal(d_qp.download(np.uint8, 6 * n_ctu), want_qp)
    level, nnz, recon = codec.code_ctu_tiles(cur, pred, w, h, qps=want_qp, rounding=171, base=base)
    assert np.array_equal(dl.download(np.int16, n_ctu * 6144).reshape(n_ctu, 6, 1024), level) and level.any()
    assert np.array_equal(dn.download(np.uint32, 6 * n_ctu).reshape(n_ctu, 6), nnz)
    assert np.array_equal(dr.download(np.uint8, w * h * 2), recon)


def test_fade_weights_end_to_end(codec):
    """the totals of a faded frame and of its reference give weights under which the list-0 prediction is closer to the faded frame
    than the default prediction"""
    w, h = 64, 64
    ref, _, _ = frame("noise", w, h)
    cur = ref.copy()
    cur[:, :384] = ((ref[:, :384].astype(np.int64) * 96 + 64) >> 7) + 10
    rec_c, tot_c = codec.aq_stats(cur, w, h)
    rec_r, tot_r = codec.aq_stats(ref, w, h)
    assert np.array_equal(rec_c, R.tile_stats(cur)) and tot_r.tolist() == R.totals(R.tile_stats(ref)).tolist()
    wp = codec.weights_from_totals(tot_c, tot_r, 0, (7, 7))
    want_w, want_o = R.weights(tot_c, tot_r, (7, 7))
    assert [wp.w[0][i] for i in range(3)] == want_w and [wp.o[0][i] for i in range(3)] == want_o
    nb = (w // 8) * (h // 8)
    zero, one = np.zeros((nb, 2), np.int16), np.ones(nb, np.uint8)
    weighted = codec.motion_comp_bi_qpel(ref, None, zero, zero, w, h, direction=one, wp=wp).reshape(-1, 512)
    default = codec.motion_comp_bi_qpel(ref, None, zero, zero, w, h, direction=one, wp=None).reshape(-1, 512)
    assert np.array_equal(default[:, :384], ref[:, :384])
    sae = lambda a: int(np.abs(a[:, :384].astype(np.int64) - cur[:, :384].astype(np.int64)).sum())
    print("fade: summed absolute error weighted %d, default %d" % (sae(weighted), sae(default)))
    assert sae(weighted) < sae(default)
