"""GPU (-m gpu): the lookahead (xLaDownscaleGpu, xLaIntraCostsGpu, xLaFrameCostGpu, xLaPropagateGpu, xLaTreeQpGpu, and xSceneCutFromTotals
behind them) against tests/_la_ref.py, bit-exact.  Every buffer of every call sits between the guard bands of tests/_arena.py at exactly
its documented alignment; the guards and the inputs are checked after every call."""
import ctypes
import functools

import numpy as np
import pytest

import _aq_ref as A
import _la_ref as R
import x266_amd
from _arena import Arena
from _dev import EINVAL, call_struct, dev, same, sync_or_exit

pytestmark = pytest.mark.gpu

try:
    CHUNK = x266_amd.la_totals_chunk()                                      # the totals' step, as the implementation exposes it
except (x266_amd.X266Error, AttributeError):                                # collected without a built library: the GPU tests then fail on their own
    CHUNK = 2048
PTRS = {"d_src": 16, "d_low": 16, "d_intra": 4, "d_mode": 1, "d_inter0": 8, "d_inter1": 8, "d_block": 16, "d_total": 8, "d_prop": 8, "d_prop_ref0": 8,
        "d_prop_ref1": 8, "d_aq_offset": 2, "d_offset": 2, "d_qp": 1}
DISP = {name: align * (2 * i + 1) for i, (name, align) in enumerate(PTRS.items())}          # exactly the documented alignment, no more
SIZES = [(32, 32), (64, 32), (32, 64), (96, 160), (160, 96)]
# n = (w / 16) (h / 16) is a multiple of 4 (both sides are multiples of 32): CHUNK - 4 and CHUNK + 4 are the block counts next to the totals'
# step, 2 CHUNK + 12 is two full steps and a ragged one
TALL = [(32, 8 * n) for n in (CHUNK - 4, CHUNK, CHUNK + 4, 2 * CHUNK + 12)]
KINDS = ["zeros", "ones", "random", "hramp", "vramp", "checker"]
M_I = np.arange(512) >= 384                                                 # a tile's info bytes: no lookahead call reads or writes them


@functools.lru_cache(None)
def ref(kind, w, h):
    """(tiles, lowres tiles, intra costs, modes) of the reference, computed once per frame and shared"""
    tiles = R.frame(kind, w, h)
    low = R.downscale(tiles, w, h)
    cost, mode = R.intra_costs(low, w, h)
    for a in (tiles, low, cost, mode):
        a.setflags(write=False)
    return tiles, low, cost, mode


lists = R.lists                                                             # the recipe lives with the frames the CPU and GPU tests share


# ---- the calls inside an arena, each held against the reference ---------------------------------------------------------------------------------
def downscale(codec, tiles, w, h, want, stream=None, guard_seed=41):
    a = Arena(codec)
    src = a.input("d_src", tiles, 16, DISP["d_src"], guard_seed)
    low = a.output("d_low", want.size, 16, DISP["d_low"], written=~np.tile(M_I, want.size // 512))
    call_struct(codec, "xLaDownscaleGpu", codec.la_params(w, h, -1, -1, 99, 99, d_src=src.ptr, d_low=low.ptr), stream)    # it reads no scalar
    got = a.check()["d_low"].reshape(-1, 512)                               # guard bands, the input, and m_I untouched
    same(got[:, :384], want.reshape(-1, 512)[:, :384], "d_low")
    return got


def intra_costs(codec, low, w, h, want_cost, want_mode, with_mode=True, guard_seed=43):
    a = Arena(codec)
    d_low = a.input("d_low", low, 16, DISP["d_low"], guard_seed)
    d_intra = a.output("d_intra", 4 * want_cost.size, 4, DISP["d_intra"])
    d_mode = a.output("d_mode", want_cost.size, 1, DISP["d_mode"]) if with_mode else None
    call_struct(codec, "xLaIntraCostsGpu", codec.la_params(w, h, -1, -1, 99, 99, d_low=d_low.ptr, d_intra=d_intra.ptr, d_mode=d_mode.ptr if with_mode else 0))
    got = a.check()
    same(got["d_intra"].view(np.uint32), want_cost, "d_intra")
    if with_mode:
        same(got["d_mode"], want_mode, "d_mode")


def frame_cost(codec, intra, mode, l0, l1, w, h, penalty, stream=None, guard_seed=45):
    want, want_tot = R.frame_cost(intra, mode, l0, l1, penalty)
    a, s = Arena(codec), {}
    for name, data in (("d_intra", intra), ("d_mode", mode), ("d_inter0", l0), ("d_inter1", l1)):
        s[name] = 0 if data is None else a.input(name, np.ascontiguousarray(data).view(np.uint8), PTRS[name], DISP[name], guard_seed + len(s)).ptr
    block = a.output("d_block", 16 * intra.size, 16, DISP["d_block"])
    total = a.output("d_total", 64, 8, DISP["d_total"])
    call_struct(codec, "xLaFrameCostGpu", codec.la_params(w, h, penalty, -1, 99, 99, d_block=block.ptr, d_total=total.ptr, **s), stream)
    got = a.check()
    same(got["d_block"].view(R.BLOCK_DTYPE), want, "d_block")
    assert got["d_total"].view(np.int64).tolist() == want_tot.tolist(), (got["d_total"].view(np.int64), want_tot)
    return want, want_tot


def propagate(codec, rec, prop, ref0, ref1, w, h, stream=None, guard_seed=47):
    """ref0 / ref1: the accumulators as they stand, or None for a NULL target; returns the reference's"""
    want = R.propagate(rec, prop, ref0, ref1, w, h)
    a, s = Arena(codec), {}
    s["d_block"] = a.input("d_block", np.ascontiguousarray(rec).view(np.uint8), 16, DISP["d_block"], guard_seed).ptr
    if prop is not None:
        s["d_prop"] = a.input("d_prop", np.ascontiguousarray(prop, np.uint64).view(np.uint8), 8, DISP["d_prop"], guard_seed + 1).ptr
    slots = {}
    for name, acc in (("d_prop_ref0", ref0), ("d_prop_ref1", ref1)):
        if acc is not None:                                                 # an accumulator is read and written: an output slot that starts as `acc`
            slots[name] = a.output(name, 8 * rec.size, 8, DISP[name])
            start = slots[name].start
            slots[name].image[start:start + 8 * rec.size] = np.ascontiguousarray(acc, np.uint64).view(np.uint8)
            slots[name].buf.upload(slots[name].image)
            s[name] = slots[name].ptr
    call_struct(codec, "xLaPropagateGpu", codec.la_params(w, h, -1, -1, 99, 99, **s), stream)
    got = a.check()                                                         # the guard bands prove that nothing outside the grid was written
    for name, acc in zip(("d_prop_ref0", "d_prop_ref1"), want):
        if acc is not None:
            same(got[name].view(np.uint64), acc, name)
    return want


def tree_qp(codec, rec, prop, aq, w, h, strength, qp=30, chroma=0, offset=True, qps=True, guard_seed=49):
    want_off, want_qp = R.tree_qp(rec, prop, aq, w, h, strength, qp, chroma)
    a, s = Arena(codec), {}
    s["d_block"] = a.input("d_block", np.ascontiguousarray(rec).view(np.uint8), 16, DISP["d_block"], guard_seed).ptr
    if prop is not None:
        s["d_prop"] = a.input("d_prop", np.ascontiguousarray(prop, np.uint64).view(np.uint8), 8, DISP["d_prop"], guard_seed + 1).ptr
    if aq is not None:
        s["d_aq_offset"] = a.input("d_aq_offset", np.ascontiguousarray(aq, np.int16).view(np.uint8), 2, DISP["d_aq_offset"], guard_seed + 2).ptr
    if offset:
        s["d_offset"] = a.output("d_offset", want_off.nbytes, 2, DISP["d_offset"]).ptr
    if qps:
        s["d_qp"] = a.output("d_qp", want_qp.nbytes, 1, DISP["d_qp"]).ptr
    call_struct(codec, "xLaTreeQpGpu", codec.la_params(w, h, -1, strength, qp, chroma, **s))
    got = a.check()
    if offset:
        same(got["d_offset"].view(np.int16), want_off, "d_offset")
    if qps:
        same(got["d_qp"], want_qp, "d_qp")
    return want_off, want_qp


# ---- 1. sizes and contents: downscale and intra costs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_downscale_and_intra_costs(codec, w, h, kind):
    tiles, low, cost, mode = ref(kind, w, h)
    for seed in (41, 77):                                                   # whatever lies around the frame must not reach the result
        got = downscale(codec, tiles, w, h, low, guard_seed=seed)
    intra_costs(codec, got, w, h, cost, mode)                                # on the device's own lowres frame, m_I the arena's fill
    intra_costs(codec, low, w, h, cost, mode, with_mode=False, guard_seed=91)
    if kind in ("zeros", "ones"):
        assert not cost[1:].any() and not mode.any() and cost[0] == R.satd8x8(np.full((8, 8), (0 if kind == "zeros" else 255) - 128))
    if kind == "checker":
        assert cost.max() >= 2048 and cost.max() <= 32640


@pytest.mark.parametrize("w,h", TALL)
def test_a_frame_past_the_totals_step(codec, w, h):
    n = (w // 16) * (h // 16)
    assert CHUNK == x266_amd.la_totals_chunk() and codec.L.xLaTotalsChunk() == CHUNK
    assert n in (CHUNK - 4, CHUNK, CHUNK + 4, 2 * CHUNK + 12)
    tiles, low, cost, mode = ref("random", w, h)
    downscale(codec, tiles, w, h, low)
    intra_costs(codec, low, w, h, cost, mode)
    l0, l1 = lists(cost, 5)
    rec, tot = frame_cost(codec, cost, mode, l0, l1, w, h, 300)
    assert int(tot[7]) == n and tot[2] and tot[3] and tot[4]
    prop = np.random.RandomState(6).randint(0, 1 << 20, rec.size).astype(np.uint64)
    propagate(codec, rec, prop, np.zeros(rec.size, np.uint64), prop.copy(), w, h)
    tree_qp(codec, rec, prop, None, w, h, 512)


# ---- 2. frame cost ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(32, 32), (96, 160), (160, 96)])
def test_frame_cost_lists_penalties_and_ties(codec, w, h):
    _, _, cost, mode = ref("random", w, h)
    l0, l1 = lists(cost, 7 + w)
    rec, tot = frame_cost(codec, cost, mode, l0, l1, w, h, 300)
    if cost.size >= 16:                                                      # every branch, ties included
        k = np.arange(cost.size) % 8
        assert (rec["kind"][k == 1] != 2).all() and (rec["kind"][k == 4] == 1).all() and set(rec["kind"].tolist()) == {0, 1, 2}
        assert (rec["kind"][k == 2] != 0).all() and (rec["kind"][k == 3] != 0).all()
    for penalty in (0, 65535):
        for a, b in ((l0, l1), (l0, None), (None, l1), (None, None)):
            rec, tot = frame_cost(codec, cost, mode, a, b, w, h, penalty)
            if a is None and b is None:
                assert (rec["kind"] == 0).all() and tot[0] == tot[1] + penalty * cost.size and not tot[5] and not tot[6]
            elif penalty == 65535:
                assert not (rec["kind"] == 0).any()
    frame_cost(codec, cost, None, l0, l1, w, h, 300)                         # d_mode NULL: every mode 0
    frame_cost(codec, cost, mode, l0, l0, w, h, 300)                         # the lists' contents equal: list 0 everywhere it is not intra


# ---- 3. propagate -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def searched(w, h):
    """a frame, a copy moved by (4, -2) and the reference's search of their lowres frames: (cur low, ref low, records)"""
    tiles = R.frame("smooth", w, h)
    cur_low, ref_low = R.downscale(tiles, w, h), R.downscale(R.shifted(tiles, w, h, 4, -2), w, h)
    return cur_low, ref_low, R.search(cur_low, ref_low, w, h, 3)


@pytest.mark.parametrize("w,h", [(96, 160), (160, 96)])
def test_propagate_with_the_vectors_of_a_real_search(codec, w, h):
    cur_low, ref_low, want = searched(w, h)
    n = want.size
    d_cur, d_ref, d_best = codec._upload(cur_low), codec._upload(ref_low), codec.alloc(8 * n)
    codec.satd_search_from_tiles_dev(d_cur.ptr, d_ref.ptr, w // 2, h // 2, 3, d_best.ptr)   # the lowres frame is an ordinary tiled frame
    sync_or_exit(codec, 0)
    got = d_best.download(np.uint8, 8 * n).view(R.ME_DTYPE)
    same(got, want, "the search of the lowres frames")
    assert (got["mvx"] != 0).any() and (got["mvy"] != 0).any()
    cost, mode = R.intra_costs(cur_low, w, h)
    rec, tot = frame_cost(codec, cost, mode, got, None, w, h, 0)
    assert tot[3] > n // 2                                                   # the moved copy predicts most blocks better than intra does
    prop = np.random.RandomState(8).randint(0, 1 << 16, n).astype(np.uint64)
    ref0, _ = propagate(codec, rec, prop, np.zeros(n, np.uint64), None, w, h)
    assert ref0.any()
    propagate(codec, rec, None, ref0, np.zeros(n, np.uint64), w, h)         # d_prop NULL counts as zeros; added INTO what is there


def test_propagate_contention_edges_and_large_values(codec):
    w, h = 160, 96
    bw, bh, n = 10, 6, 60
    rec = np.zeros(n, R.BLOCK_DTYPE)
    rec["intra"], rec["cost"], rec["kind"] = 30000, 1000, 1 + np.arange(n) % 2
    bx, by = np.arange(n) % bw, np.arange(n) // bw
    zeros = np.zeros(n, np.uint64)
    # every block points into block (4, 2), a little off the grid: all adds land on four addresses
    rec["mvx"], rec["mvy"] = 8 * (4 - bx) + 3, 8 * (2 - by) + 5
    prop = np.full(n, 123456, np.uint64)
    ref0, ref1 = propagate(codec, rec, prop, zeros, zeros, w, h)
    assert np.count_nonzero(ref0) == 4 and np.count_nonzero(ref1) == 4
    # vectors of +-64 leave the grid on each of the four sides, whole and in part
    for mvx, mvy in ((-64, 0), (64, 0), (0, -64), (0, 64), (-64, -64), (64, 64), (-61, 59), (61, -59)):
        rec["mvx"], rec["mvy"] = mvx, mvy
        propagate(codec, rec, prop, zeros, zeros, w, h)
    # d_prop at and above 2^32 - 1, accumulators that start high, intra 0 and kind 0 among the blocks
    rec["mvx"], rec["mvy"] = np.random.RandomState(9).randint(-20, 21, n), np.random.RandomState(10).randint(-20, 21, n)
    rec["intra"][::7], rec["kind"][3::7] = 0, 0
    prop = np.array([2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1] * 12, np.uint64)
    start = np.full(n, 2 ** 60, np.uint64)
    a = propagate(codec, rec, prop, start, start, w, h)
    b = propagate(codec, rec, np.minimum(prop, np.uint64(2 ** 32 - 1)), start, start, w, h)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # NULL targets: the blocks of that kind are skipped, the other accumulator is the same as before
    only0, none1 = propagate(codec, rec, prop, start, None, w, h)
    none0, only1 = propagate(codec, rec, prop, None, start, w, h)
    assert none0 is None and none1 is None and np.array_equal(only0, a[0]) and np.array_equal(only1, a[1])
    p = codec.la_params(w, h, d_block=codec._upload(rec.view(np.uint8)).ptr)
    call_struct(codec, "xLaPropagateGpu", p)                                       # both NULL: accepted, nothing to do


def test_two_runs_on_two_streams_give_identical_bytes(codec):
    w, h = 160, 96
    cur_low, ref_low, best = searched(w, h)
    cost, mode = R.intra_costs(cur_low, w, h)
    streams = [codec.stream_create(), codec.stream_create()]
    try:
        runs = []
        for st in streams:
            rec, tot = frame_cost(codec, cost, mode, best, best, w, h, 10, stream=st)
            runs.append((rec, tot, propagate(codec, rec, None, np.zeros(rec.size, np.uint64), np.zeros(rec.size, np.uint64), w, h, stream=st)[0]))
    finally:
        for st in streams:
            codec.stream_destroy(st)
    for a, b in zip(runs[0], runs[1]):
        assert a.tobytes() == b.tobytes()


# ---- 4. tree qp -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(32, 32), (96, 160), (160, 96)])
def test_tree_qp_strengths_clamps_and_outputs(codec, w, h):
    _, _, cost, mode = ref("random", w, h)
    n = cost.size
    rec, _ = R.frame_cost(cost, mode, None, None, 0)
    r = np.random.RandomState(12 + w)
    prop = (r.randint(0, 1 << 30, n).astype(np.uint64) >> r.randint(0, 30, n).astype(np.uint64))
    aq = r.randint(-3072, 3073, n).astype(np.int16)
    for strength in (0, 512, 1024):
        for a in (None, aq):
            off, qp = tree_qp(codec, rec, prop, a, w, h, strength)
            if strength == 0:
                assert np.array_equal(off, aq if a is not None else np.zeros(n, np.int16))
    # the clamps from both sides: a large gain on a low offset, no gain on the highest offset, intra 0
    rec2, prop2, aq2 = rec.copy(), prop.copy(), aq.copy()
    rec2["intra"][0], prop2[0], aq2[0] = 1, 2 ** 63, -3000
    rec2["intra"][1], prop2[1], aq2[1] = 5000, 0, 3072
    rec2["intra"][2], prop2[2], aq2[2] = 0, 2 ** 40, -3072
    rec2["intra"][3], prop2[3], aq2[3] = 2 ** 32 - 1, 2 ** 64 - 1, 7
    off, _ = tree_qp(codec, rec2, prop2, aq2, w, h, 1024)
    assert off[:4].tolist() == [-3072, 3072, -3072, 7]
    for base, chroma in ((0, -12), (0, 12), (51, -12), (51, 12)):
        off, qp = tree_qp(codec, rec, prop, aq, w, h, 1024, qp=base, chroma=chroma)
        assert qp.min() >= 0 and qp.max() <= 51
    tree_qp(codec, rec, prop, aq, w, h, 512, offset=True, qps=False)
    tree_qp(codec, rec, prop, aq, w, h, 512, offset=False, qps=True)
    tree_qp(codec, rec, None, None, w, h, 512)                               # nothing received, no AQ: every offset 0, every qp the base
    # d_prop zero and the offsets of the source analysis: the bytes of its own decision
    stats = A.tile_stats(R.frame("random", w, h))
    aq_off, aq_qp = A.decide(stats, A.totals(stats), w, h, 2, 256, 30, 2)
    off, qp = tree_qp(codec, rec, np.zeros(n, np.uint64), aq_off, w, h, 1024, qp=30, chroma=2)
    assert np.array_equal(off, aq_off) and np.array_equal(qp, aq_qp)


# ---- 5. the whole chain in one graph ----------------------------------------------------------------------------------------------------------
def test_the_chain_in_one_graph(codec):
    """downscale x 2 -> intra -> lowres SATD search -> frame cost -> propagate -> tree qp, captured once and replayed on other data"""
    w, h, rng = 96, 160, 3
    n, n_ctu = 60, 6
    frames = [R.frame("smooth", w, h, 1), R.frame("smooth", w, h, 2), R.frame("random", w, h, 3)]
    pairs = [(frames[0], R.shifted(frames[0], w, h, 4, -2)), (frames[1], frames[2])]
    al = lambda nbytes: codec.alloc(max(nbytes, 16))
    d = dict(cur=al(n * 512), ref=al(n * 512), cur_low=al(n * 128), ref_low=al(n * 128), intra=al(4 * n), mode=al(n), best=al(8 * n), block=al(16 * n),
             total=al(64), prop=al(8 * n), ref0=al(8 * n), off=al(2 * n), qp=al(6 * n_ctu))
    p_cur = codec.la_params(w, h, 200, 512, 30, -1, d_src=d["cur"].ptr, d_low=d["cur_low"].ptr, d_intra=d["intra"].ptr, d_mode=d["mode"].ptr,
                            d_inter0=d["best"].ptr, d_block=d["block"].ptr, d_total=d["total"].ptr, d_prop=d["prop"].ptr, d_prop_ref0=d["ref0"].ptr,
                            d_offset=d["off"].ptr, d_qp=d["qp"].ptr)
    p_ref = codec.la_params(w, h, d_src=d["ref"].ptr, d_low=d["ref_low"].ptr)
    prop = np.random.RandomState(14).randint(0, 1 << 18, n).astype(np.uint64)
    d["prop"].upload(prop)
    st = codec.stream_create()
    try:
        assert codec.L.xHipMeScratchReserve(codec.ctx, st, w // 2, h // 2) == 0
        codec.graph_begin(st)
        codec.la_downscale_dev(p_cur, stream=st)
        codec.la_downscale_dev(p_ref, stream=st)
        codec.la_intra_costs_dev(p_cur, stream=st)
        codec.satd_search_from_tiles_dev(d["cur_low"].ptr, d["ref_low"].ptr, w // 2, h // 2, rng, d["best"].ptr, stream=st)
        codec.la_frame_cost_dev(p_cur, stream=st)
        codec.la_propagate_dev(p_cur, stream=st)
        codec.la_tree_qp_dev(p_cur, stream=st)
        graph = codec.graph_end(st)
        try:
            for i in (1, 0):                                                 # replayed twice, on other data than it was captured with
                cur, other = pairs[i]
                d["cur"].upload(cur)
                d["ref"].upload(other)
                d["ref0"].upload(np.zeros(n, np.uint64))                     # the caller zeroes an accumulator
                d["block"].upload(np.full(16 * n, 0x5A, np.uint8))
                codec.graph_launch(graph, st)
                sync_or_exit(codec, 0, st)
                cur_low, ref_low = R.downscale(cur, w, h), R.downscale(other, w, h)
                cost, mode = R.intra_costs(cur_low, w, h)
                best = R.search(cur_low, ref_low, w, h, rng)
                rec, tot = R.frame_cost(cost, mode, best, None, 200)
                ref0, _ = R.propagate(rec, prop, np.zeros(n, np.uint64), None, w, h)
                off, qp = R.tree_qp(rec, prop, None, w, h, 512, 30, -1)
                same(d["cur_low"].download(np.uint8, n * 128).reshape(-1, 512)[:, :384], cur_low[:, :384], "cur_low")
                same(d["intra"].download(np.uint32, n), cost, "intra")
                same(d["best"].download(np.uint8, 8 * n).view(R.ME_DTYPE), best, "best")
                same(d["block"].download(np.uint8, 16 * n).view(R.BLOCK_DTYPE), rec, "block")
                assert d["total"].download(np.int64, 8).tolist() == tot.tolist()
                same(d["ref0"].download(np.uint64, n), ref0, "ref0")
                same(d["off"].download(np.int16, n), off, "off")
                same(d["qp"].download(np.uint8, 6 * n_ctu), qp, "qp")
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------------
def test_the_tree_qp_map_feeds_the_fused_coding_call(codec):
    """xLaTreeQpGpu's d_qp goes into xDct32CodeCtuTilesGpu without leaving the device; the levels are those of the restatement's bytes"""
    from test_gpu_quant import _tiles_mix
    w, h = 64, 64
    n, n_ctu = 16, 1
    cur = R.frame("smooth", w, h, 4)
    pred, base = _tiles_mix(w, h, 0x7B00), _tiles_mix(w, h, 0x7B01)
    low = R.downscale(cur, w, h)
    cost, mode = R.intra_costs(low, w, h)
    prop = (np.arange(n, dtype=np.uint64) % np.uint64(4)) * np.uint64(400000)        # the right columns were referred to a lot
    dc, dp, dr = dev(codec, cur.ravel()), dev(codec, pred), dev(codec, base)
    al = lambda nbytes: codec.alloc(max(nbytes, 16))
    d_low, d_intra, d_block, d_total, d_prop, d_qp = al(n * 128), al(4 * n), al(16 * n), al(64), codec._upload(prop), al(6)
    dl, dn = al(n_ctu * 12288), al(n_ctu * 24)
    p = codec.la_params(w, h, 0, 1024, 30, 2, d_src=dc.ptr, d_low=d_low.ptr, d_intra=d_intra.ptr, d_block=d_block.ptr, d_total=d_total.ptr, d_prop=d_prop.ptr,
                        d_qp=d_qp.ptr)
    codec.la_downscale_dev(p)
    codec.la_intra_costs_dev(p)
    codec.la_frame_cost_dev(p)
    codec.la_tree_qp_dev(p)
    codec.dct32_code_ctu_tiles_dev(dc.ptr, dp.ptr, w, h, d_qp.ptr, 0, 171, dl.ptr, dn.ptr, dr.ptr)
    sync_or_exit(codec, 0)
    rec, _ = R.frame_cost(cost, None, None, None, 0)
    want_qp = R.tree_qp(rec, prop, None, w, h, 1024, 30, 2)[1]
    assert len(set(want_qp.tolist())) > 2 and want_qp.min() < 30                 # a map, and the tree lowered it
    assert np.array_equal(d_qp.download(np.uint8, 6), want_qp)
    level, nnz, recon = codec.code_ctu_tiles(cur, pred, w, h, qps=want_qp, rounding=171, base=base)
    assert np.array_equal(dl.download(np.int16, n_ctu * 6144).reshape(n_ctu, 6, 1024), level) and level.any()
    assert np.array_equal(dn.download(np.uint32, 6 * n_ctu).reshape(n_ctu, 6), nnz)
    assert np.array_equal(dr.download(np.uint8, w * h * 2), recon)


def _p_totals(codec, cur, prev, w, h, penalty, rng=3):
    """the totals of a P decision of `cur` against `prev`, on the device"""
    low = [codec.la_downscale(t, w, h) for t in (cur, prev)]
    cost, mode = codec.la_intra_costs(low[0], w, h)
    best = codec.search_tiles(low[0], low[1], w // 2, h // 2, rng)
    me = np.zeros(cost.size, R.ME_DTYPE)
    me["mvx"], me["mvy"], me["cost"] = best[0][:, 0], best[0][:, 1], best[1]
    return codec.la_frame_cost(cost, mode, me, None, w, h, penalty)


def _ref_totals(cur, prev, w, h, penalty, rng=3):
    low = [R.downscale(t, w, h) for t in (cur, prev)]
    cost, mode = R.intra_costs(low[0], w, h)
    return R.frame_cost(cost, mode, R.search(low[0], low[1], w, h, rng), None, penalty)


def _margin(tot, threshold_q8, g, lo, hi):
    """p * 65536 over (65536 - bias) * i: 1 is the threshold"""
    return int(tot[0]) * 65536 / ((65536 - R.scene_cut_bias(threshold_q8, g, lo, hi)) * int(tot[1]))


def test_scene_cut_end_to_end(codec):
    """a frame against a moved copy of itself is no cut; against an unrelated frame it is one.  The seeds are chosen so that the restatement's
    decision lies more than 5 % from the threshold: a property of the inputs, not a coincidence"""
    w, h = 96, 160
    smooth, noise = R.frame("smooth", w, h, 1), R.frame("random", w, h, 2)
    cases = [(smooth, R.shifted(smooth, w, h, 4, -2), 0, 0), (noise, R.frame("random", w, h, 3), 100, 1)]
    for cur, prev, penalty, want in cases:
        rec, tot = _ref_totals(cur, prev, w, h, penalty)
        m = _margin(tot, 102, 100, 25, 250)
        print("scene cut: p %d, i %d, list-0 blocks %d of %d, p / threshold %.3f" % (tot[0], tot[1], tot[3], tot[7], m))
        assert (m < 0.95, m > 1.05)[want] and R.scene_cut(tot, 102, 100, 25, 250) == want
        if want:
            assert tot[3] > 0 and tot[2] > 0                                 # the penalty leaves list-0 blocks winning somewhere
        got_rec, got_tot = _p_totals(codec, cur, prev, w, h, penalty)
        same(got_rec, rec, "d_block")
        assert got_tot.tolist() == tot.tolist()
        assert x266_amd.scene_cut_from_totals(got_tot, 102, 100, 25, 250) == bool(want)


def test_numpy_conveniences(codec):
    w, h = 96, 160
    tiles, low, cost, mode = ref("random", w, h)
    got = codec.la_downscale(tiles, w, h)
    assert np.array_equal(got[:, :384], low[:, :384]) and not got[:, 384:].any()
    c, m = codec.la_intra_costs(low, w, h)
    assert np.array_equal(c, cost) and np.array_equal(m, mode)
    l0, l1 = lists(cost, 3)
    rec, tot = codec.la_frame_cost(cost, mode, l0, l1, w, h, 300)
    want, want_tot = R.frame_cost(cost, mode, l0, l1, 300)
    assert np.array_equal(rec, want) and tot.tolist() == want_tot.tolist() and rec.dtype == x266_amd.LA_BLOCK_DTYPE
    prop = np.arange(rec.size, dtype=np.uint64) * np.uint64(999)
    zeros = np.zeros(rec.size, np.uint64)
    r0, r1 = codec.la_propagate(rec, prop, zeros, None, w, h)
    w0, _ = R.propagate(want, prop, zeros, None, w, h)
    assert r1 is None and np.array_equal(r0, w0)
    off, qp = codec.la_tree_qp(rec, prop, None, w, h, strength_q8=700, qp=27, chroma_qp_offset=3)
    want_off, want_qp = R.tree_qp(want, prop, None, w, h, 700, 27, 3)
    assert np.array_equal(off, want_off) and np.array_equal(qp.ravel(), want_qp)


# ---- 7. refusals through the ABI --------------------------------------------------------------------------------------------------------------
def test_argument_errors(codec):
    """every rule once per call: X266HIP_EINVAL, the call named in the error text, nothing launched, the buffers untouched"""
    L, ctx = codec.L, codec.ctx
    M = 1 << 18
    names = list(PTRS)
    buf = codec.alloc((len(names) + 1) * M)
    fill = np.random.RandomState(9).randint(1, 255, (len(names) + 1) * M).astype(np.uint8)
    buf.upload(fill)
    w, h, n, n_ctu = 160, 96, 60, 6
    good = {name: buf.ptr + (i + 1) * M for i, name in enumerate(names)}
    good.update(width=w, height=h, intra_penalty=300, strength_q8=256, qp=30, chroma_qp_offset=0)
    extent = dict(d_src=n * 512, d_low=n * 128, d_intra=4 * n, d_mode=n, d_inter0=8 * n, d_inter1=8 * n, d_block=16 * n, d_total=64, d_prop=8 * n,
                  d_prop_ref0=8 * n, d_prop_ref1=8 * n, d_aq_offset=2 * n, d_offset=2 * n, d_qp=6 * n_ctu)
    # per call: (required, optional, outputs)
    calls = {"xLaDownscaleGpu": (["d_src", "d_low"], [], ["d_low"]),
             "xLaIntraCostsGpu": (["d_low", "d_intra"], ["d_mode"], ["d_intra", "d_mode"]),
             "xLaFrameCostGpu": (["d_intra", "d_block", "d_total"], ["d_mode", "d_inter0", "d_inter1"], ["d_block", "d_total"]),
             "xLaPropagateGpu": (["d_block"], ["d_prop", "d_prop_ref0", "d_prop_ref1"], ["d_prop_ref0", "d_prop_ref1"]),
             "xLaTreeQpGpu": (["d_block"], ["d_prop", "d_aq_offset", "d_offset", "d_qp"], ["d_offset", "d_qp"])}

    def refused(name, **change):
        p = codec.la_params(**dict(good, **change))
        assert getattr(L, name)(ctx, ctypes.byref(p), None) == EINVAL, (name, change)
        assert name.encode() in L.xHipLastError(ctx), (name, change)

    for name, (required, optional, outputs) in calls.items():
        assert getattr(L, name)(ctx, None, None) == EINVAL and name.encode() in L.xHipLastError(ctx)    # NULL p
        assert getattr(L, name)(None, ctypes.byref(codec.la_params(**good)), None) == EINVAL
        for field in required:
            refused(name, **{field: 0})
        for field in required + optional:
            if PTRS[field] > 1:
                refused(name, **{field: good[field] + PTRS[field] // 2})
            refused(name, **{field: 2 ** 64 - PTRS[field]})                  # aligned, and the extent does not fit behind it
        for side in ("width", "height"):
            for v in (0, -32, 16, 48, 176 if side == "width" else 112):
                refused(name, **{side: v})
        for field in outputs:                                                # an output, or an accumulator, over any other buffer of the call
            for other in required + optional:
                if other != field:
                    refused(name, **{field: good[other] + (extent[other] - 1) // PTRS[field] * PTRS[field]})   # onto the other's last bytes
                    refused(name, **{field: good[other]})
    refused("xLaFrameCostGpu", intra_penalty=-1)
    refused("xLaFrameCostGpu", intra_penalty=65536)
    refused("xLaTreeQpGpu", d_offset=0, d_qp=0)
    for change in (dict(strength_q8=-1), dict(strength_q8=1025), dict(qp=-1), dict(qp=52), dict(chroma_qp_offset=-13), dict(chroma_qp_offset=13)):
        refused("xLaTreeQpGpu", **change)
    sync_or_exit(codec, 0)
    assert np.array_equal(buf.download(np.uint8, fill.size), fill)          # nothing was launched
    # the edges of what is accepted: every optional field NULL, every scalar at either end of its range, the fields a call does not read garbage
    junk = dict(d_src=3, d_inter0=5, d_aq_offset=1, intra_penalty=-7, strength_q8=-7, qp=99, chroma_qp_offset=99)
    tiles, low, cost, mode = ref("random", w, h)
    image = fill.copy()
    image[M:M + n * 512] = tiles.ravel()
    buf.upload(image)
    call_struct(codec, "xLaDownscaleGpu", codec.la_params(**dict(good, **{k: v for k, v in junk.items() if k != "d_src"})))
    call_struct(codec, "xLaIntraCostsGpu", codec.la_params(**dict(good, d_mode=0, **{k: v for k, v in junk.items() if k != "d_mode"})))
    for penalty in (0, 65535):
        call_struct(codec, "xLaFrameCostGpu", codec.la_params(**dict(good, d_mode=0, d_inter0=0, d_inter1=0, d_src=3, intra_penalty=penalty, strength_q8=-7, qp=99)))
    call_struct(codec, "xLaPropagateGpu", codec.la_params(**dict(good, d_prop=0, d_prop_ref1=0, **junk)))
    call_struct(codec, "xLaTreeQpGpu", codec.la_params(**dict(good, d_prop=0, d_aq_offset=0, d_offset=0, d_src=3, strength_q8=0, qp=0, chroma_qp_offset=-12)))
    call_struct(codec, "xLaTreeQpGpu", codec.la_params(**dict(good, d_prop=0, d_aq_offset=0, d_qp=0, d_src=3, strength_q8=1024, qp=51, chroma_qp_offset=12)))
    now = buf.download(np.uint8, fill.size)
    at = lambda name, dtype=np.uint8: now[(names.index(name) + 1) * M:(names.index(name) + 1) * M + extent[name]].view(dtype)
    same(at("d_low").reshape(-1, 512)[:, :384], low[:, :384], "d_low")
    same(at("d_intra", np.uint32), cost, "d_intra")
    rec, tot = R.frame_cost(cost, None, None, None, 65535)
    same(at("d_block", R.BLOCK_DTYPE), rec, "d_block")
    assert at("d_total", np.int64).tolist() == tot.tolist()
    assert np.array_equal(at("d_prop_ref0"), image[(names.index("d_prop_ref0") + 1) * M:][:8 * n])     # every block is intra: nothing is handed on
    assert not at("d_offset", np.int16).any() and (at("d_qp")[:4 * n_ctu] == 0).all()
    for name in ("d_low", "d_intra", "d_block", "d_total", "d_offset", "d_qp"):
        lo = (names.index(name) + 1) * M
        keep = ~np.tile(M_I, n // 4) if name == "d_low" else np.ones(extent[name], bool)
        now[lo:lo + extent[name]][keep] = image[lo:lo + extent[name]][keep]
    assert np.array_equal(now, image)                                        # ... and nothing else was written
