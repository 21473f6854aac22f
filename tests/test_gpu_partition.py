"""GPU (-m gpu): the inter partition decision (xInterPartitionDecideGpu) against tests/_partition_ref.py, bit-exact in every output byte:
d_out, d_level, d_ctu and d_nodes.  Every buffer of every call sits between the guard bands of tests/_arena.py at exactly its documented
alignment; the guards and the inputs are checked after every call, and the stream is synchronised (or the session ended) after every call.

The shapes, each for what can go wrong there: 16 x 16 one tile, only levels 0 and 1 whole; 64 x 64 one whole CTU; 80 x 48 a cut CTU column,
no whole level-3 node, level 2 whole only in the top row; 144 x 112 whole and cut CTUs and a top-right neighbour in another CTU; 1104 x 16
69 tiles in a row, every CTU cut."""
import ctypes
import functools

import numpy as np
import pytest

import _option_cases as O
import _partition_ref as R
import _seeded_ref as S
import x266_amd.partition as P
from _arena import Arena
from _dev import EINVAL, call_struct, dev, records, same, sync_or_exit
from _util import Oracle

pytestmark = pytest.mark.gpu

CALL = "xInterPartitionDecideGpu"
PTRS = {"d_cur": 16, "d_ref": 16, "d_mv": 8, "d_out": 8, "d_level": 1, "d_ctu": 8, "d_nodes": 8}
DISP = {name: align * (2 * i + 1) for i, (name, align) in enumerate(PTRS.items())}          # exactly the documented alignment, no more
OUTPUTS = ("d_out", "d_level", "d_ctu", "d_nodes")
MIX_SIZES = [(16, 16), (64, 64), (80, 48)]


@functools.lru_cache(None)
def _oracle():
    return Oracle()


@functools.lru_cache(None)
def content(kind, w, h):
    """(cur plane, ref plane, cur tiles, ref tiles, field [nb, 2] int16), computed once and shared"""
    cur, ref = (R.motion_frames if kind == "motion" else R.mix_frames)(w, h, 0)
    mv = (R.motion_field if kind == "motion" else R.mix_field)(w, h, 0)
    out = (cur, ref, S.tiles_of(_oracle(), cur, 1).ravel(), S.tiles_of(_oracle(), ref, 2).ravel(), mv)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(None)
def want(kind, w, h, lam, r):
    """the reference's decision of a case, computed once, shared and left unchanged"""
    cur, ref, _, _, mv = content(kind, w, h)
    d = R.decide(_oracle(), cur, ref, mv, r, lam)
    for k in ("out", "level", "ctu", "nodes"):
        d[k].setflags(write=False)
    return d


def sizes(w, h):
    nb, n_ctu = (w // 8) * (h // 8), ((w + 63) // 64) * ((h + 63) // 64)
    return dict(d_out=8 * nb, d_level=nb, d_ctu=16 * n_ctu, d_nodes=8 * R.nodes_total(w // 8, h // 8))


def junk_records(mv, seed=7):
    """x266_me_result_t records of a field; cost is ignored by the call, so it is garbage"""
    return records(mv, np.random.RandomState(seed).randint(0, 1 << 32, len(mv), dtype=np.uint64).astype(np.uint32))


def decide(codec, cur_t, ref_t, w, h, mv, lam, r, with_nodes=True, stream=None, guard_seed=51, same_frame=False):
    """the call inside an arena -> {output: its bytes}"""
    a = Arena(codec)
    cur = a.input("d_cur", cur_t, 16, DISP["d_cur"], guard_seed)
    ref = cur if same_frame else a.input("d_ref", ref_t, 16, DISP["d_ref"], guard_seed + 1)
    field = a.input("d_mv", junk_records(mv, guard_seed).view(np.uint8), 8, DISP["d_mv"], guard_seed + 2)
    n = sizes(w, h)
    outs = {f: a.output(f, n[f], PTRS[f], DISP[f]) for f in OUTPUTS if f != "d_nodes" or with_nodes}
    p = P.part_params(d_cur=cur.ptr, d_ref=ref.ptr, d_mv=field.ptr, width=w, height=h, range=r, lambda_q4=lam, **{f: s.ptr for f, s in outs.items()})
    call_struct(codec, CALL, p, stream)
    got = a.check()                                                         # guard bands, and every input unchanged
    return {f: got[f] for f in outs}


def compare(got, d, what):
    same(got["d_out"].view(R.ME_DTYPE), d["out"], ("d_out",) + what)
    same(got["d_level"], d["level"], ("d_level",) + what)
    same(got["d_ctu"].view(R.CTU_DTYPE), d["ctu"], ("d_ctu",) + what)
    if "d_nodes" in got:
        same(got["d_nodes"].view(R.ME_DTYPE), d["nodes"], ("d_nodes",) + what)


def check_case(codec, kind, w, h, lam, r, **kw):
    _, _, cur_t, ref_t, mv = content(kind, w, h)
    d = want(kind, w, h, lam, r)
    got = decide(codec, cur_t, ref_t, w, h, mv, lam, r, **kw)
    compare(got, d, (kind, w, h, lam, r))
    return got, d


# ---- 1. the shapes x the settings, both contents ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,r", R.SETTINGS)
@pytest.mark.parametrize("w,h", R.SIZES)
def test_motion_content(codec, w, h, lam, r):
    if (w, h, lam, r) == (144, 112, 4096, 1):                                # the condition, on the reference, before the device is asked
        d = want("motion", w, h, lam, r)
        assert (np.bincount(d["level"], minlength=4) > 0).all(), np.bincount(d["level"], minlength=4)
        assert d["cut_split"] and any(not m for m in d["merged"].values())
    check_case(codec, "motion", w, h, lam, r)


@pytest.mark.parametrize("lam,r", R.SETTINGS)
@pytest.mark.parametrize("w,h", MIX_SIZES)
def test_vector_mix(codec, w, h, lam, r):
    """the clamp of the input, candidates at the ends of int16, vectors wholly outside the frame"""
    mv = content("mix", w, h)[4].astype(np.int64)
    if (w, h) != (16, 16):
        assert (np.abs(mv) > R.CLAMP).any() and (np.abs(mv) > 4 * max(w, h)).any()
    check_case(codec, "mix", w, h, lam, r)


def test_vector_mix_across_ctus(codec):
    check_case(codec, "mix", 144, 112, 64, 1)
    check_case(codec, "mix", 144, 112, 64, 1, guard_seed=97)                # whatever lies around the buffers must not reach the result


def test_one_frame_as_both_and_without_d_nodes(codec):
    """d_cur == d_ref is allowed; with d_nodes NULL the other outputs hold the same bytes"""
    w, h, lam, r = 80, 48, 64, 1
    cur, _, cur_t, ref_t, mv = content("motion", w, h)
    d = R.decide(_oracle(), cur, cur, mv, r, lam)
    compare(decide(codec, cur_t, None, w, h, mv, lam, r, same_frame=True), d, ("one frame",))
    with_nodes, _ = check_case(codec, "motion", w, h, lam, r)
    without, _ = check_case(codec, "motion", w, h, lam, r, with_nodes=False)
    assert "d_nodes" not in without
    for f in without:
        assert without[f].tobytes() == with_nodes[f].tobytes(), f


# ---- 2. what follows from the contract, against the calls that are already there -----------------------------------------------------------------
def through_mc_and_satd(codec, ref_t, cur_t, w, h, out_records):
    """the costs of a field through xMotionCompQpelLumaGpu and xSatd8x8FromTilesDev"""
    nb = (w // 8) * (h // 8)
    d_ref, d_cur, d_mv = dev(codec, ref_t), dev(codec, cur_t), dev(codec, out_records.view(np.uint8))
    d_pred, d_cost = dev(codec, np.zeros(w * h * 2, np.uint8)), codec.alloc(max(4 * nb, 16))
    codec.motion_comp_qpel_luma_dev(d_ref.ptr, d_mv.ptr, w, h, d_pred.ptr)
    codec.satd8x8_from_tiles_dev(d_cur.ptr, d_pred.ptr, w, h, d_cost.ptr)
    sync_or_exit(codec, 0)
    return d_cost.download(np.uint32, nb)


@pytest.mark.parametrize("kind,w,h,lam,r", [("motion", 144, 112, 4096, 1), ("motion", 80, 48, 0, 0), ("mix", 80, 48, 64, 1), ("motion", 1104, 16, 64, 1)])
def test_the_output_field_reproduces_its_own_costs(codec, kind, w, h, lam, r):
    """consequence 4"""
    _, _, cur_t, ref_t, _ = content(kind, w, h)
    got, _ = check_case(codec, kind, w, h, lam, r)
    out = got["d_out"].view(R.ME_DTYPE)
    same(through_mc_and_satd(codec, ref_t, cur_t, w, h, out), out["cost"], ("costs", kind, w, h, lam, r))


@pytest.mark.parametrize("lam", [0, 8, 64, 65535])
def test_a_constant_field_merges_into_the_largest_whole_nodes(codec, lam):
    """consequence 2, range 0"""
    w, h, q = 144, 112, (5, -3)
    cur, ref, cur_t, ref_t, _ = content("motion", w, h)
    bw, bh = w // 8, h // 8
    mv = np.tile(np.array([q], np.int16), (bw * bh, 1))
    got = decide(codec, cur_t, ref_t, w, h, mv, lam, 0)
    compare(got, R.decide(_oracle(), cur, ref, mv, 0, lam), ("constant", lam))
    out = got["d_out"].view(R.ME_DTYPE)
    assert (out["mvx"] == q[0]).all() and (out["mvy"] == q[1]).all()
    largest = [max(k for k in range(4) if R.whole(bw, bh, k, (b % bw) >> k, (b // bw) >> k)) for b in range(bw * bh)]
    assert got["d_level"].tolist() == largest
    same(through_mc_and_satd(codec, ref_t, cur_t, w, h, junk_records(mv).view(R.ME_DTYPE)), out["cost"], ("D(b, q)", lam))


# ---- 3. a graph, the launch options ----------------------------------------------------------------------------------------------------------
def plain_buffers(codec, w, h, kind="motion"):
    _, _, cur_t, ref_t, mv = content(kind, w, h)
    n = sizes(w, h)
    bufs = dict(d_cur=dev(codec, cur_t), d_ref=dev(codec, ref_t), d_mv=dev(codec, junk_records(mv).view(np.uint8)), **{f: codec.alloc(max(n[f], 16)) for f in OUTPUTS})
    fill = lambda: [bufs[f].upload(np.full(n[f], 0x5A, np.uint8)) for f in OUTPUTS]
    grab = lambda: {f: bufs[f].download(np.uint8, n[f]) for f in OUTPUTS}
    return bufs, fill, grab


def test_in_a_graph(codec):
    """captured once, replayed twice: the same bytes as the plain call, which are the reference's"""
    w, h, lam, r = 144, 112, 4096, 1
    bufs, fill, grab = plain_buffers(codec, w, h)
    p = P.part_params(width=w, height=h, range=r, lambda_q4=lam, **{f: b.ptr for f, b in bufs.items()})
    fill()
    codec.inter_partition_decide_dev(p)
    sync_or_exit(codec, 0)
    plain = grab()
    compare(plain, want("motion", w, h, lam, r), ("plain",))
    st = codec.stream_create()
    try:
        codec.graph_begin(st)                                                # no xHipMeScratchReserve: the call uses no scratch
        codec.inter_partition_decide_dev(p, stream=st)
        graph = codec.graph_end(st)
        try:
            for _ in range(2):
                fill()
                codec.graph_launch(graph, st)
                sync_or_exit(codec, 0, st)
                now = grab()
                for f in OUTPUTS:
                    assert now[f].tobytes() == plain[f].tobytes(), f
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


def test_every_launch_option_set_gives_the_same_bytes(codec):
    w, h, lam, r = 144, 112, 4096, 1
    d = want("motion", w, h, lam, r)
    before = {k: codec.get_option(k) for k in O.VALUES}
    setting = {k: max(v for v in O.VALUES[k] if v != O.DEFAULTS[k]) for k in O.VALUES}
    setting[O.ADAPTIVE] = 0                                                 # the per-wave values in force, not clamped
    try:
        for k, v in setting.items():
            codec.set_option(k, v)
        assert all(codec.get_option(k) == v != O.DEFAULTS[k] for k, v in setting.items())
        got, _ = check_case(codec, "motion", w, h, lam, r)
    finally:
        for k, v in before.items():
            codec.set_option(k, v)
    plain, _ = check_case(codec, "motion", w, h, lam, r)
    for f in OUTPUTS:
        assert got[f].tobytes() == plain[f].tobytes(), f
    assert d["ctu"]["parts"].sum() > 0


def test_numpy_convenience(codec):
    w, h, lam, r = 80, 48, 64, 1
    _, _, cur_t, ref_t, mv = content("motion", w, h)
    d = want("motion", w, h, lam, r)
    out_mv, satd, level, ctu, nodes = P.partition_decide(codec, cur_t, ref_t, w, h, mv, r, lam, want_nodes=True)
    assert np.array_equal(out_mv[:, 0], d["out"]["mvx"]) and np.array_equal(out_mv[:, 1], d["out"]["mvy"]) and np.array_equal(satd, d["out"]["cost"])
    assert np.array_equal(level, d["level"]) and np.array_equal(ctu, d["ctu"].astype(ctu.dtype))
    assert np.array_equal(nodes[0][:, 0], d["nodes"]["mvx"]) and np.array_equal(nodes[0][:, 1], d["nodes"]["mvy"]) and np.array_equal(nodes[1], d["nodes"]["cost"])
    assert P.partition_decide(codec, cur_t, ref_t, w, h, mv, r, lam)[4] is None


# ---- 4. refusals through the ABI --------------------------------------------------------------------------------------------------------------
def test_argument_errors(codec):
    """every rule of the header: X266HIP_EINVAL, the call named in the error text, nothing launched, the arena untouched"""
    L, ctx = codec.L, codec.ctx
    fn = getattr(L, CALL)
    w, h = 144, 112
    _, _, cur_t, ref_t, mv = content("motion", w, h)
    n = sizes(w, h)
    a = Arena(codec)
    slots = {"d_cur": a.input("d_cur", cur_t, 16, DISP["d_cur"], 61), "d_ref": a.input("d_ref", ref_t, 16, DISP["d_ref"], 62),
             "d_mv": a.input("d_mv", junk_records(mv).view(np.uint8), 8, DISP["d_mv"], 63)}
    slots.update({f: a.output(f, n[f], PTRS[f], DISP[f]) for f in OUTPUTS})
    good = dict({f: s.ptr for f, s in slots.items()}, width=w, height=h, range=1, lambda_q4=64)
    extent = dict(n, d_cur=w * h * 2, d_ref=w * h * 2, d_mv=n["d_out"])

    def refused(**change):
        p = P.part_params(**dict(good, **change))
        assert fn(ctx, ctypes.byref(p), None) == EINVAL, change
        assert CALL.encode() in L.xHipLastError(ctx), change

    assert fn(ctx, None, None) == EINVAL and CALL.encode() in L.xHipLastError(ctx)                # NULL p
    assert fn(None, ctypes.byref(P.part_params(**good)), None) == EINVAL
    for field in PTRS:
        if field != "d_nodes":
            refused(**{field: 0})
        if PTRS[field] > 1:
            refused(**{field: good[field] + PTRS[field] // 2})
        refused(**{field: 2 ** 64 - PTRS[field]})                            # aligned, and the extent does not fit behind it
    for side in ("width", "height"):
        for v in (0, -16, 8, 24, 152 if side == "width" else 120):
            refused(**{side: v})
    for change in (dict(range=-1), dict(range=2), dict(lambda_q4=-1), dict(lambda_q4=65536)):
        refused(**change)
    for field in OUTPUTS:                                                    # an output over any other buffer of the call, the input field included
        for other in PTRS:
            if other != field:
                refused(**{field: good[other] + (extent[other] - 1) // PTRS[field] * PTRS[field]})   # onto the other's last bytes
                if good[other] % PTRS[field] == 0:
                    refused(**{field: good[other]})
    sync_or_exit(codec, 0)
    a.check_untouched()                                                     # nothing was launched
    # the edges of what is accepted: d_nodes NULL, one frame as both, the scalars at either end of their ranges
    for lam, r, one in ((0, 0, False), (65535, 1, False), (64, 1, True)):
        p = P.part_params(**dict(good, range=r, lambda_q4=lam, d_nodes=0, d_ref=good["d_cur"] if one else good["d_ref"]))
        call_struct(codec, CALL, p)
    slots["d_nodes"].check_untouched()


# ---- 5. the plain-C host ----------------------------------------------------------------------------------------------------------------------------
def test_plain_c_host_example():
    """host/partition_example.c: a C host without HIP headers searches, refines, merges and predicts a frame of two motions; the records add
    up as the header says, and large partitions appear where the motion is uniform"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "partition_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "host"), "--no-print-directory", exe])
    out = subprocess.run([exe, "208", "144"], timeout=120, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["as_expected"] is True and d["blocks"] == 26 * 18 and d["ctus"] == 12
    assert sum(p * 4 ** k for k, p in enumerate(d["partitions"])) == d["blocks"] and sum(d["partitions"]) == d["parts"] < d["blocks"]
    assert d["dist"] == d["satd_merged"] <= d["j"] and d["partitions"][3] >= 1 and d["predicted_exactly"] == d["zero_satd_blocks"]
