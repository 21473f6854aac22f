"""Bi-directional inter prediction on tiled frames: motion compensation from two references (xMotionCompBiQpelTiles), the three
costs and the direction of a block (xSatd8x8BiCostsFromTiles) and the refinement of one list against the other
(xSatd8x8RefineBiQpelFromTiles).  The reference statement is tests/_bipred_ref.py (the header's arithmetic in numpy int64, checked
by tests/test_bipred_ref.py, which also asserts what the recipes used here cover); every comparison is bit-exact.

Sizes: 16x16 one tile, every tap clamps; 32x32 all 16 luma phases (and the crafted extremes of V); 64x64 all 64 chroma phases;
48x32 an odd tile count; 144x80 mv_mix_q vectors -- int16 extremes, vectors wholly outside the frame -- differing per list."""
import ctypes

import numpy as np
import pytest

import _bipred_ref as B
import _subpel_ref as R
from _dev import EINVAL, arena_slots, dev, displacements, records, sentinels, sync_or_exit, tiles
from _util import me_frames
from test_gpu_mc_chroma import _mv_mix
from test_gpu_subpel import _unpack

gpu = pytest.mark.gpu
SLICES = {1: [slice(0, 256)], 2: [slice(256, 384)], 3: [slice(0, 384)]}


def _wp(codec, wp):
    return None if wp is None else codec.wp_params(wp.w.tolist(), wp.o.tolist(), wp.log2_denom)


def _only(full, base, planes):
    """the tile array of a call that writes `planes`, from the reference of the whole prediction"""
    out = np.array(base, np.uint8).reshape(-1, 512)
    for s in SLICES[planes]:
        out[:, s] = full.reshape(-1, 512)[:, s]
    return out.ravel()


# ---- 1. motion compensation ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", B.SIZES)
def test_mc_against_the_statement(codec, oracle, w, h):
    """planes 1, 2 and 3 on random and on {0, 255} planes, with d_dir NULL and mixed, default weights and every weighted case: the
    planes a call owns equal the statement, blocks of direction 0, m_I and the unselected plane are the random pre-fill"""
    mv0, mv1 = B.vectors(w, h, w * h)
    direction = B.directions(len(mv0), w + h)
    base = sentinels(w, h)
    for n, kind in enumerate(B.KINDS):
        p0, p1 = B.case_planes(kind, w, h)
        t0, t1 = tiles(oracle, p0, 40 + h), tiles(oracle, p1, 41 + h)
        for d in (None, direction):
            for name, wp in [("default", None)] + list(B.WEIGHTS.items()):
                if wp is not None and (d is None) != (n == 0):              # weighted: d_dir NULL on one content kind, mixed on the other
                    continue
                full = B.bi_tiles(oracle, t0, t1, mv0, mv1, d, wp, w, h, base)
                for planes in (1, 2, 3):
                    got = codec.motion_comp_bi_qpel(t0, t1, mv0, mv1, w, h, d, _wp(codec, wp), planes, base)
                    assert np.array_equal(got, _only(full, base, planes)), (kind, d is None, name, planes)


@gpu
def test_direction_zero_leaves_the_prediction_untouched(codec, oracle):
    w, h = 48, 32
    mv0, mv1 = B.vectors(w, h, 70)
    p0, p1 = B.case_planes("random", w, h)
    t0, t1 = tiles(oracle, p0, 71), tiles(oracle, p1, 72)
    base = sentinels(w, h, 73)
    zero = np.full(len(mv0), 0xFC, np.uint8)                                # & 3 == 0
    for planes in (1, 2, 3):
        assert np.array_equal(codec.motion_comp_bi_qpel(t0, t1, mv0, mv1, w, h, zero, None, planes, base), base)


@gpu
def test_one_frame_as_both_references(codec, oracle):
    """d_ref0 == d_ref1: with equal vectors the bi prediction is the uni prediction, with different ones the statement's"""
    w, h = 48, 32
    mv0, mv1 = B.vectors(w, h, 80)
    t0 = tiles(oracle, B.case_planes("extreme", w, h)[0], 81)
    base = sentinels(w, h, 82)
    assert np.array_equal(codec.motion_comp_bi_qpel(t0, None, mv0, mv1, w, h, base=base), B.bi_tiles(oracle, t0, t0, mv0, mv1, None, None, w, h, base))
    assert np.array_equal(codec.motion_comp_bi_qpel(t0, None, mv0, mv0, w, h, base=base), codec.motion_comp_qpel(t0, mv0, w, h, base=base))


@gpu
def test_directions_1_and_2_are_the_uni_call_on_the_device(codec, oracle):
    w, h = 144, 80
    mv0, mv1 = B.vectors(w, h, w * h)
    p0, p1 = B.case_planes("extreme", w, h)
    t0, t1 = tiles(oracle, p0, 90), tiles(oracle, p1, 91)
    base = sentinels(w, h, 92)
    nb = len(mv0)
    assert np.array_equal(codec.motion_comp_bi_qpel(t0, t1, mv0, mv1, w, h, np.full(nb, 1, np.uint8), base=base), codec.motion_comp_qpel(t0, mv0, w, h, base=base))
    assert np.array_equal(codec.motion_comp_bi_qpel(t0, t1, mv0, mv1, w, h, np.full(nb, 2, np.uint8), base=base), codec.motion_comp_qpel(t1, mv1, w, h, base=base))


@gpu
def test_crafted_extremes_of_v(codec, oracle):
    """V = 33150 and -16830 (tests/test_bipred_ref.py) through every pairing of the two planes, default and at the weights' extremes"""
    hi, lo = B.crafted_extremes()
    u = R.plane("random", 16, 16, 95)
    mv = np.tile(np.int16([[2, 2]]), (16, 1))
    base = sentinels(32, 32, 96)
    big = B.WP([[127, 1, 1], [127, 1, 1]], [[127, 0, 0], [127, 0, 0]], (0, 0))
    small = B.WP([[-128, 1, 1], [-128, 1, 1]], [[-128, 0, 0], [-128, 0, 0]], (7, 0))
    for a, b in ((hi, hi), (lo, lo), (hi, lo)):
        ta, tb = tiles(oracle, (a, u, u), 97), tiles(oracle, (b, u, u), 98)
        for wp in (None, big, small):
            for d in (1, 2, 3):
                direction = np.full(16, d, np.uint8)
                got = codec.motion_comp_bi_qpel(ta, tb, mv, mv, 32, 32, direction, _wp(codec, wp), 1, base)
                assert np.array_equal(got, _only(B.bi_tiles(oracle, ta, tb, mv, mv, direction, wp, 32, 32, base), base, 1)), (d, wp is big, wp is small)


# ---- 2. the three costs and the direction ------------------------------------------------------------------------------------------------
def _chroma_for(w, h, seed):
    return R.plane("random", w // 2, h // 2, seed), R.plane("random", w // 2, h // 2, seed + 1)


@gpu
@pytest.mark.parametrize("penalty", [0, 40, 65535])
def test_costs_and_direction_of_the_decision_recipe(codec, oracle, penalty):
    """cur is per block list 0's prediction, list 1's or the bi prediction: every direction wins somewhere without a penalty, a
    large penalty prices direction 3 out"""
    w, h = 144, 80
    cur, ref0, ref1, mv0, mv1 = B.decision_case(oracle, w, h, 900)
    ct, t0, t1 = (tiles(oracle, (p, *_chroma_for(w, h, 100 + i)), 110 + i) for i, p in enumerate((cur, ref0, ref1)))
    want_costs, want_dir = B.costs3(oracle, cur, ref0, ref1, mv0, mv1, None, penalty)
    costs, direction = codec.satd8x8_bi_costs(ct, t0, t1, w, h, mv0, mv1, None, penalty)
    assert np.array_equal(costs, want_costs) and np.array_equal(direction, want_dir)
    if penalty == 0:
        assert set(direction.tolist()) == {1, 2, 3}
    if penalty == 65535:
        assert direction.max() == 2


@gpu
@pytest.mark.parametrize("w,h", [(16, 16), (32, 32), (48, 32), (144, 80)])
def test_costs_against_the_statement(codec, oracle, w, h):
    """the vectors and contents of the motion compensation cases, default and weighted; either output alone gives the same bytes"""
    mv0, mv1 = B.vectors(w, h, w * h)
    nb = len(mv0)
    for n, kind in enumerate(B.KINDS):
        p0, p1 = B.case_planes(kind, w, h)
        cur = me_frames(w, h, 0, 120 + n)[0]
        ct, t0, t1 = tiles(oracle, (cur, *_chroma_for(w, h, 121)), 122), tiles(oracle, p0, 123), tiles(oracle, p1, 124)
        for wp in (None, list(B.WEIGHTS.values())[n]):
            want_costs, want_dir = B.costs3(oracle, cur, p0[0], p1[0], mv0, mv1, wp, 9)
            costs, direction = codec.satd8x8_bi_costs(ct, t0, t1, w, h, mv0, mv1, _wp(codec, wp), 9)
            assert np.array_equal(costs, want_costs) and np.array_equal(direction, want_dir), (kind, wp is None)
    dc, d0, d1, dm0, dm1 = dev(codec, ct), dev(codec, t0), dev(codec, t1), dev(codec, records(mv0)), dev(codec, records(mv1))
    dk, dd = dev(codec, np.full(nb * 3, 0xA5A5A5A5, np.uint32)), dev(codec, np.full(max(nb, 16), 0xA5, np.uint8))
    wpc = _wp(codec, wp)
    codec.satd8x8_bi_costs_dev(dc.ptr, d0.ptr, d1.ptr, w, h, dm0.ptr, dm1.ptr, dk.ptr, 0, wpc, 9)
    codec.satd8x8_bi_costs_dev(dc.ptr, d0.ptr, d1.ptr, w, h, dm0.ptr, dm1.ptr, 0, dd.ptr, wpc, 9)
    codec.stream_sync()
    assert np.array_equal(dk.download(np.uint32, nb * 3).reshape(nb, 3), want_costs) and np.array_equal(dd.download(np.uint8, nb), want_dir)


@gpu
def test_identical_lists_tie_and_list_0_wins(codec, oracle):
    w, h = 48, 32
    cur, ref = me_frames(w, h, 0, 130, mv=(1, -2), noise=4)
    ct, rt = tiles(oracle, (cur, *_chroma_for(w, h, 131)), 132), tiles(oracle, (ref, *_chroma_for(w, h, 133)), 134)
    mv = R.mv_mix_q((w // 8) * (h // 8), w, h, 135)
    costs, direction = codec.satd8x8_bi_costs(ct, rt, rt, w, h, mv, mv)
    assert (costs[:, 0] == costs[:, 1]).all() and (costs[:, 0] == costs[:, 2]).all() and (direction == 1).all()


@gpu
def test_c0_is_the_cost_the_uni_refinement_reported(codec, oracle):
    w, h = 144, 80
    nb = (w // 8) * (h // 8)
    cur, ref0 = me_frames(w, h, 0, 140, mv=(-3, 2), noise=5)
    ref1 = R.plane("random", w, h, 141)
    ct, t0, t1 = (tiles(oracle, (p, *_chroma_for(w, h, 142 + i)), 146 + i) for i, p in enumerate((cur, ref0, ref1)))
    q, q_cost, _ = codec.refine_qpel_tiles(ct, t0, w, h, _mv_mix(nb, w, h, 149))
    costs, _ = codec.satd8x8_bi_costs(ct, t0, t1, w, h, q, R.mv_mix_q(nb, w, h, 150))
    assert np.array_equal(costs[:, 0], q_cost)


# ---- 3. the bi refinement ----------------------------------------------------------------------------------------------------------------
def _refine_case(w, h):
    """(cur, fixed reference, refined reference planes, mv_fix in quarter samples, integer vectors, beyond +-8191 at the larger sizes)"""
    nb = (w // 8) * (h // 8)
    cur, ref = me_frames(w, h, 0, 200 + w, mv=(2, -1), noise=4)
    fix = R.plane("extreme", w, h, 201 + w)
    mv_int = _mv_mix(nb, w, h, 202 + h)
    if nb >= 24:
        assert (np.abs(mv_int.astype(np.int64)) > 8191).any()
    return cur, fix, ref, R.mv_mix_q(nb, w, h, 203 + w), mv_int


@pytest.fixture(scope="module")
def refine_refs(oracle):
    """the reference's answers, computed once per case"""
    cache = {}

    def get(w, h, lst, weights):
        if (w, h, lst, weights) not in cache:
            cur, fix, ref, mv_fix, mv_int = _refine_case(w, h)
            wp = B.WEIGHTS[weights] if weights else None
            cache[(w, h, lst, weights)] = B.refine_bi(oracle, cur, fix, mv_fix, ref, mv_int, lst, wp)
        return cache[(w, h, lst, weights)]
    return get


@gpu
@pytest.mark.parametrize("weights", [None, "fade", "field extremes"])
@pytest.mark.parametrize("lst", [0, 1])
@pytest.mark.parametrize("w,h", [(16, 16), (48, 32), (144, 80)])
def test_refinement_against_the_reference(codec, oracle, refine_refs, w, h, lst, weights):
    cur, fix, ref, mv_fix, mv_int = _refine_case(w, h)
    want_mv, want_cost, want_costs = refine_refs(w, h, lst, weights)
    ct, ft, rt = (tiles(oracle, (p, *_chroma_for(w, h, 210 + i)), 214 + i) for i, p in enumerate((cur, fix, ref)))
    wp = _wp(codec, B.WEIGHTS[weights] if weights else None)
    mv, cost, costs = codec.satd8x8_refine_bi_qpel(ct, ft, mv_fix, rt, mv_int, lst, w, h, wp, want_costs=True)
    assert np.array_equal(costs, want_costs)
    assert np.array_equal(mv, want_mv) and np.array_equal(cost, want_cost)


@gpu
def test_refinement_in_place_without_costs_and_its_centre_is_c2(codec, oracle, refine_refs):
    """d_best == d_int and d_costs NULL give the same records; the centre entry of d_costs is the c2 of the cost call for the
    vectors (4 m, mv_fix)"""
    w, h = 48, 32
    nb = (w // 8) * (h // 8)
    cur, fix, ref, mv_fix, mv_int = _refine_case(w, h)
    ct, ft, rt = (tiles(oracle, (p, *_chroma_for(w, h, 220 + i)), 224 + i) for i, p in enumerate((cur, fix, ref)))
    centre = (4 * np.clip(mv_int.astype(np.int64), -8191, 8191)).astype(np.int16)
    wp = _wp(codec, B.WEIGHTS["fade"])
    for lst in (0, 1):
        want_mv, want_cost, want_costs = refine_refs(w, h, lst, "fade")
        dc, df, dr, dmf, di = dev(codec, ct), dev(codec, ft), dev(codec, rt), dev(codec, records(mv_fix)), dev(codec, records(mv_int, 0xFFFFFFFF))
        codec.satd8x8_refine_bi_qpel_dev(dc.ptr, df.ptr, dmf.ptr, dr.ptr, di.ptr, lst, w, h, di.ptr, 0, wp)
        codec.stream_sync()
        mv, cost = _unpack(di.download(np.uint8, nb * 8), nb)
        assert np.array_equal(mv, want_mv) and np.array_equal(cost, want_cost)
        refs, mvs = ((rt, ft), (centre, mv_fix)) if lst == 0 else ((ft, rt), (mv_fix, centre))
        costs3, _ = codec.satd8x8_bi_costs(ct, refs[0], refs[1], w, h, mvs[0], mvs[1], wp)
        assert np.array_equal(costs3[:, 2], want_costs[:, 24])
        for t, d in ((ct, dc), (ft, df), (rt, dr)):
            assert np.array_equal(d.download(np.uint8, w * h * 2), t)


# ---- 4. a captured graph -------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_three_calls_eagerly_and_in_a_graph(codec, oracle):
    """refine list 0 against list 1 -> costs and directions -> motion compensation under those directions, on one stream, eagerly
    and replayed from a graph: the same bytes, and the statement's"""
    w, h = 48, 32
    nb = (w // 8) * (h // 8)
    cur, fix, ref, mv_fix, mv_int = _refine_case(w, h)
    ct, ft, rt = (tiles(oracle, (p, *_chroma_for(w, h, 230 + i)), 234 + i) for i, p in enumerate((cur, fix, ref)))
    weights = B.WEIGHTS["fade"]
    wp = _wp(codec, weights)
    start = sentinels(w, h, 237)
    q, _, _ = B.refine_bi(oracle, cur, fix, mv_fix, ref, mv_int, 0, weights)
    want_costs, want_dir = B.costs3(oracle, cur, ref, fix, q, mv_fix, weights, 25)
    want_pred = B.bi_tiles(oracle, rt, ft, q, mv_fix, want_dir, weights, w, h, start)

    dc, df, dr, dmf, di = dev(codec, ct), dev(codec, ft), dev(codec, rt), dev(codec, records(mv_fix)), dev(codec, records(mv_int))
    db, dk, dd, dp = codec.alloc(nb * 8), codec.alloc(nb * 12), codec.alloc(max(nb, 16)), dev(codec, start)
    st = codec.stream_create()
    try:
        def enqueue():
            codec.satd8x8_refine_bi_qpel_dev(dc.ptr, df.ptr, dmf.ptr, dr.ptr, di.ptr, 0, w, h, db.ptr, 0, wp, stream=st)
            codec.satd8x8_bi_costs_dev(dc.ptr, dr.ptr, df.ptr, w, h, db.ptr, dmf.ptr, dk.ptr, dd.ptr, wp, 25, stream=st)
            codec.motion_comp_bi_qpel_dev(dr.ptr, df.ptr, db.ptr, dmf.ptr, w, h, dp.ptr, dd.ptr, wp, 3, stream=st)

        def results():
            codec.stream_sync(st)
            return db.download(np.uint8, nb * 8), dk.download(np.uint32, nb * 3), dd.download(np.uint8, nb), dp.download(np.uint8, w * h * 2)

        codec.graph_begin(st)
        enqueue()
        graph = codec.graph_end(st)
        try:
            enqueue()
            eager = results()
            assert np.array_equal(_unpack(eager[0], nb)[0], q)
            assert np.array_equal(eager[1].reshape(nb, 3), want_costs) and np.array_equal(eager[2], want_dir)
            assert np.array_equal(eager[3], want_pred)
            for buf in (db, dk, dd):
                buf.upload(np.zeros(buf.nbytes, np.uint8))
            dp.upload(start)
            codec.graph_launch(graph, st)
            for x, y in zip(eager, results()):
                assert np.array_equal(x, y)
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 5. minimum alignment inside guard bands -----------------------------------------------------------------------------------------------
AW, AH = 48, 32
ANB = (AW // 8) * (AH // 8)
PTRS = {"mc": {"d_ref0": 16, "d_ref1": 16, "d_mv0": 8, "d_mv1": 8, "d_dir": 1, "d_pred": 16},
        "costs": {"d_cur": 16, "d_ref0": 16, "d_ref1": 16, "d_mv0": 8, "d_mv1": 8, "d_costs": 4, "d_dir": 1},
        "refine": {"d_cur": 16, "d_ref_fix": 16, "d_mv_fix": 8, "d_ref": 16, "d_int": 8, "d_best": 8, "d_costs": 4}}
NAMES = {"mc": b"xMotionCompBiQpelTiles", "costs": b"xSatd8x8BiCostsFromTiles", "refine": b"xSatd8x8RefineBiQpelFromTiles"}


@pytest.fixture(scope="module")
def arena_data(oracle):
    cur, fix, ref, mv_fix, mv_int = _refine_case(AW, AH)
    ct, ft, rt = (tiles(oracle, (p, *_chroma_for(AW, AH, 300 + i)), 304 + i) for i, p in enumerate((cur, fix, ref)))
    return dict(planes=(cur, fix, ref), ct=ct, t0=rt, t1=ft, mv0=R.mv_mix_q(ANB, AW, AH, 307), mv1=mv_fix, mv_int=mv_int, direction=B.directions(ANB, 308))


def _arena(codec, oracle, data, call, disp, guard_seed):
    """the call's buffers placed by `disp`, and the call itself on them"""
    wp = _wp(codec, B.WEIGHTS["fade"])
    L, c = codec.L, codec.ctx
    if call == "mc":
        skip = (data["direction"].reshape(AH // 8, AW // 8) & 3) == 0          # blocks of direction 0 are holes: marked planes, in tile order
        marks = oracle.conv_input_fmt(*(np.repeat(np.repeat(skip, e, 0), e, 1).astype(np.uint8) for e in (8, 4, 4))).reshape(-1, 512)
        written = np.zeros(marks.shape, bool)
        written[:, :384] = marks[:, :384] == 0
        payload = {"d_ref0": data["t0"], "d_ref1": data["t1"], "d_mv0": records(data["mv0"]), "d_mv1": records(data["mv1"]), "d_dir": data["direction"]}
        a, s = arena_slots(codec, PTRS[call], ("d_pred",), payload, disp, guard_seed, written={"d_pred": written.ravel()}, sizes={"d_pred": AW * AH * 2})
        fn = lambda: L.xMotionCompBiQpelTiles(c, s["d_ref0"].ptr, s["d_ref1"].ptr, s["d_mv0"].ptr, s["d_mv1"].ptr, s["d_dir"].ptr, ctypes.byref(wp), 3, AW, AH,
                                              s["d_pred"].ptr, None)
    elif call == "costs":
        payload = {"d_cur": data["ct"], "d_ref0": data["t0"], "d_ref1": data["t1"], "d_mv0": records(data["mv0"]), "d_mv1": records(data["mv1"])}
        a, s = arena_slots(codec, PTRS[call], ("d_costs", "d_dir"), payload, disp, guard_seed, sizes={"d_costs": ANB * 12, "d_dir": ANB})
        fn = lambda: L.xSatd8x8BiCostsFromTiles(c, s["d_cur"].ptr, s["d_ref0"].ptr, s["d_ref1"].ptr, AW, AH, s["d_mv0"].ptr, s["d_mv1"].ptr, ctypes.byref(wp), 11,
                                                s["d_costs"].ptr, s["d_dir"].ptr, None)
    else:
        payload = {"d_cur": data["ct"], "d_ref_fix": data["t1"], "d_mv_fix": records(data["mv1"]), "d_ref": data["t0"], "d_int": records(data["mv_int"])}
        a, s = arena_slots(codec, PTRS[call], ("d_best", "d_costs"), payload, disp, guard_seed, sizes={"d_best": ANB * 8, "d_costs": ANB * 196})
        fn = lambda: L.xSatd8x8RefineBiQpelFromTiles(c, s["d_cur"].ptr, s["d_ref_fix"].ptr, s["d_mv_fix"].ptr, s["d_ref"].ptr, s["d_int"].ptr, 1, ctypes.byref(wp),
                                                     AW, AH, s["d_best"].ptr, s["d_costs"].ptr, None)
    return a, s, fn


@gpu
@pytest.mark.parametrize("call", list(PTRS))
def test_at_minimum_alignment(codec, oracle, arena_data, call):
    """every pointer at exactly its documented alignment: the guards, the holes and the inputs are intact, the results are the
    statement's and do not depend on the garbage around the inputs"""
    cur, fix, ref = arena_data["planes"]
    weights = B.WEIGHTS["fade"]
    results = []
    for guard_seed in (51, 61):
        a, s, fn = _arena(codec, oracle, arena_data, call, displacements(PTRS[call]), guard_seed)
        rc = fn()
        sync_or_exit(codec, rc)
        assert rc == 0, codec.L.xHipLastError(codec.ctx)
        got = a.check()
        if call == "mc":
            base = s["d_pred"].image[s["d_pred"].start:][:AW * AH * 2]
            assert np.array_equal(got["d_pred"], B.bi_tiles(oracle, arena_data["t0"], arena_data["t1"], arena_data["mv0"], arena_data["mv1"],
                                                            arena_data["direction"], weights, AW, AH, base))
            results.append((got["d_pred"],))
        elif call == "costs":
            want_costs, want_dir = B.costs3(oracle, cur, ref, fix, arena_data["mv0"], arena_data["mv1"], weights, 11)
            assert np.array_equal(got["d_costs"].view(np.uint32).reshape(ANB, 3), want_costs) and np.array_equal(got["d_dir"], want_dir)
            results.append((got["d_costs"], got["d_dir"]))
        else:
            want_mv, want_cost, want_costs = B.refine_bi(oracle, cur, fix, arena_data["mv1"], ref, arena_data["mv_int"], 1, weights)
            got_mv, got_cost = _unpack(got["d_best"], ANB)
            assert np.array_equal(got["d_costs"].view(np.uint32).reshape(ANB, 49), want_costs)
            assert np.array_equal(got_mv, want_mv) and np.array_equal(got_cost, want_cost)
            results.append((got["d_best"], got["d_costs"]))
    for x, y in zip(*results):
        assert np.array_equal(x, y)


@gpu
@pytest.mark.parametrize("call,ptr", [(c, p) for c in PTRS for p, align in PTRS[c].items() if align > 1])
def test_half_alignment_is_rejected(codec, oracle, arena_data, call, ptr):
    a, _, fn = _arena(codec, oracle, arena_data, call, displacements(PTRS[call], halved=ptr), 71)
    rc = fn()
    sync_or_exit(codec, rc)
    assert rc == EINVAL and NAMES[call] in codec.L.xHipLastError(codec.ctx)
    a.check_untouched()


# ---- 6. arguments --------------------------------------------------------------------------------------------------------------------------
def _bad_weights(codec):
    out = []
    for field, index, value in (("w", (0, 0), 128), ("w", (1, 2), -129), ("o", (0, 1), 128), ("o", (1, 0), -129), ("log2_denom", 0, 8), ("log2_denom", 1, 255)):
        wp = codec.wp_params()
        if field == "log2_denom":
            wp.log2_denom[index] = value
        else:
            getattr(wp, field)[index[0]][index[1]] = value
        out.append(wp)
    return out


@gpu
def test_argument_errors(codec):
    """one call per rule of each entry point on a 64x64 frame; a refused call names its entry point and launches nothing (the
    outputs keep their fill), the base tuples are accepted"""
    L, ctx = codec.L, codec.ctx
    buf = codec.alloc(12 << 20)
    fill = np.full(12 << 20, 0x5A, np.uint8)
    buf.upload(fill)
    M = 1 << 20
    c, r0, r1, m0, m1, i, d, p, b, k, k3 = (buf.ptr + n * M for n in range(1, 12))   # 64x64: tiles 8 KiB, 64 records 512 bytes, 64 directions
    top, top8 = ctypes.c_void_p(2 ** 64 - 4096), ctypes.c_void_p(2 ** 64 - 8)       # no frame fits behind top, no 64 records behind top8
    ok = ctypes.byref(codec.wp_params())
    bad = [ctypes.byref(wp) for wp in _bad_weights(codec)]

    def refused(fn, name, cases):
        for args in cases:
            assert fn(ctx, *args, None) == EINVAL, (name, args)
            assert name in L.xHipLastError(ctx), (name, args)

    mc = lambda **kw: tuple({**dict(r0=r0, r1=r1, m0=m0, m1=m1, d=d, wp=ok, planes=3, w=64, h=64, p=p), **kw}.values())
    assert L.xMotionCompBiQpelTiles(None, *mc(), None) == EINVAL
    refused(L.xMotionCompBiQpelTiles, NAMES["mc"],
            [mc(w=56), mc(h=8), mc(w=0), mc(h=-16), mc(planes=0), mc(planes=4)] + [mc(wp=x) for x in bad] +
            [mc(r0=None), mc(r1=None), mc(m0=None), mc(m1=None), mc(p=None)] +
            [mc(r0=r0 + 8), mc(r1=r1 + 8), mc(m0=m0 + 4), mc(m1=m1 + 4), mc(p=p + 8)] +
            [mc(r0=top), mc(r1=top), mc(m0=top8), mc(m1=top8), mc(d=ctypes.c_void_p(2 ** 64 - 32)), mc(p=top)] +
            [mc(p=r0), mc(p=r1 + 4096), mc(p=r0 - 4096), mc(p=m0 - 8192 + 16), mc(m1=p + 8192 - 8), mc(d=p + 100)])
    cost = lambda **kw: tuple({**dict(c=c, r0=r0, r1=r1, w=64, h=64, m0=m0, m1=m1, wp=ok, pen=5, k=k3, d=d), **kw}.values())
    assert L.xSatd8x8BiCostsFromTiles(None, *cost(), None) == EINVAL
    refused(L.xSatd8x8BiCostsFromTiles, NAMES["costs"],
            [cost(w=56), cost(h=8), cost(w=0), cost(pen=-1), cost(pen=65536), cost(k=None, d=None)] + [cost(wp=x) for x in bad] +
            [cost(c=None), cost(r0=None), cost(r1=None), cost(m0=None), cost(m1=None)] +
            [cost(c=c + 8), cost(r0=r0 + 8), cost(r1=r1 + 8), cost(m0=m0 + 4), cost(m1=m1 + 4), cost(k=k3 + 2)] +
            [cost(c=top), cost(r0=top), cost(r1=top), cost(m0=top8), cost(m1=top8), cost(k=ctypes.c_void_p(2 ** 64 - 64)), cost(d=ctypes.c_void_p(2 ** 64 - 32))] +
            [cost(k=c + 8188), cost(k=r1 - 4), cost(k=m0 + 256), cost(d=c), cost(d=m1 + 511), cost(d=k3 + 767), cost(k=d - 764)])
    ref = lambda **kw: tuple({**dict(c=c, rf=r1, mf=m1, r=r0, i=i, lst=0, wp=ok, w=64, h=64, b=b, k=k), **kw}.values())
    assert L.xSatd8x8RefineBiQpelFromTiles(None, *ref(), None) == EINVAL
    refused(L.xSatd8x8RefineBiQpelFromTiles, NAMES["refine"],
            [ref(w=56), ref(h=8), ref(w=0), ref(lst=-1), ref(lst=2)] + [ref(wp=x) for x in bad] +
            [ref(c=None), ref(rf=None), ref(mf=None), ref(r=None), ref(i=None), ref(b=None)] +
            [ref(c=c + 8), ref(rf=r1 + 8), ref(mf=m1 + 4), ref(r=r0 + 8), ref(i=i + 4), ref(b=b + 4), ref(k=k + 2)] +
            [ref(c=top), ref(rf=top), ref(mf=top8), ref(r=top), ref(i=top8), ref(b=top8), ref(k=top)] +
            [ref(b=c + 4096), ref(b=r0 - 256), ref(b=i + 8), ref(b=m1), ref(k=c + 8188), ref(k=r1 - 4), ref(k=i + 256), ref(k=b - 12540), ref(k=m1 + 508)])
    codec.stream_sync()
    assert np.array_equal(buf.download(np.uint8, 12 << 20), fill)           # nothing was launched
    for args in (mc(), mc(d=None), mc(wp=None), mc(r1=r0), mc(planes=1), mc(planes=2)):
        assert L.xMotionCompBiQpelTiles(ctx, *args, None) == 0, args
    for args in (cost(), cost(k=None), cost(d=None), cost(wp=None), cost(c=r0, r1=r0), cost(pen=0), cost(pen=65535)):
        assert L.xSatd8x8BiCostsFromTiles(ctx, *args, None) == 0, args
    for args in (ref(), ref(k=None), ref(wp=None), ref(lst=1), ref(b=i), ref(rf=c, r=c)):
        assert L.xSatd8x8RefineBiQpelFromTiles(ctx, *args, None) == 0, args
    codec.stream_sync()
