"""Adaptive loop filter on tiled frames: xAlfClassifyGpu / StatsGpu / SumStatsGpu / DecideGpu / ApplyGpu against the reference statement
of tests/_alf_ref.py (the header's arithmetic in numpy int64, checked against plain loops by tests/test_alf_ref.py).  Every comparison
is bit-exact; every test but the export test is marked gpu."""
import ctypes
import subprocess

import numpy as np
import pytest

import _alf_ref as R
import x266_amd
from _dev import EINVAL, dev, noise, run, sync_or_exit, tiles
from _util import splitmix64

gpu = pytest.mark.gpu
NAMES = ("xAlfClassifyGpu", "xAlfStatsGpu", "xAlfSumStatsGpu", "xAlfDecideGpu", "xAlfApplyGpu")
WORDS = R.CTU_WORDS


# ---- the export test (CPU) ------------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_five_calls():
    x266_amd.build_library()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode().split()
    lib = x266_amd.load_library()
    for name in NAMES:
        assert name in exported, name
        assert getattr(lib, name).argtypes, name                            # bound by _lib.py, with its argument types
    for method in ("alf_classify", "alf_stats", "alf_sum_stats", "alf_decide", "alf_apply"):
        assert callable(getattr(x266_amd.Codec, method)) and callable(getattr(x266_amd.Codec, method + "_dev")), method
    luma, chroma = x266_amd.Codec.alf_pack_filters(np.full((2, 25, 12), -128), np.full((2, 25, 12), 3), np.arange(6) - 3)
    assert luma.shape == (2, 600) and chroma.shape == (1, 16)
    assert (luma[:, :300] == 0x80).all() and (luma[:, 300:] == 3).all() and chroma[0].tolist() == [253, 254, 255, 0, 1, 2] + [0] * 10


@pytest.fixture(scope="module")
def cases(oracle):
    """per (kind, w, h): planes, tile arrays and the statement's class map and statistics, computed once"""
    cache = {}

    def get(kind, w, h):
        if (kind, w, h) not in cache:
            org_p, dec_p = R.case(kind, w, h)
            c = {"org_p": org_p, "dec_p": dec_p, "org": tiles(oracle, org_p, 40 + h), "dec": tiles(oracle, dec_p, 41 + h), "classes": R.classify(dec_p[0])}
            c["stats"] = R.stats(org_p, dec_p, c["classes"]) if kind in R.STATS_KINDS else None
            cache[(kind, w, h)] = c
        return cache[(kind, w, h)]
    return get


def _class_map(w, h, seed):
    """seeded random bytes over the whole byte range; 100 seeded places carry the 25 x 4 (class, transposition) pairs, so that all occur
    at every size, class 24 also as 25..31"""
    nb = (w // 4) * (h // 4)
    cmap = noise(nb, seed)
    order = np.argsort(splitmix64(seed + 1, 0, nb), kind="stable")[:100]
    pairs = np.arange(100)
    cmap[order] = (cmap[order] & 0x80) | ((pairs % 4) << 5).astype(np.uint8) | np.where(pairs // 4 == 24, 24 | (cmap[order] & 7), pairs // 4).astype(np.uint8)
    return cmap.reshape(h // 4, w // 4)


def _ctrl_cycle(n, n_luma, n_chroma, seed):
    """d_ctrl that walks 0, every valid value and values above the count (255 among them), differently per component"""
    vals = [list(range(0, n_luma + 3)) + [255], list(range(0, n_chroma + 3)) + [200], [255] + list(range(n_chroma + 2, -1, -1))]
    return np.array([[vals[m][(t + seed + 2 * m) % len(vals[m])] for m in range(3)] for t in range(n)], np.uint8)


# ---- 1. classification ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", R.SIZES)
def test_classification(codec, cases, w, h):
    nb = (w // 4) * (h // 4)
    for kind in R.CLASSIFY_KINDS + ("spikes",):
        c = cases(kind, w, h)
        d_dec, d_cls = dev(codec, c["dec"]), dev(codec, noise(nb + 64, 50))
        run(codec, codec.alf_classify_dev, d_dec.ptr, w, h, d_cls.ptr)
        got = d_cls.download(np.uint8, nb + 64)
        assert np.array_equal(got[:nb], c["classes"].ravel()), kind
        assert np.array_equal(got[nb:], noise(nb + 64, 50)[nb:]), kind      # nothing behind the map
        assert np.array_equal(d_dec.download(np.uint8, c["dec"].size), c["dec"]), kind
    assert np.array_equal(codec.alf_classify(c["dec"], w, h), c["classes"])


# ---- 2. apply with a caller's class map -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", R.SIZES)
def test_apply_with_a_callers_class_map(codec, oracle, cases, w, h):
    """random class bytes over the whole byte range, random int8 coefficients, all clip indices, every kind of d_ctrl byte, on noise"""
    n = codec.ctu_count(w, h)
    c = cases("noise", w, h)
    cmap = _class_map(w, h, 60 + w)
    cls, tr = R.decode(cmap)
    assert len(set((cls * 4 + tr).ravel().tolist())) == 100 and (cmap & 31).max() > 24
    base = noise(w * h * 2, 61)
    d_in, d_cls = dev(codec, c["dec"]), dev(codec, cmap)
    for n_luma, n_chroma in ((1, 1), (3, 8), (8, 1)):
        luma, chroma = R.random_filters(n_luma, n_chroma, 62 + n_luma)
        assert {0x80, 0x7F} <= set(luma[:, :300].ravel().tolist()) and set((luma[:, 300:] & 3).ravel().tolist()) == {0, 1, 2, 3}
        for seed in range(-(-(max(n_luma, n_chroma) + 4) // n)):                # over the seeds every CTU-independent value of d_ctrl occurs
            ctrl = _ctrl_cycle(n, n_luma, n_chroma, seed)
            d_luma, d_chroma, d_ctrl, d_out = dev(codec, luma), dev(codec, chroma), dev(codec, ctrl), dev(codec, base)
            run(codec, codec.alf_apply_dev, d_in.ptr, w, h, d_cls.ptr, d_luma.ptr, n_luma, d_chroma.ptr, n_chroma, d_ctrl.ptr, d_out.ptr)
            want = R.apply_tiles(oracle, c["dec"], w, h, cmap, luma, chroma, ctrl, base)
            assert np.array_equal(d_out.download(np.uint8, base.size), want), (n_luma, n_chroma, seed)
            for d, a in ((d_luma, luma), (d_chroma, chroma), (d_ctrl, ctrl), (d_cls, cmap), (d_in, c["dec"])):
                assert np.array_equal(d.download(np.uint8, a.size), a.ravel())
    assert np.array_equal(codec.alf_apply(c["dec"], w, h, luma, chroma, ctrl, classes=cmap, base=base), want)
    # no sets at all, with NULL arrays: a copy of the two planes
    d_out = dev(codec, base)
    run(codec, codec.alf_apply_dev, d_in.ptr, w, h, d_cls.ptr, 0, 0, 0, 0, d_ctrl.ptr, d_out.ptr)
    got = d_out.download(np.uint8, base.size).reshape(-1, 512)
    assert np.array_equal(got[:, :384], c["dec"].reshape(-1, 512)[:, :384]) and np.array_equal(got[:, 384:], base.reshape(-1, 512)[:, 384:])


# ---- 3. internal classification ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", R.SIZES)
def test_internal_classification_is_the_two_step_path(codec, oracle, cases, w, h):
    n, nb = codec.ctu_count(w, h), (w // 4) * (h // 4)
    luma, chroma = R.random_filters(2, 2, 70)
    ctrl = _ctrl_cycle(n, 2, 2, 1)
    ctrl[:, 0] = 1 + np.arange(n) % 2                                       # every CTU filters its luma
    base = noise(w * h * 2, 71)
    for kind in ("quad", "blur"):
        c = cases(kind, w, h)
        d_org, d_dec, d_cls = dev(codec, c["org"]), dev(codec, c["dec"]), codec.alloc(max(nb, 16))
        d_luma, d_chroma, d_ctrl = dev(codec, luma), dev(codec, chroma), dev(codec, ctrl)
        run(codec, codec.alf_classify_dev, d_dec.ptr, w, h, d_cls.ptr)
        outs, stats = [], []
        for d_map in (d_cls.ptr, 0):
            d_out, d_stats = dev(codec, base), dev(codec, noise(n * WORDS * 4, 72))
            run(codec, codec.alf_apply_dev, d_dec.ptr, w, h, d_map, d_luma.ptr, 2, d_chroma.ptr, 2, d_ctrl.ptr, d_out.ptr)
            run(codec, codec.alf_stats_dev, d_org.ptr, d_dec.ptr, w, h, d_map, d_stats.ptr)
            outs.append(d_out.download(np.uint8, base.size))
            stats.append(d_stats.download(np.int32, n * WORDS))
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(stats[0], stats[1]), kind
        assert np.array_equal(outs[1], R.apply_tiles(oracle, c["dec"], w, h, None, luma, chroma, ctrl, base)), kind
        assert np.array_equal(stats[1], R.stats_words(R.stats(c["org_p"], c["dec_p"]))), kind


# ---- 4. statistics and totals -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", R.SIZES)
def test_statistics_and_totals(codec, cases, w, h):
    n = codec.ctu_count(w, h)
    for kind in R.STATS_KINDS:
        c = cases(kind, w, h)
        words = R.stats_words(c["stats"])
        assert np.array_equal(words.astype(np.int64), c["stats"].ravel())   # the statement's sums fit int32
        d_org, d_dec, d_cls, d_stats = dev(codec, c["org"]), dev(codec, c["dec"]), dev(codec, c["classes"]), dev(codec, noise(n * WORDS * 4 + 64, 80))
        run(codec, codec.alf_stats_dev, d_org.ptr, d_dec.ptr, w, h, d_cls.ptr, d_stats.ptr)
        assert np.array_equal(d_stats.download(np.int32, n * WORDS), words), kind
        assert np.array_equal(d_stats.download(np.uint8, n * WORDS * 4 + 64)[n * WORDS * 4:], noise(n * WORDS * 4 + 64, 80)[n * WORDS * 4:]), kind
        assert np.array_equal(d_org.download(np.uint8, c["org"].size), c["org"]) and np.array_equal(d_dec.download(np.uint8, c["dec"].size), c["dec"]), kind
        masks = [None, np.zeros(n, np.uint8), (noise(n, 81 + w) & 1) * (1 + noise(n, 82) % 255).astype(np.uint8), np.ones(n, np.uint8)]
        for mask in masks:
            d_total = dev(codec, noise(WORDS * 8, 83))
            d_mask = None if mask is None else dev(codec, mask)
            run(codec, codec.alf_sum_stats_dev, d_stats.ptr, n, 0 if mask is None else d_mask.ptr, d_total.ptr)
            assert np.array_equal(d_total.download(np.int64, WORDS), R.sum_stats(c["stats"], mask)), (kind, mask)
        assert np.array_equal(d_stats.download(np.int32, n * WORDS), words), kind
    # a caller's map with every (class, transposition) pair, and the host-array forms
    c = cases("far", w, h)
    cmap = _class_map(w, h, 84)
    want = R.stats(c["org_p"], c["dec_p"], cmap)
    got = codec.alf_stats(c["org"], c["dec"], w, h, classes=cmap)
    assert np.array_equal(got.ravel(), R.stats_words(want))
    assert np.array_equal(codec.alf_sum_stats(got), R.sum_stats(want))


# ---- 5. decision ------------------------------------------------------------------------------------------------------------------------
def _decision_sets(c):
    """zero filters, the filters solved from the statement's totals, and their negation; chroma: zero, U's and V's solution, the negated U's"""
    lc, uc, vc = R.solve(R.sum_stats(c["stats"]))
    zero_l, zero_c = np.zeros((25, 12), np.int64), np.zeros(6, np.int64)
    return R.pack(np.stack([zero_l, lc, np.clip(-lc, -128, 127)]), None, np.stack([zero_c, uc, vc, np.clip(-uc, -128, 127)]), None)


@gpu
@pytest.mark.parametrize("w,h", R.SIZES)
def test_decision(codec, cases, w, h):
    n = codec.ctu_count(w, h)
    picked = set()
    for kind in ("blur", "noise", "far"):
        c = cases(kind, w, h)
        luma, chroma = _decision_sets(cases("blur", w, h))
        st = c["stats"].copy()
        if n > 1:
            st[n - 1, 0:2300:92] = 0                                        # a CTU without luma samples, and one without V samples
            st[0, 2329] = 0
        d_stats, d_luma, d_chroma = dev(codec, R.stats_words(st)), dev(codec, luma), dev(codec, chroma)
        for lam in R.LAMBDAS:
            for n_luma, n_chroma in ((3, 4), (1, 1), (2, 3), (0, 0)):
                d_ctrl = dev(codec, noise(3 * n + 16, 90))
                run(codec, codec.alf_decide_dev, d_stats.ptr, n, d_luma.ptr if n_luma else 0, n_luma, d_chroma.ptr if n_chroma else 0, n_chroma, lam, d_ctrl.ptr)
                want = R.decide(st, luma[:n_luma], chroma[:n_chroma], lam)
                got = d_ctrl.download(np.uint8, 3 * n + 16)
                assert np.array_equal(got[:3 * n], want.ravel()), (kind, lam, n_luma, n_chroma)
                assert np.array_equal(got[3 * n:], noise(3 * n + 16, 90)[3 * n:])
                picked |= {(kind, int(v)) for v in want.ravel()}
        assert np.array_equal(d_stats.download(np.int32, n * WORDS), R.stats_words(st))
    assert ("blur", 2) in picked and ("blur", 0) in picked                 # the solved filters win somewhere and something stays off
    assert np.array_equal(codec.alf_decide(st, luma, chroma, 37), R.decide(st, luma, chroma, 37))


# ---- 6. frame edges and CTU seams ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", R.SIZES)
def test_frame_edges_and_ctu_seams(codec, oracle, cases, w, h):
    """a constant frame with one bright sample near each corner and each seam: every output and statistic a neighbouring CTU or the
    clamped border contributes to"""
    n = codec.ctu_count(w, h)
    c = cases("spikes", w, h)
    luma, chroma = R.random_filters(2, 2, 95)
    luma[:, 300:], chroma[:, 6:12] = 0, 0                                   # clip index 0: a spike reaches every tap unclipped
    ctrl = np.tile(np.array([1, 2, 1], np.uint8), (n, 1))
    base = noise(w * h * 2, 96)
    d_org, d_dec, d_out, d_stats = dev(codec, c["org"]), dev(codec, c["dec"]), dev(codec, base), codec.alloc(n * WORDS * 4)
    d_luma, d_chroma, d_ctrl = dev(codec, luma), dev(codec, chroma), dev(codec, ctrl)
    run(codec, codec.alf_apply_dev, d_dec.ptr, w, h, 0, d_luma.ptr, 2, d_chroma.ptr, 2, d_ctrl.ptr, d_out.ptr)
    run(codec, codec.alf_stats_dev, d_org.ptr, d_dec.ptr, w, h, 0, d_stats.ptr)
    want = R.apply_tiles(oracle, c["dec"], w, h, None, luma, chroma, ctrl, base)
    assert not np.array_equal(want.reshape(-1, 512)[:, :384], c["dec"].reshape(-1, 512)[:, :384])
    assert np.array_equal(d_out.download(np.uint8, base.size), want)
    assert np.array_equal(d_stats.download(np.int32, n * WORDS), R.stats_words(R.stats(c["org_p"], c["dec_p"])))


# ---- 7. one graph ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_classify_stats_decide_and_apply_in_one_graph(codec, oracle, cases):
    w, h = 144, 80
    n, nb = codec.ctu_count(w, h), (w // 4) * (h // 4)
    luma, chroma = _decision_sets(cases("blur", w, h))
    frames = [cases(kind, w, h) for kind in ("quad", "blur", "noise")]
    d_org, d_dec, d_cls, d_stats = codec.alloc(w * h * 2), codec.alloc(w * h * 2), codec.alloc(nb), codec.alloc(n * WORDS * 4)
    d_total, d_ctrl, d_out = codec.alloc(WORDS * 8), codec.alloc(max(3 * n, 16)), codec.alloc(w * h * 2)
    d_luma, d_chroma = dev(codec, luma), dev(codec, chroma)
    st = codec.stream_create()
    try:
        def enqueue():
            codec.alf_classify_dev(d_dec.ptr, w, h, d_cls.ptr, stream=st)
            codec.alf_stats_dev(d_org.ptr, d_dec.ptr, w, h, d_cls.ptr, d_stats.ptr, stream=st)
            codec.alf_sum_stats_dev(d_stats.ptr, n, 0, d_total.ptr, stream=st)
            codec.alf_decide_dev(d_stats.ptr, n, d_luma.ptr, 3, d_chroma.ptr, 4, 37, d_ctrl.ptr, stream=st)
            codec.alf_apply_dev(d_dec.ptr, w, h, d_cls.ptr, d_luma.ptr, 3, d_chroma.ptr, 4, d_ctrl.ptr, d_out.ptr, stream=st)

        def load(i):
            d_org.upload(frames[i]["org"])
            d_dec.upload(frames[i]["dec"])
            d_out.upload(np.zeros(w * h * 2, np.uint8))

        def results():
            sync_or_exit(codec, 0, st)
            return d_out.download(np.uint8, w * h * 2), d_ctrl.download(np.uint8, 3 * n), d_total.download(np.int64, WORDS)

        load(0)
        codec.graph_begin(st)
        enqueue()
        graph = codec.graph_end(st)
        try:
            for i in (1, 2, 1):
                load(i)
                codec.graph_launch(graph, st)
                out, ctrl, total = results()
                c = frames[i]
                stats = R.stats(c["org_p"], c["dec_p"])
                want_ctrl = R.decide(stats, luma, chroma, 37)
                assert np.array_equal(total, R.sum_stats(stats)) and np.array_equal(ctrl, want_ctrl.ravel()), i
                assert np.array_equal(out, R.apply_tiles(oracle, c["dec"], w, h, None, luma, chroma, want_ctrl, np.zeros(w * h * 2, np.uint8))), i
                if i == 1:
                    assert want_ctrl.any()
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_argument_errors(codec):
    """one refused call per rule, for every call; a refused call launches nothing and names itself"""
    L, ctx = codec.L, codec.ctx
    buf = codec.alloc(8 << 20)
    fill = noise(8 << 20, 97)
    buf.upload(fill)
    M = 1 << 20
    o, d, out, st, cls, lu, ch, ctl, tot, msk = (buf.ptr + i * M // 2 for i in range(1, 11))   # 64x64: 8 KiB of tiles, 9432 bytes of statistics
    top, top8, top4, top1 = 2 ** 64 - 4096, 2 ** 64 - 8, 2 ** 64 - 4, 2 ** 64 - 1             # aligned, and nothing fits behind them
    V = ctypes.c_void_p

    def refused(name, *args):
        assert getattr(L, name)(ctx, *args, None) == EINVAL, (name, args)
        assert name.encode() in L.xHipLastError(ctx), (name, args)

    good = {"xAlfClassifyGpu": (V(d), 64, 64, V(cls)), "xAlfStatsGpu": (V(o), V(d), 64, 64, V(cls), V(st)), "xAlfSumStatsGpu": (V(st), 1, V(msk), V(tot)),
            "xAlfDecideGpu": (V(st), 1, V(lu), 1, V(ch), 1, 0, V(ctl)), "xAlfApplyGpu": (V(d), 64, 64, V(cls), V(lu), 1, V(ch), 1, V(ctl), V(out))}
    for name in NAMES:
        assert getattr(L, name)(None, *good[name], None) == EINVAL           # a NULL context is refused, not dereferenced
    for a in ((None, 64, 64, cls), (d, 64, 64, None), (d + 8, 64, 64, cls), (d, 56, 64, cls), (d, 64, 0, cls), (d, -16, 64, cls), (top, 64, 64, cls),
              (d, 64, 64, top1), (d, 64, 64, d + 100), (d, 64, 64, d - 255)):
        refused("xAlfClassifyGpu", *a)
    for a in ((None, d, 64, 64, cls, st), (o, None, 64, 64, cls, st), (o, d, 64, 64, cls, None), (o + 8, d, 64, 64, cls, st), (o, d + 8, 64, 64, cls, st),
              (o, d, 64, 64, cls, st + 2), (o, d, 72, 64, cls, st), (o, d, 64, -64, cls, st), (top, d, 64, 64, cls, st), (o, top, 64, 64, cls, st),
              (o, d, 64, 64, top1, st), (o, d, 64, 64, cls, top4), (o, d, 64, 64, cls, o + 4), (o, d, 64, 64, cls, d - 9428), (o, d, 64, 64, st + 9431, st)):
        refused("xAlfStatsGpu", *a)
    for a in ((None, 1, msk, tot), (st, 1, msk, None), (st + 2, 1, msk, tot), (st, 1, msk, tot + 4), (st, 2 ** 31, msk, tot), (st, 2 ** 62, None, tot),
              (top4, 1, msk, tot), (st, 1, top1, tot), (st, 1, msk, top8), (st, 1, msk, st + 8), (st, 2, msk, st + 2 * 9432 - 8), (st, 1, tot + 18863, tot)):
        refused("xAlfSumStatsGpu", *a)
    for a in ((None, 1, lu, 1, ch, 1, 0, ctl), (st, 1, None, 1, ch, 1, 0, ctl), (st, 1, lu, 1, None, 1, 0, ctl), (st, 1, lu, 1, ch, 1, 0, None),
              (st + 2, 1, lu, 1, ch, 1, 0, ctl), (st, 1, lu + 2, 1, ch, 1, 0, ctl), (st, 1, lu, 1, ch + 2, 1, 0, ctl),
              (st, 1, lu, -1, ch, 1, 0, ctl), (st, 1, lu, 9, ch, 1, 0, ctl), (st, 1, lu, 1, ch, -1, 0, ctl), (st, 1, lu, 1, ch, 9, 0, ctl),
              (st, 1, lu, 1, ch, 1, -1, ctl), (st, 1, lu, 1, ch, 1, 65536, ctl), (st, 2 ** 31, lu, 1, ch, 1, 0, ctl),
              (top4, 1, lu, 1, ch, 1, 0, ctl), (st, 1, top4, 1, ch, 1, 0, ctl), (st, 1, lu, 1, top4, 1, 0, ctl), (st, 1, lu, 1, ch, 1, 0, top1),
              (st, 1, lu, 1, ch, 1, 0, st + 9431), (st, 1, lu, 2, ch, 1, 0, lu + 1199), (st, 1, lu, 1, ch, 8, 0, ch + 127), (st, 2, lu, 1, ch, 1, 0, st - 5)):
        refused("xAlfDecideGpu", *a)
    for a in ((None, 64, 64, cls, lu, 1, ch, 1, ctl, out), (d, 64, 64, cls, None, 1, ch, 1, ctl, out), (d, 64, 64, cls, lu, 1, None, 1, ctl, out),
              (d, 64, 64, cls, lu, 1, ch, 1, None, out), (d, 64, 64, cls, lu, 1, ch, 1, ctl, None), (d + 8, 64, 64, cls, lu, 1, ch, 1, ctl, out),
              (d, 64, 64, cls, lu + 2, 1, ch, 1, ctl, out), (d, 64, 64, cls, lu, 1, ch + 2, 1, ctl, out), (d, 64, 64, cls, lu, 1, ch, 1, ctl, out + 8),
              (d, 56, 64, cls, lu, 1, ch, 1, ctl, out), (d, 64, 24, cls, lu, 1, ch, 1, ctl, out), (d, 64, 64, cls, lu, 9, ch, 1, ctl, out),
              (d, 64, 64, cls, lu, 1, ch, -1, ctl, out), (top, 64, 64, cls, lu, 1, ch, 1, ctl, out), (d, 64, 64, top1, lu, 1, ch, 1, ctl, out),
              (d, 64, 64, cls, top4, 1, ch, 1, ctl, out), (d, 64, 64, cls, lu, 1, top4, 1, ctl, out), (d, 64, 64, cls, lu, 1, ch, 1, top1, out),
              (d, 64, 64, cls, lu, 1, ch, 1, ctl, top), (d, 64, 64, cls, lu, 1, ch, 1, ctl, d), (d, 64, 64, cls, lu, 1, ch, 1, ctl, d + 4096),
              (d, 64, 64, cls, lu, 1, ch, 1, ctl, d - 8176), (d, 64, 64, out + 8191, lu, 1, ch, 1, ctl, out), (d, 64, 64, cls, out - 592, 1, ch, 1, ctl, out),
              (d, 64, 64, cls, lu, 1, out + 8188, 8, ctl, out), (d, 64, 64, cls, lu, 1, ch, 1, out - 2, out)):
        refused("xAlfApplyGpu", *a)
    assert np.array_equal(buf.download(np.uint8, 8 << 20), fill)            # nothing was launched
    # the edges of what is accepted: no CTUs, lambda and the counts at both ends, NULL set arrays with a count of 0, d_org == d_dec, NULL d_class
    buf.upload(np.zeros(8 << 20, np.uint8))
    for rc in (L.xAlfSumStatsGpu(ctx, V(st), 0, None, V(tot), None), L.xAlfDecideGpu(ctx, V(st), 0, V(lu), 1, V(ch), 1, 0, V(ctl), None),
               L.xAlfDecideGpu(ctx, V(st), 1, V(lu), 8, V(ch), 8, 65535, V(ctl), None), L.xAlfDecideGpu(ctx, V(st), 1, None, 0, None, 0, 0, V(ctl), None),
               L.xAlfStatsGpu(ctx, V(o), V(o), 64, 64, None, V(st), None), L.xAlfApplyGpu(ctx, V(d), 64, 64, None, None, 0, None, 0, V(ctl), V(out), None),
               L.xAlfApplyGpu(ctx, V(d), 64, 64, V(cls), V(lu), 8, V(ch), 8, V(ctl), V(out), None), L.xAlfClassifyGpu(ctx, V(d), 64, 64, V(cls), None)):
        sync_or_exit(codec, rc)
        assert rc == 0, L.xHipLastError(ctx)
