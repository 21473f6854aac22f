"""GPU (-m gpu): the transform decision (xTransformDecideCtuTilesGpu).  Check 1: all five outputs equal the composition of the existing
device calls -- xTransformCtuFromTilesDev + xRdoQuantRegionsGpu per candidate class, the argmin in numpy -- for every region of the
frame.  Check 2: they equal tests/_tdecide_ref.py (the oracle's transforms and _rdoq_ref) on a sample of regions.  Every buffer of the
call sits between the guard bands of tests/_arena.py at exactly its documented alignment; guards and inputs are checked after every
call."""
import ctypes
import functools

import numpy as np
import pytest

import _levels_ref as LR
import _quant_ref as Q
import _rdoq_ref as R
import _tdecide_ref as T
import x266_amd
from _arena import Arena
from _dev import EINVAL, call_struct, dev, sync_or_exit
from test_gpu_transform_ctu_tiles import _slot_mats, _tiles_mix, _wholly_outside, ref_inverse

pytestmark = pytest.mark.gpu

PTRS = {"d_cur": 16, "d_pred": 16, "d_qp": 1, "d_cand": 2, "d_class": 1, "d_level": 16, "d_nnz": 4, "d_stat": 8, "d_cost": 8}
DISP = {name: align * (2 * i + 1) for i, (name, align) in enumerate(PTRS.items())}          # exactly the documented alignment, no more
EXTENT = {"d_class": 1, "d_level": 2048, "d_nnz": 4, "d_stat": 16, "d_cost": 128}          # bytes per region of the outputs
FRAMES = [(64, 64), (80, 48), (144, 80)]


@functools.lru_cache(None)
def frames(w, h, kind):
    """(cur, pred) tile arrays: "kinds" the five synthetic residuals tiled over the frame, "mix" the extremes (0 / 255 / random)"""
    from _util import Oracle
    if kind == "kinds":
        cur, pred = T.content_frames(Oracle(), w, h)
    else:
        cur, pred = _tiles_mix(w, h, 0x7D00 + w), _tiles_mix(w, h, 0x7D80 + h)
    for a in (cur, pred):
        a.setflags(write=False)
    return cur, pred


def decide(codec, cur, pred, w, h, qps=None, qp=32, lam=368, cand_luma=T.CLASSES, cand_chroma=T.CLASSES, cand=None, class_bits=None, without=(),
           stream=None, same_frame=False):
    """the call inside an arena -> {"d_class", "d_level", "d_nnz", "d_stat", "d_cost"} (None for the outputs named in `without`)"""
    n = T.n_regions(w, h)
    a, s = Arena(codec), {}
    s["d_cur"] = a.input("d_cur", cur, 16, DISP["d_cur"], 61)
    s["d_pred"] = s["d_cur"] if same_frame else a.input("d_pred", pred, 16, DISP["d_pred"], 62)
    if qps is not None:
        s["d_qp"] = a.input("d_qp", np.asarray(qps, np.uint8), 1, DISP["d_qp"], 63)
    if cand is not None:
        s["d_cand"] = a.input("d_cand", np.asarray(cand, np.uint16), 2, DISP["d_cand"], 64)
    for name, each in EXTENT.items():
        if name not in without:
            s[name] = a.output(name, each * n, PTRS[name], DISP[name])
    p = codec.tdecide_params(*[s[name].ptr if name in s else 0 for name in PTRS], width=w, height=h, qp=qp, lam=lam, cand_luma=cand_luma,
                             cand_chroma=cand_chroma, class_bits=class_bits)
    call_struct(codec, "xTransformDecideCtuTilesGpu", p, stream)
    got = a.check()                                                         # guard bands and inputs
    view = {"d_class": np.uint8, "d_level": np.int16, "d_nnz": np.uint32, "d_stat": R.STAT_DTYPE, "d_cost": np.uint64}
    out = {name: got[name].view(view[name]) if name in got else None for name in EXTENT}
    out["d_level"] = out["d_level"].reshape(n, 1024)
    if out["d_cost"] is not None:
        out["d_cost"] = out["d_cost"].reshape(n, 16)
    return out


def compose(codec, cur, pred, w, h, qps=None, qp=32, lam=368, cand_luma=T.CLASSES, cand_chroma=T.CLASSES, cand=None, class_bits=None):
    """the composition the call replaces: per candidate class the two existing device calls on the whole frame, then the rule in numpy"""
    n = T.n_regions(w, h)
    masks = T.effective_masks(n, cand_luma, cand_chroma, cand)
    bits = [0] * 16 if class_bits is None else list(class_bits) + [0] * (16 - len(class_bits))
    dc, dp, dk = dev(codec, cur), dev(codec, pred), codec.alloc(max(n, 16))
    d_qp = dev(codec, np.asarray(qps, np.uint8)) if qps is not None else None
    dz, dl, ds = codec.alloc(n * 2048), codec.alloc(n * 2048), codec.alloc(n * 16)
    out = {"d_class": np.zeros(n, np.uint8), "d_level": np.zeros((n, 1024), np.int16), "d_stat": np.zeros(n, R.STAT_DTYPE),
           "d_cost": np.full((n, 16), T.ALL_ONES, np.uint64)}
    best = [None] * n
    for k in T.CLASS_LIST:
        if not ((masks >> k) & 1).any():
            continue
        dk.upload(np.full(max(n, 16), k, np.uint8))
        codec.transform_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dk.ptr, dz.ptr)
        codec.rdo_quant_dev(codec.rdoq_params(dz.ptr, dl.ptr, dk.ptr, d_qp.ptr if d_qp else 0, 0, ds.ptr, n, qp, lam))
        sync_or_exit(codec, 0)
        level, stat = dl.download(np.int16, n * 1024).reshape(n, 1024), ds.download(np.uint8, 16 * n).view(R.STAT_DTYPE)
        for r in np.flatnonzero((masks >> k) & 1):
            j = int(stat["dist"][r]) + lam * (int(stat["bits"][r]) + bits[k])
            out["d_cost"][r, k] = np.uint64(j)
            if best[r] is None or j < best[r]:
                best[r], out["d_class"][r], out["d_level"][r], out["d_stat"][r] = j, k, level[r], stat[r]
    out["d_nnz"] = out["d_stat"]["n_nz"].astype(np.uint32)
    return out


def _same(got, want, regions=None):
    """every output the call was given equals `want` (on `regions` of the frame: want holds those regions only)"""
    for name in EXTENT:
        if got[name] is None:
            continue
        g = got[name] if regions is None else got[name][regions]
        bad = np.flatnonzero((g != want[name]).reshape(g.shape[0], -1).any(1))
        assert bad.size == 0, (name, bad[:8], g[bad[:2]], want[name][bad[:2]])


def _ref(oracle, cur, pred, w, h, regions, mats=None, **kw):
    cls, level, stat, cost = T.decide(oracle, cur, pred, w, h, regions=regions, mats=mats, **kw)
    return {"d_class": cls, "d_level": level, "d_nnz": stat["n_nz"].astype(np.uint32), "d_stat": stat, "d_cost": cost}


def _sample(w, h):
    """at most 18 regions, every q and the cut and outside regions among them: the python reference stays within a few seconds"""
    n = T.n_regions(w, h)
    return np.arange(n) if n <= 18 else np.arange(0, n, 2)


def _both_checks(codec, oracle, cur, pred, w, h, mats=None, **kw):
    kw.setdefault("qp", 32)
    kw.setdefault("lam", 368)
    got = decide(codec, cur, pred, w, h, **kw)
    _same(got, compose(codec, cur, pred, w, h, **kw))
    sel = _sample(w, h)
    _same(got, _ref(oracle, cur, pred, w, h, sel, mats, **kw), sel)
    assert int(got["d_class"].max()) <= 14
    return got


# ---- 1. all 13 candidates on every frame and both kinds of content ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["kinds", "mix"])
@pytest.mark.parametrize("w,h", FRAMES)
def test_all_candidates(codec, oracle, w, h, kind):
    cur, pred = frames(w, h, kind)
    got = _both_checks(codec, oracle, cur, pred, w, h)
    outside = _wholly_outside(w, h).ravel()
    assert outside.any() == ((w, h) != (64, 64))
    # a region wholly outside the frame: residual 0, no side bits, every J is 0 and the lowest class byte wins
    assert not got["d_class"][outside].any() and not got["d_level"][outside].any() and not got["d_cost"][outside][:, T.CLASS_LIST].any()
    assert np.all(got["d_cost"][:, [7, 11, 15]] == T.ALL_ONES)
    if kind == "kinds" and (w, h) == (144, 80):
        assert len(set(got["d_class"].tolist())) >= 4                        # the choice is not degenerate


# ---- 2. masks, qp bytes, lambda, side bits ------------------------------------------------------------------------------------------------
def test_two_candidate_masks(codec, oracle):
    w, h = 80, 48
    cur, pred = frames(w, h, "kinds")
    got = _both_checks(codec, oracle, cur, pred, w, h, cand_luma=(1 << 3) | (1 << 5), cand_chroma=(1 << 1) | (1 << 13))
    q = np.arange(T.n_regions(w, h)) % 6
    assert set(got["d_class"][q < 4].tolist()) <= {3, 5} and set(got["d_class"][q >= 4].tolist()) <= {1, 13}
    assert np.all((got["d_cost"] != T.ALL_ONES).sum(1) == 2)


@pytest.mark.parametrize("w,h", [(80, 48), (144, 80)])
def test_per_region_masks_as_an_encoder_sets_them(codec, oracle, w, h):
    """d_cand keeps N from straddling the frame edge on cut regions; 0 and bits outside 0x777F alone fall back to the scalar masks"""
    cur, pred = frames(w, h, "kinds")
    cand = T.encoder_masks(w, h)
    assert (cand != 0).any() and (cand == 0).any()
    cand = cand | np.where(np.arange(cand.size) % 2 == 1, 0x8880, 0).astype(np.uint16)      # garbage outside the valid bits
    got = _both_checks(codec, oracle, cur, pred, w, h, cand=cand, cand_luma=0x000F, cand_chroma=0x00F0 & T.CLASSES)
    own = cand & T.CLASSES
    assert np.all((own[own != 0] >> got["d_class"][own != 0]) & 1)
    q = np.arange(cand.size) % 6
    assert np.all(got["d_class"][(own == 0) & (q < 4)] < 4) and np.all(got["d_class"][(own == 0) & (q >= 4)] >> 2 == 1)


def test_qp_bytes_above_51_clamp(codec, oracle):
    w, h = 144, 80
    cur, pred = frames(w, h, "kinds")
    n = T.n_regions(w, h)
    qps = np.array([32, 22, 37, 27, 0, 51, 200, 30, 52, 255], np.uint8)[np.arange(n) % 10]
    got = _both_checks(codec, oracle, cur, pred, w, h, qps=qps, qp=99)        # the scalar qp is not looked at beside d_qp
    clamped = _both_checks(codec, oracle, cur, pred, w, h, qps=np.minimum(qps, 51), qp=0)
    for name in EXTENT:
        assert got[name].tobytes() == clamped[name].tobytes()


@pytest.mark.parametrize("lam", [0, 8192])
def test_lambda_extremes(codec, oracle, lam):
    w, h = 80, 48
    for kind in ("kinds", "mix"):
        cur, pred = frames(w, h, kind)
        got = _both_checks(codec, oracle, cur, pred, w, h, lam=lam, class_bits=[40000] * 16)
        if lam == 0:                                                         # J is the distortion alone
            cand = got["d_cost"] != T.ALL_ONES
            assert np.array_equal(got["d_cost"][np.arange(cand.shape[0]), got["d_class"]], got["d_stat"]["dist"])


def test_side_bits_flip_a_winner(codec, oracle):
    w, h = 64, 64
    cur, pred = frames(w, h, "kinds")
    free = _both_checks(codec, oracle, cur, pred, w, h)
    bits = [0] * 16
    for k in set(free["d_class"].tolist()):
        bits[k] = 65535                                                      # every former winner becomes dear
    paid = _both_checks(codec, oracle, cur, pred, w, h, class_bits=bits)
    moved = paid["d_class"] != free["d_class"]
    assert moved.any()
    # ... and the costs of the classes that stayed free did not move
    stay = [k for k in T.CLASS_LIST if bits[k] == 0]
    assert np.array_equal(paid["d_cost"][:, stay], free["d_cost"][:, stay])


def test_cur_equals_pred_and_ties(codec, oracle):
    """residual 0 everywhere: every J_k = lambda * class_bits[k]; equal side bits: the lowest set bit wins; one cheaper class wins"""
    w, h = 80, 48
    cur, _ = frames(w, h, "mix")
    got = decide(codec, cur, cur, w, h, cand_luma=0x7770, cand_chroma=0x0408, class_bits=[48] * 16, same_frame=True)
    q = np.arange(T.n_regions(w, h)) % 6
    assert np.all(got["d_class"][q < 4] == 4) and np.all(got["d_class"][q >= 4] == 3) and not got["d_level"].any()
    assert np.all(got["d_cost"][q >= 4][:, [3, 10]] == 368 * 48)
    bits = [48] * 16
    bits[9] = 47
    got = decide(codec, cur, cur, w, h, class_bits=bits, same_frame=True)
    assert np.all(got["d_class"] == 9) and np.all(got["d_cost"][:, 9] == 368 * 47) and not got["d_stat"]["bits"].any()


@pytest.fixture()
def fresh():
    """a context of its own: installed matrices are per context"""
    c = x266_amd.Codec(0)
    yield c
    c.close()


def test_installed_preset_dct8(fresh, oracle):
    w, h = 80, 48
    cur, pred = frames(w, h, "kinds")
    fresh.use_transform_preset(x266_amd._lib.PRESET_VTM_DCT8)
    try:
        got = _both_checks(fresh, oracle, cur, pred, w, h, mats=_slot_mats(fresh))
    finally:
        fresh.use_transform_preset(0)
    plain = decide(fresh, cur, pred, w, h)
    assert plain["d_cost"].tobytes() != got["d_cost"].tobytes()              # the installed matrices were the ones used


# ---- 3. optional outputs, streams, a graph -------------------------------------------------------------------------------------------------
def test_optional_outputs_one_at_a_time(codec, oracle):
    w, h = 144, 80
    cur, pred = frames(w, h, "mix")
    full = decide(codec, cur, pred, w, h)
    for name in ("d_nnz", "d_stat", "d_cost"):
        part = decide(codec, cur, pred, w, h, without=(name,))
        assert part[name] is None
        for other in EXTENT:
            assert other == name or part[other].tobytes() == full[other].tobytes(), (name, other)
    none = decide(codec, cur, pred, w, h, without=("d_nnz", "d_stat", "d_cost"))
    assert none["d_class"].tobytes() == full["d_class"].tobytes() and none["d_level"].tobytes() == full["d_level"].tobytes()


def test_two_streams_give_identical_bytes(codec):
    w, h = 144, 80
    cur, pred = frames(w, h, "mix")
    streams = [codec.stream_create(), codec.stream_create()]
    try:
        runs = [decide(codec, cur, pred, w, h, stream=st) for st in streams]
    finally:
        for st in streams:
            codec.stream_destroy(st)
    for name in EXTENT:
        assert runs[0][name].tobytes() == runs[1][name].tobytes(), name


def test_in_a_graph(codec):
    w, h = 144, 80
    n = T.n_regions(w, h)
    data = [frames(w, h, "kinds"), frames(w, h, "mix")]
    want = [decide(codec, cur, pred, w, h) for cur, pred in data]
    dc, dp = codec.alloc(w * h * 2), codec.alloc(w * h * 2)
    outs = {name: codec.alloc(max(each * n, 16)) for name, each in EXTENT.items()}
    p = codec.tdecide_params(dc.ptr, dp.ptr, 0, 0, outs["d_class"].ptr, outs["d_level"].ptr, outs["d_nnz"].ptr, outs["d_stat"].ptr, outs["d_cost"].ptr,
                             w, h, 32, 368)
    st = codec.stream_create()
    try:
        dc.upload(data[0][0])
        dp.upload(data[0][1])
        codec.graph_begin(st)
        codec.transform_decide_dev(p, stream=st)
        graph = codec.graph_end(st)
        try:
            for i in (1, 0):                                                 # replayed twice, on other data than it was captured with
                dc.upload(data[i][0])
                dp.upload(data[i][1])
                outs["d_level"].upload(np.full(n * 1024, 0x5A5A, np.int16))
                codec.graph_launch(graph, st)
                sync_or_exit(codec, 0, st)
                for name, each in EXTENT.items():
                    assert outs[name].download(np.uint8, each * n).tobytes() == want[i][name].tobytes(), (i, name)
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 4. the chain behind the call -------------------------------------------------------------------------------------------------------------
def test_chain(codec, oracle):
    """decide -> xQuantRegionsGpu(1, d_class) -> xTransformCtuToTilesDev(d_class) -> xLevelsPackGpu(d_class) -> xLevelsUnpackGpu; xLevelsBitsGpu
    on the levels reproduces the winner's bits"""
    w, h, qp, lam = 128, 64, 32, 368
    n = T.n_regions(w, h)
    cur, pred = frames(w, h, "kinds")
    base = _tiles_mix(w, h, 0x7E00)
    dc, dp, dr = dev(codec, cur), dev(codec, pred), dev(codec, base)
    outs = {name: codec.alloc(max(each * n, 16)) for name, each in EXTENT.items()}
    dz = codec.alloc(n * 2048)
    codec.transform_decide_dev(codec.tdecide_params(dc.ptr, dp.ptr, 0, 0, outs["d_class"].ptr, outs["d_level"].ptr, outs["d_nnz"].ptr, outs["d_stat"].ptr,
                                                    outs["d_cost"].ptr, w, h, qp, lam))
    codec.quant_regions_dev(1, outs["d_level"].ptr, dz.ptr, n, outs["d_class"].ptr, 0, qp, 0)
    codec.transform_ctu_to_tiles_dev(dz.ptr, outs["d_class"].ptr, dp.ptr, w, h, dr.ptr)
    sync_or_exit(codec, 0)
    cls, level = outs["d_class"].download(np.uint8, n), outs["d_level"].download(np.int16, n * 1024).reshape(n, 1024)
    nnz, stat = outs["d_nnz"].download(np.uint32, n), outs["d_stat"].download(np.uint8, 16 * n).view(R.STAT_DTYPE)
    want = _ref(oracle, cur, pred, w, h, np.arange(n), qp=qp, lam=lam)
    assert np.array_equal(cls, want["d_class"]) and np.array_equal(level, want["d_level"]) and np.array_equal(stat, want["d_stat"])
    assert len(set(cls.tolist())) >= 3 and level.any()
    coef = Q.quant_regions(level, True, cls, None, qp)
    assert np.array_equal(dr.download(np.uint8, w * h * 2), ref_inverse(oracle, coef, cls, pred, w, h, base))
    rec, words, total = codec.levels_pack(level, cls, nnz)
    want_rec, want_words, want_total = LR.pack(level, cls, nnz)
    assert np.array_equal(rec, want_rec) and np.array_equal(words, want_words) and total.tolist() == want_total.tolist()
    back, back_nnz = codec.levels_unpack(rec, words, n, cls)
    assert np.array_equal(back, level) and np.array_equal(back_nnz, nnz)
    bits = codec.levels_bits(level, cls, nnz).view(R.STAT_DTYPE)
    assert np.array_equal(bits["bits"], stat["bits"]) and np.array_equal(bits["n_nz"], stat["n_nz"])


def test_numpy_convenience(codec, oracle):
    w, h = 64, 64
    cur, pred = frames(w, h, "kinds")
    cls, level, nnz, stat, cost = codec.transform_decide(cur, pred, w, h, qp=32, lam=368)
    want = _ref(oracle, cur, pred, w, h, np.arange(6), qp=32, lam=368)
    _same({"d_class": cls, "d_level": level, "d_nnz": nnz, "d_stat": stat.view(R.STAT_DTYPE), "d_cost": cost}, want)
    assert x266_amd.TDECIDE_CLASSES == T.CLASSES


# ---- 5. refusals through the ABI ---------------------------------------------------------------------------------------------------------------
def test_argument_errors(codec):
    """every rule once: X266HIP_EINVAL, the call named in the error text, nothing launched, the sentinel-filled outputs untouched"""
    L, ctx = codec.L, codec.ctx
    name = "xTransformDecideCtuTilesGpu"
    M = 1 << 20
    buf = codec.alloc(10 * M)
    fill = np.random.RandomState(11).randint(1, 255, 10 * M).astype(np.uint8)
    buf.upload(fill)
    w, h = 144, 80
    n = T.n_regions(w, h)
    fields = list(PTRS)
    good = {f: buf.ptr + (i + 1) * M for i, f in enumerate(fields)}
    good.update(width=w, height=h, qp=30, lam=368)
    extent = dict(d_cur=w * h * 2, d_pred=w * h * 2, d_qp=n, d_cand=2 * n, d_class=n, d_level=2048 * n, d_nnz=4 * n, d_stat=16 * n, d_cost=128 * n)

    def refused(**change):
        p = codec.tdecide_params(**dict(good, **change))
        assert L.xTransformDecideCtuTilesGpu(ctx, ctypes.byref(p), None) == EINVAL, change
        assert name.encode() in L.xHipLastError(ctx), change

    assert L.xTransformDecideCtuTilesGpu(ctx, None, None) == EINVAL and name.encode() in L.xHipLastError(ctx)     # NULL p
    assert L.xTransformDecideCtuTilesGpu(None, ctypes.byref(codec.tdecide_params(**good)), None) == EINVAL
    for f in ("d_cur", "d_pred", "d_class", "d_level"):
        refused(**{f: 0})
    for f, half in (("d_cur", 8), ("d_pred", 8), ("d_cand", 1), ("d_level", 8), ("d_nnz", 2), ("d_stat", 4), ("d_cost", 4)):
        refused(**{f: good[f] + half})
    for f in fields:
        refused(**{f: 2 ** 64 - PTRS[f]})                                     # aligned, and the extent does not fit behind it
    for change in (dict(width=0), dict(width=-16), dict(width=72), dict(height=0), dict(height=88), dict(width=2 ** 31 - 16, height=2 ** 31 - 16, d_level=16)):
        refused(**change)
    for change in (dict(lam=-1), dict(lam=8193), dict(d_qp=0, qp=-1), dict(d_qp=0, qp=52)):
        refused(**change)
    for change in (dict(cand_luma=0), dict(cand_chroma=0), dict(cand_luma=0x0080), dict(cand_luma=0x0808), dict(cand_chroma=0x8001), dict(cand_chroma=0x0800)):
        refused(**change)
    for o in EXTENT:                                                          # an output onto any other buffer: its first and its last bytes
        for other in fields:
            if other != o:
                refused(**{o: good[other]})
                refused(**{o: good[other] + (extent[other] - 1) // PTRS[o] * PTRS[o]})
    sync_or_exit(codec, 0)
    assert np.array_equal(buf.download(np.uint8, 10 * M), fill)             # nothing was launched
    # the edges of what is accepted: d_cur == d_pred, a qp out of range beside d_qp, every optional pointer NULL
    for change in (dict(d_pred=good["d_cur"]), dict(qp=99), dict(d_qp=0, d_cand=0, d_nnz=0, d_stat=0, d_cost=0)):
        rc = L.xTransformDecideCtuTilesGpu(ctx, ctypes.byref(codec.tdecide_params(**dict(good, **change))), None)
        sync_or_exit(codec, rc)
        assert rc == 0, (change, L.xHipLastError(ctx))
