"""Intra coding of tiled frames: xIntra32RefsFromTilesGpu / xIntra32CodeFrameGpu against the reference statement of
tests/_intra_frame_ref.py (checked on the CPU by tests/test_intra_frame_ref.py).  Every comparison is bit-exact; every test but the
export test is marked gpu."""
import ctypes
import subprocess

import numpy as np
import pytest

import _intra_frame_ref as R
import _quant_ref as Q
import x266_amd
from _dev import EINVAL, arena_slots, dev, displacements, noise, run, sync_or_exit, tile_written
from _util import splitmix64

gpu = pytest.mark.gpu
NAMES = ("xIntra32RefsFromTilesGpu", "xIntra32CodeFrameGpu")


# ---- the export test (CPU) ------------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_two_calls():
    x266_amd.build_library()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode().split()
    lib = x266_amd.load_library()
    for name in NAMES:
        assert name in exported, name
        assert getattr(lib, name).argtypes, name                            # bound by _lib.py, with its argument types
    for method in ("intra32_refs_from_tiles_dev", "intra32_refs_from_tiles", "intra32_code_frame_dev", "intra32_code_frame"):
        assert callable(getattr(x266_amd.Codec, method)), method


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
class Frame:
    """the device buffers of one xIntra32CodeFrameGpu call over a random pre-fill, and what they hold afterwards"""

    def __init__(self, codec, cur, w, h, seed=700):
        self.codec, self.w, self.h, self.n = codec, w, h, codec.ctu_count(w, h)
        self.cur, self.base = np.ascontiguousarray(cur, np.uint8), noise(w * h * 2, seed)
        self.fill = {"level": noise(self.n * 12288, seed + 1), "nnz": noise(self.n * 24, seed + 2), "mode": noise(self.n * 6, seed + 3)}
        self.d_cur = dev(codec, self.cur)
        self.d_recon, self.d_level = codec.alloc(w * h * 2), codec.alloc(self.n * 12288)
        self.d_nnz, self.d_mode = codec.alloc(max(self.n * 24, 16)), codec.alloc(max(self.n * 6, 16))
        self.reset()

    def reset(self):
        self.d_recon.upload(self.base)
        self.d_level.upload(self.fill["level"])
        self.d_nnz.upload(self.fill["nnz"])
        self.d_mode.upload(self.fill["mode"])

    def enqueue(self, qps=0, qp=22, rounding=171, mode_in=0, nnz=True, stream=0):
        self.codec.intra32_code_frame_dev(self.d_cur.ptr, self.w, self.h, qps, qp, rounding, mode_in, self.d_level.ptr, self.d_nnz.ptr if nnz else 0,
                                          self.d_mode.ptr, self.d_recon.ptr, stream=stream)

    def code(self, **kw):
        self.reset()
        run(self.codec, self.enqueue, **kw)
        return self.results()

    def results(self):
        n = self.n
        return (self.d_level.download(np.int16, n * 6144).reshape(n, 6, 1024), self.d_nnz.download(np.uint32, n * 6).reshape(n, 6),
                self.d_mode.download(np.uint8, n * 6).reshape(n, 6), self.d_recon.download(np.uint8, self.w * self.h * 2))

    def check(self, oracle, got, want, what, nnz=True):
        level, cnt, mode, recon = got
        assert np.array_equal(mode, want.modes), what
        assert np.array_equal(level, want.levels), what
        if nnz:
            assert np.array_equal(cnt, want.nnz), what
        else:
            assert np.array_equal(cnt.view(np.uint8).ravel(), self.fill["nnz"]), what
        assert np.array_equal(recon, want.recon_tiles(oracle, self.base)), what   # m_I and nothing else keeps the pre-fill
        assert np.array_equal(self.d_cur.download(np.uint8, self.cur.size), self.cur), what


# ---- 1. the gather --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", R.SIZES)
def test_gather_against_the_statement(codec, oracle, w, h):
    planes = R.case("noise", w, h, seed=w + h)
    t = R.tiles(oracle, planes, 50 + w)
    d_t = dev(codec, t)
    for comp in range(3):
        want = R.refs_from_planes(planes, w, h, comp)
        d_refs = dev(codec, noise(want.size, 51 + comp))
        run(codec, codec.intra32_refs_from_tiles_dev, d_t.ptr, w, h, comp, d_refs.ptr)
        got = d_refs.download(np.uint8, want.size).reshape(want.shape)
        assert not got[:, 129:].any(), comp                                 # the reserved bytes are written as 0
        assert np.array_equal(got, want), comp
        assert np.array_equal(codec.intra32_refs_from_tiles(t, w, h, comp, base=noise(want.size, 3)), want), comp
    assert np.array_equal(d_t.download(np.uint8, t.size), t)


# ---- 2. the closed loop ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("w,h", R.SIZES)
def test_code_frame_against_the_statement(codec, oracle, w, h, kind):
    planes = R.case(kind, w, h)
    f = Frame(codec, R.tiles(oracle, planes, 60 + h), w, h)
    for qp in (0, 22, 37, 51):
        for rounding in (171, 256):
            f.check(oracle, f.code(qp=qp, rounding=rounding), R.coded(oracle, kind, w, h, qp, rounding), (qp, rounding))
    qps = (splitmix64(61 + w, 0, 6 * f.n) % np.uint64(70)).astype(np.uint8)    # bytes above 51 are clamped
    qps[0] = 69
    want = R.code_frame(oracle, planes, w, h, qps, 0, 256)
    d_qps = dev(codec, qps)
    f.check(oracle, f.code(qps=d_qps.ptr, qp=99, rounding=256), want, "d_qp")      # the scalar qp is not looked at
    f.check(oracle, f.code(qps=d_qps.ptr, qp=0, rounding=256, nnz=False), want, "d_nnz NULL", nnz=False)
    assert np.array_equal(d_qps.download(np.uint8, qps.size), qps)
    # the host-array form is the same call
    level, cnt, mode, recon = codec.intra32_code_frame(f.cur, w, h, qps=qps, rounding=256, base=f.base)
    assert np.array_equal(level, want.levels) and np.array_equal(cnt, want.nnz) and np.array_equal(mode, want.modes)
    assert np.array_equal(recon, want.recon_tiles(oracle, f.base))


# ---- 3. modes given -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", R.SIZES)
def test_modes_given(codec, oracle, w, h):
    planes = R.case("oriented", w, h)
    f = Frame(codec, R.tiles(oracle, planes, 62 + h), w, h)
    decided = R.coded(oracle, "oriented", w, h, 22, 171)
    given = decided.modes.copy()
    given[:, 5] = 35 + (np.arange(f.n) % 200)                               # entry 5 is ignored
    d_in = dev(codec, given)
    f.check(oracle, f.code(mode_in=d_in.ptr), decided, "decided modes")
    assert np.array_equal(d_in.download(np.uint8, given.size), given.ravel())
    rnd = (splitmix64(63 + w, 0, 6 * f.n) % np.uint64(35)).astype(np.uint8).reshape(f.n, 6)
    want = R.code_frame(oracle, planes, w, h, None, 37, 256, modes_in=rnd)
    assert np.array_equal(want.modes[:, :5], rnd[:, :5]) and np.array_equal(want.modes[:, 5], rnd[:, 4])
    d_in.upload(rnd)
    f.check(oracle, f.code(qp=37, rounding=256, mode_in=d_in.ptr), want, "random modes")
    # in place: d_mode == d_mode_in
    f.reset()
    f.d_mode.upload(rnd)
    run(codec, f.enqueue, qp=37, rounding=256, mode_in=f.d_mode.ptr)
    f.check(oracle, f.results(), want, "in place")


# ---- 4. the same answer from the calls the library already had ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ("oriented", "extreme"))
def test_cross_check_on_the_device(codec, oracle, kind):
    """the sets of the call's own d_recon (all three components) -> xIntra32PredictDev with d_mode -> the predictions as a tiled frame ->
    xDct32CodeCtuTilesGpu(cur, that frame, the same qp arguments): the same levels, counts and reconstruction"""
    w, h = 192, 128
    f = Frame(codec, R.tiles(oracle, R.case(kind, w, h), 64), w, h)
    qps = (splitmix64(65, 0, 6 * f.n) % np.uint64(56)).astype(np.uint8)
    d_qps = dev(codec, qps)
    level, cnt, mode, recon = f.code(qps=d_qps.ptr, qp=0, rounding=171)
    n = f.n
    pred = np.zeros((n, 6, 1024), np.uint8)
    for comp in range(3):
        sets = n * (4 if comp == 0 else 1)
        d_refs, d_modes, d_pred = codec.alloc(sets * 144), dev(codec, mode[:, :4] if comp == 0 else mode[:, 3 + comp]), codec.alloc(sets * 1024)
        run(codec, codec.intra32_refs_from_tiles_dev, f.d_recon.ptr, w, h, comp, d_refs.ptr)
        run(codec, codec.intra32_predict_dev, d_refs.ptr, d_modes.ptr, 0, d_pred.ptr, sets)
        p = d_pred.download(np.uint8, sets * 1024)
        if comp == 0:
            pred[:, :4] = p.reshape(n, 4, 1024)
        else:
            pred[:, 3 + comp] = p.reshape(n, 1024)
    d_predframe = dev(codec, oracle.conv_input_fmt(*Q._planes_of_regions(pred.reshape(-1, 6, 32, 32), w, h)))
    d_l, d_n, d_r = codec.alloc(n * 12288), codec.alloc(n * 24), dev(codec, f.base)
    run(codec, codec.dct32_code_ctu_tiles_dev, f.d_cur.ptr, d_predframe.ptr, w, h, d_qps.ptr, 0, 171, d_l.ptr, d_n.ptr, d_r.ptr)
    assert np.array_equal(d_l.download(np.int16, n * 6144).reshape(n, 6, 1024), level)
    assert np.array_equal(d_n.download(np.uint32, n * 6).reshape(n, 6), cnt)
    assert np.array_equal(d_r.download(np.uint8, w * h * 2), recon)


# ---- 5. captured into a graph, and on a stream of its own -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("given", (False, True))
def test_graph_replay_and_created_stream(codec, oracle, given):
    w, h = 192, 128
    f = Frame(codec, R.tiles(oracle, R.case("oriented", w, h), 66), w, h)
    eager = f.code(qp=22, rounding=171)
    f.check(oracle, eager, R.coded(oracle, "oriented", w, h, 22, 171), "eager")
    d_in = dev(codec, eager[2])
    kw = dict(qp=22, rounding=171, mode_in=d_in.ptr if given else 0)
    st = codec.stream_create()
    try:
        kw["stream"] = st
        for x, y in zip(eager, f.code(**kw)):
            assert np.array_equal(x, y)                                     # a created stream: the default stream's bits
        codec.graph_begin(st)
        f.enqueue(**kw)
        graph = codec.graph_end(st)
        try:
            for _ in range(2):
                f.reset()
                codec.graph_launch(graph, st)
                sync_or_exit(codec, 0, st)
                for x, y in zip(eager, f.results()):
                    assert np.array_equal(x, y)
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 6. minimum alignment, inside guard bands ---------------------------------------------------------------------------------------------
AW, AH = 128, 128
PTRS = {"xIntra32RefsFromTilesGpu": {"d_frame": 16, "d_refs": 16},
        "xIntra32CodeFrameGpu": {"d_cur": 16, "d_qp": 1, "d_mode_in": 1, "d_level": 16, "d_nnz": 4, "d_mode": 1, "d_recon": 16}}
OUTPUTS = {"xIntra32RefsFromTilesGpu": ("d_refs",), "xIntra32CodeFrameGpu": ("d_level", "d_nnz", "d_mode", "d_recon")}


@pytest.fixture(scope="module")
def arena_case(oracle):
    planes = R.case("oriented", AW, AH)
    n = (AW // 64) * (AH // 64)
    qps = (splitmix64(67, 0, 6 * n) % np.uint64(60)).astype(np.uint8)
    modes = (splitmix64(68, 0, 6 * n) % np.uint64(35)).astype(np.uint8)
    want = R.code_frame(oracle, planes, AW, AH, qps, 0, 171, modes_in=modes)
    cur = R.tiles(oracle, planes, 69)
    return {"d_frame": cur, "d_cur": cur, "d_qp": qps, "d_mode_in": modes, "d_refs": R.refs_from_planes(planes, AW, AH, 0).ravel(),
            "d_level": want.levels.ravel(), "d_nnz": want.nnz.ravel(), "d_mode": want.modes.ravel(), "coded": want, "oracle": oracle}


def _arena(codec, arena_case, name, disp, guard_seed):
    return arena_slots(codec, PTRS[name], OUTPUTS[name], arena_case, disp, guard_seed, written={"d_recon": tile_written(AW * AH // 256, "both")},
                       sizes={"d_recon": AW * AH * 2})


def _call_arena(codec, name, s):
    L = codec.L
    if name == "xIntra32RefsFromTilesGpu":
        rc = L.xIntra32RefsFromTilesGpu(codec.ctx, s["d_frame"].ptr, AW, AH, 0, s["d_refs"].ptr, None)
    else:
        rc = L.xIntra32CodeFrameGpu(codec.ctx, s["d_cur"].ptr, AW, AH, s["d_qp"].ptr, 0, 171, s["d_mode_in"].ptr, s["d_level"].ptr, s["d_nnz"].ptr,
                                    s["d_mode"].ptr, s["d_recon"].ptr, None)
    sync_or_exit(codec, rc)
    return rc


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_minimum_alignment(codec, arena_case, name):
    results = []
    for guard_seed in (31, 51):
        a, s = _arena(codec, arena_case, name, displacements(PTRS[name]), guard_seed)
        assert _call_arena(codec, name, s) == 0, codec.L.xHipLastError(codec.ctx)
        got = a.check()                                                     # guards, m_I of d_recon, inputs
        for p in OUTPUTS[name]:
            if p == "d_recon":
                want = arena_case["coded"].recon_tiles(arena_case["oracle"], s[p].image[s[p].start:][:AW * AH * 2])
            else:
                want = np.ascontiguousarray(arena_case[p]).view(np.uint8)
            assert np.array_equal(got[p], want), p
        results.append([got[p] for p in OUTPUTS[name]])
    for x, y in zip(*results):
        assert np.array_equal(x, y)                                         # the garbage around the inputs reaches no output byte


@gpu
@pytest.mark.parametrize("name,ptr", [(n, p) for n in NAMES for p in PTRS[n] if PTRS[n][p] > 1])
def test_half_alignment_is_rejected(codec, arena_case, name, ptr):
    a, s = _arena(codec, arena_case, name, displacements(PTRS[name], halved=ptr), 33)
    assert _call_arena(codec, name, s) == EINVAL
    assert name.encode() in codec.L.xHipLastError(codec.ctx)
    a.check_untouched()


# ---- 7. arguments ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_argument_errors(codec):
    """one refused call per rule, for both calls; a refused call launches nothing and names itself"""
    L, ctx = codec.L, codec.ctx
    buf = codec.alloc(8 << 20)
    fill = noise(8 << 20, 95)
    buf.upload(fill)
    cur, rec, lvl = buf.ptr + (1 << 20), buf.ptr + (2 << 20), buf.ptr + (3 << 20)   # 64x64: tile arrays of 8 KiB, 12 KiB of levels
    nnz, mode, min_, qps, refs = (buf.ptr + (4 << 20) + 4096 * i for i in range(5))  # 24, 6, 6, 6 bytes; 4 sets of 144
    top, top16, top4, top1 = 2 ** 64 - 4096, 2 ** 64 - 16, 2 ** 64 - 4, 2 ** 64 - 1   # aligned, and nothing of theirs fits behind them

    def refused(name, *args):
        assert getattr(L, name)(ctx, *args, None) == EINVAL, (name, args)
        assert name.encode() in L.xHipLastError(ctx), (name, args)

    assert L.xIntra32RefsFromTilesGpu(None, cur, 64, 64, 0, refs, None) == EINVAL
    assert L.xIntra32CodeFrameGpu(None, cur, 64, 64, None, 22, 171, None, lvl, nnz, mode, rec, None) == EINVAL
    for a in ((None, 64, 64, 0, refs), (cur, 64, 64, 0, None), (cur + 8, 64, 64, 0, refs), (cur, 64, 64, 0, refs + 8),
              (cur, 0, 64, 0, refs), (cur, 64, -64, 0, refs), (cur, 96, 64, 0, refs), (cur, 64, 80, 0, refs), (cur, 64, 64, -1, refs), (cur, 64, 64, 3, refs),
              (top, 64, 64, 0, refs), (cur, 64, 64, 0, top16), (cur, 64, 64, 2, top16),
              (cur, 64, 64, 0, cur), (cur, 64, 64, 0, cur + 8176), (cur, 64, 64, 1, cur - 128), (cur, 64, 64, 0, cur - 560)):
        refused("xIntra32RefsFromTilesGpu", *a)

    def code(cur=cur, w=64, h=64, qps=None, qp=22, rounding=171, min_=None, lvl=lvl, nnz=nnz, mode=mode, rec=rec):
        return (cur, w, h, qps, qp, rounding, min_, lvl, nnz, mode, rec)

    for a in (code(cur=None), code(lvl=None), code(mode=None), code(rec=None),
              code(cur=cur + 8), code(lvl=lvl + 8), code(rec=rec + 8), code(nnz=nnz + 2),
              code(w=0), code(h=-64), code(w=32), code(w=96), code(h=80),
              code(qp=52), code(qp=-1), code(rounding=-1), code(rounding=512), code(qps=qps, rounding=512),
              code(cur=top), code(rec=top), code(lvl=top), code(nnz=top4), code(mode=top1), code(qps=top1), code(min_=top1),
              code(rec=cur), code(rec=cur + 4096), code(rec=cur - 8176),                       # d_recon against d_cur, d_recon == d_cur included
              code(lvl=cur + 16), code(lvl=rec - 12272), code(nnz=cur + 8188), code(nnz=rec), code(nnz=lvl + 12284), code(mode=cur), code(mode=rec + 8191),
              code(mode=lvl + 100), code(mode=nnz + 23), code(qps=qps, mode=qps + 5), code(qps=rec + 17), code(qps=lvl - 5), code(qps=nnz - 5),
              code(min_=rec), code(min_=lvl + 12287), code(min_=nnz + 23), code(min_=mode + 1), code(min_=mode - 5)):   # only d_mode_in == d_mode may overlap
        refused("xIntra32CodeFrameGpu", *a)
    assert np.array_equal(buf.download(np.uint8, 8 << 20), fill)            # nothing was launched
    # the edges of what is accepted: the qp and the rounding at both ends, qp out of range under d_qp, every optional pointer NULL or given
    buf.upload(np.zeros(8 << 20, np.uint8))                                 # mode bytes above 34 are undefined input
    for rc in (L.xIntra32RefsFromTilesGpu(ctx, cur, 64, 64, 2, refs, None),
               L.xIntra32CodeFrameGpu(ctx, *code(qp=0, rounding=0, nnz=None), None), L.xIntra32CodeFrameGpu(ctx, *code(qp=51, rounding=511), None),
               L.xIntra32CodeFrameGpu(ctx, *code(qps=qps, qp=99, min_=min_), None), L.xIntra32CodeFrameGpu(ctx, *code(min_=mode), None)):
        sync_or_exit(codec, rc)
        assert rc == 0, L.xHipLastError(ctx)
