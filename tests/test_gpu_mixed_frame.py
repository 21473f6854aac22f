"""Mixed inter / intra coding of a frame: xDct32CodeMixedFrameGpu against the reference statement of tests/_mixed_frame_ref.py (checked on
the CPU by tests/test_mixed_frame_ref.py), against the two coding calls it must agree with, and through the deblocking call that reads
its kinds.  Every comparison is bit-exact; every test here is marked gpu (the export and binding tests are in
tests/test_mixed_arg_rules.py)."""
import numpy as np
import pytest

import _deblock_ref as D
import _intra_frame_ref as R
import _mixed_frame_ref as M
import _quant_ref as Q
from _dev import EINVAL, arena_slots, dev, displacements, noise, run, sync_or_exit, tile_written
from _util import me_frames, splitmix64

gpu = pytest.mark.gpu
CALL = "xDct32CodeMixedFrameGpu"
QP, ROUNDING = 22, 171


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def _qps(n, seed=61):
    q = (splitmix64(seed, 0, 6 * n) % np.uint64(70)).astype(np.uint8)       # bytes above 51 are clamped
    q[0] = 69
    return q


def _modes(n, seed=63):
    return (splitmix64(seed, 0, 6 * n) % np.uint64(35)).astype(np.uint8).reshape(n, 6)


class Frame:
    """the device buffers of one call over a random pre-fill, and what they hold afterwards"""
    OUT = (("level", 12288), ("nnz", 24), ("kind", 6), ("mode", 6), ("cost", 48))

    def __init__(self, codec, oracle, cur, pred, w, h, seed=700):
        self.codec, self.oracle, self.w, self.h, self.n = codec, oracle, w, h, codec.ctu_count(w, h)
        self.cur_planes, self.pred_planes = cur, pred
        self.cur, self.pred, self.base = R.tiles(oracle, cur, seed + 10), R.tiles(oracle, pred, seed + 11), noise(w * h * 2, seed)
        self.fill = {name: noise(self.n * per, seed + 1 + i) for i, (name, per) in enumerate(self.OUT)}
        self.d_cur, self.d_pred, self.d_recon = dev(codec, self.cur), dev(codec, self.pred), codec.alloc(w * h * 2)
        self.d = {name: codec.alloc(max(self.n * per, 16)) for name, per in self.OUT}
        self.reset()

    def reset(self):
        self.d_recon.upload(self.base)
        self.d_pred.upload(self.pred)
        for name, _ in self.OUT:
            self.d[name].upload(self.fill[name])

    def params(self, qps=0, qp=QP, rounding=ROUNDING, penalty=0, kind_in=0, mode_in=0, nnz=True, cost=True, recon=None, kind=None, mode=None):
        return self.codec.mixed_params(self.w, self.h, qp, rounding, penalty, d_cur=self.d_cur.ptr, d_pred=self.d_pred.ptr, d_qp=qps, d_kind_in=kind_in,
                                       d_mode_in=mode_in, d_level=self.d["level"].ptr, d_nnz=self.d["nnz"].ptr if nnz else 0,
                                       d_kind=kind or self.d["kind"].ptr, d_mode=mode or self.d["mode"].ptr, d_cost=self.d["cost"].ptr if cost else 0,
                                       d_recon=recon or self.d_recon.ptr)

    def enqueue(self, stream=0, **kw):
        self.codec.dct32_code_mixed_frame_dev(self.params(**kw), stream=stream)

    def code(self, **kw):
        self.reset()
        run(self.codec, self.enqueue, **kw)
        return self.results()

    def results(self, recon=None):
        n, dt = self.n, {"level": np.int16, "nnz": np.uint32, "kind": np.uint8, "mode": np.uint8, "cost": np.uint32}
        got = {name: self.d[name].download(dt[name], n * per // np.dtype(dt[name]).itemsize) for name, per in self.OUT}
        got["recon"] = (recon or self.d_recon).download(np.uint8, self.w * self.h * 2)
        return got

    def want(self, **kw):
        return M.code_frame(self.oracle, self.cur_planes, self.pred_planes, self.w, self.h, **kw)

    def check(self, got, want, what, nnz=True, cost=True, base=None, pred_kept=True):
        n = self.n
        assert np.array_equal(got["kind"].reshape(n, 6), want.kinds), what
        assert np.array_equal(got["mode"].reshape(n, 6), want.modes), what
        assert np.array_equal(got["level"].reshape(n, 6, 1024), want.levels), what
        for name, on, ref in (("nnz", nnz, want.nnz), ("cost", cost, want.costs)):
            if on:
                assert np.array_equal(got[name].reshape(ref.shape), ref), (what, name)
            else:
                assert np.array_equal(got[name].view(np.uint8), self.fill[name]), (what, name)
        assert np.array_equal(got["recon"], want.recon_tiles(self.oracle, self.base if base is None else base)), what   # m_I keeps the pre-fill
        assert np.array_equal(self.d_cur.download(np.uint8, self.cur.size), self.cur), what
        if pred_kept:
            assert np.array_equal(self.d_pred.download(np.uint8, self.pred.size), self.pred), what


def _kind_inputs(n):
    return (("NULL", None), ("all 2", np.full((n, 6), 2, np.uint8)), ("all 0", np.zeros((n, 6), np.uint8)), ("all 1", np.ones((n, 6), np.uint8)),
            ("mixed", M.kinds_mixed(n)))


# ---- 1. against the statement ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("flip", (0, 1))
@pytest.mark.parametrize("w,h", R.SIZES)
def test_against_the_statement(codec, oracle, w, h, flip):
    cur, pred = M.pred_planes(w, h, flip)
    f = Frame(codec, oracle, cur, pred, w, h, 600 + w + flip)
    n = f.n
    qps, modes = _qps(n, 61 + w), _modes(n, 63 + h)
    d_qps, d_modes = dev(codec, qps), dev(codec, modes)
    for penalty in (0, 4096):
        for name, kinds in _kind_inputs(n):
            d_kinds = None if kinds is None else dev(codec, kinds)
            kp = d_kinds.ptr if d_kinds else 0
            # the scalar qp, the call chooses the modes (the statement of these is shared with the CPU tests where they have it)
            want = M.coded(oracle, w, h, flip, penalty, None) if kinds is None else f.want(qp=QP, rounding=ROUNDING, penalty=penalty, kinds_in=kinds)
            f.check(f.code(penalty=penalty, kind_in=kp), want, (penalty, name, "scalar qp"))
            # d_qp (the scalar qp is not looked at), the modes given
            want = f.want(qps=qps, qp=0, rounding=256, penalty=penalty, kinds_in=kinds, modes_in=modes)
            f.check(f.code(qps=d_qps.ptr, qp=99, rounding=256, penalty=penalty, kind_in=kp, mode_in=d_modes.ptr), want, (penalty, name, "d_qp, modes given"))
            if d_kinds:
                assert np.array_equal(d_kinds.download(np.uint8, 6 * n), kinds.ravel())
    kinds = M.kinds_mixed(n)
    d_kinds = dev(codec, kinds)
    f.check(f.code(qps=d_qps.ptr, kind_in=d_kinds.ptr, penalty=100), f.want(qps=qps, rounding=ROUNDING, penalty=100, kinds_in=kinds), "d_qp, modes chosen")
    f.check(f.code(mode_in=d_modes.ptr, kind_in=d_kinds.ptr, qp=37), f.want(qp=37, rounding=ROUNDING, kinds_in=kinds, modes_in=modes), "scalar qp, modes given")
    assert np.array_equal(d_qps.download(np.uint8, qps.size), qps) and np.array_equal(d_modes.download(np.uint8, modes.size), modes.ravel())
    # the host-array form is the same call
    got = codec.code_mixed_frame(f.cur, f.pred, w, h, qps=qps, rounding=ROUNDING, intra_penalty=100, kinds_in=kinds, base=f.base)
    want = f.want(qps=qps, rounding=ROUNDING, penalty=100, kinds_in=kinds)
    assert np.array_equal(got["levels"], want.levels) and np.array_equal(got["nnz"], want.nnz) and np.array_equal(got["kinds"], want.kinds)
    assert np.array_equal(got["modes"], want.modes) and np.array_equal(got["costs"], want.costs)
    assert np.array_equal(got["recon"], want.recon_tiles(oracle, f.base))


# ---- 2. the consequences, on the device -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", R.SIZES)
def test_every_kind_inter_is_the_fused_ctu_call(codec, oracle, w, h):
    """consequence (a): the same arguments into xDct32CodeCtuTilesGpu"""
    cur, pred = M.pred_planes(w, h, 0)
    f = Frame(codec, oracle, cur, pred, w, h, 610 + w)
    n = f.n
    d_kinds, d_qps = dev(codec, np.zeros(6 * n, np.uint8)), dev(codec, _qps(n, 64))
    d_l, d_n, d_r = codec.alloc(n * 12288), codec.alloc(max(n * 24, 16)), codec.alloc(w * h * 2)
    for qps, qp in ((0, QP), (d_qps.ptr, 0)):
        got = f.code(qps=qps, qp=qp, kind_in=d_kinds.ptr)
        d_r.upload(f.base)
        run(codec, codec.dct32_code_ctu_tiles_dev, f.d_cur.ptr, f.d_pred.ptr, w, h, qps, qp, ROUNDING, d_l.ptr, d_n.ptr, d_r.ptr)
        assert np.array_equal(got["level"], d_l.download(np.int16, n * 6144))
        assert np.array_equal(got["nnz"], d_n.download(np.uint32, n * 6))
        assert np.array_equal(got["recon"], d_r.download(np.uint8, w * h * 2))
        assert not got["kind"].any() and (got["mode"] == 255).all() and (got["cost"] == M.NO_COST).all()


@gpu
@pytest.mark.parametrize("given", (False, True))
@pytest.mark.parametrize("w,h", R.SIZES)
def test_every_kind_intra_is_the_intra_frame(codec, oracle, w, h, given):
    """consequence (b): xIntra32CodeFrameGpu on the same arguments; d_pred holds poison and is never read"""
    cur, _ = M.pred_planes(w, h, 0)
    poison = tuple(np.full_like(p, 0xA5) for p in cur)
    f = Frame(codec, oracle, cur, poison, w, h, 620 + w)
    n = f.n
    d_kinds, d_qps, d_modes = dev(codec, np.ones(6 * n, np.uint8)), dev(codec, _qps(n, 65)), dev(codec, _modes(n, 66))
    d_l, d_n, d_m, d_r = codec.alloc(n * 12288), codec.alloc(max(n * 24, 16)), codec.alloc(max(n * 6, 16)), codec.alloc(w * h * 2)
    mp = d_modes.ptr if given else 0
    results = []
    for fill in (0xA5, 0x11):                                               # two poisons, one result
        f.pred = R.tiles(oracle, tuple(np.full_like(p, fill) for p in cur), 5)
        got = f.code(qps=d_qps.ptr, kind_in=d_kinds.ptr, mode_in=mp, penalty=1 << 24)
        results.append(got)
    d_r.upload(f.base)
    run(codec, codec.intra32_code_frame_dev, f.d_cur.ptr, w, h, d_qps.ptr, 0, ROUNDING, mp, d_l.ptr, d_n.ptr, d_m.ptr, d_r.ptr)
    for got in results:
        assert np.array_equal(got["level"], d_l.download(np.int16, n * 6144))
        assert np.array_equal(got["nnz"], d_n.download(np.uint32, n * 6))
        assert np.array_equal(got["mode"], d_m.download(np.uint8, n * 6))
        assert np.array_equal(got["recon"], d_r.download(np.uint8, w * h * 2))
        assert (got["kind"] == 1).all() and (got["cost"][0::2] == M.NO_COST).all()
        assert ((got["cost"][1::2] == M.NO_COST).all() if given else (got["cost"][1::2] < 1 << 26).all())


@gpu
@pytest.mark.parametrize("w,h", ((128, 128), (192, 128)))
def test_the_kinds_are_a_deblocking_d_intra(codec, oracle, w, h):
    """consequence (d): xDeblockGpu with d_kind as d_intra (and the call's d_nnz) equals the deblocking statement"""
    cur, pred = M.pred_planes(w, h, 1)
    f = Frame(codec, oracle, cur, pred, w, h, 630 + w)
    got = f.code(qp=37)
    want = M.coded(oracle, w, h, 1, 0, None, 37, ROUNDING)
    f.check(got, want, "coded")
    assert set(want.kinds[:, :4].ravel()) == {0, 1}
    d_out = dev(codec, f.base)
    run(codec, codec.deblock_dev, f.d_recon.ptr, w, h, codec.deblock_params(d_intra=f.d["kind"].ptr, d_nnz=f.d["nnz"].ptr, qp=37), d_out.ptr)
    side = D.Side(intra=want.kinds, nnz=want.nnz, qp=37)
    ref = D.deblock_tiles(oracle, got["recon"], w, h, side, base=f.base)
    assert np.array_equal(d_out.download(np.uint8, w * h * 2), ref)
    assert not np.array_equal(ref, D.deblock_tiles(oracle, got["recon"], w, h, D.Side(nnz=want.nnz, qp=37), base=f.base))   # the kinds matter


# ---- 3. in place, and the optional outputs ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("given", (False, True))
@pytest.mark.parametrize("w,h", R.SIZES)
def test_in_place_and_optional_outputs(codec, oracle, w, h, given):
    """d_recon == d_pred, d_kind == d_kind_in and d_mode == d_mode_in: the results of the separate-buffer call; d_nnz and d_cost NULL"""
    cur, pred = M.pred_planes(w, h, 1)
    f = Frame(codec, oracle, cur, pred, w, h, 640 + w)
    n = f.n
    kinds, modes = M.kinds_mixed(n, 11), _modes(n, 67)
    d_kinds, d_modes = dev(codec, kinds), dev(codec, modes)
    separate = f.code(kind_in=d_kinds.ptr, mode_in=d_modes.ptr if given else 0, penalty=64)
    want = f.want(qp=QP, rounding=ROUNDING, penalty=64, kinds_in=kinds, modes_in=modes if given else None)
    f.check(separate, want, "separate")
    f.reset()
    f.d["kind"].upload(kinds)
    f.d["mode"].upload(modes)
    run(codec, f.enqueue, kind_in=f.d["kind"].ptr, mode_in=f.d["mode"].ptr if given else 0, penalty=64, recon=f.d_pred.ptr, nnz=False, cost=False)
    got = f.results(recon=f.d_pred)
    f.check(got, want, "in place", nnz=False, cost=False, base=f.pred, pred_kept=False)
    for name in ("level", "kind", "mode"):
        assert np.array_equal(got[name], separate[name]), name
    assert np.array_equal(got["recon"].reshape(-1, 512)[:, :384], separate["recon"].reshape(-1, 512)[:, :384])
    assert np.array_equal(f.d_recon.download(np.uint8, w * h * 2), f.base)  # the separate reconstruction buffer was not part of the call


# ---- 4. contents: every clip of both loops side by side -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ("noise", "flat", "extreme"))
def test_contents(codec, oracle, kind):
    w, h = 128, 128
    cur, pred = M.pred_planes(w, h, 0, kind)
    f = Frame(codec, oracle, cur, pred, w, h, 650)
    kinds = M.kinds_mixed(f.n, 13)
    d_kinds = dev(codec, kinds)
    for qp in (0, 22, 51):
        f.check(f.code(qp=qp, kind_in=d_kinds.ptr), f.want(qp=qp, rounding=ROUNDING, kinds_in=kinds), (kind, qp))


# ---- 5. the tie ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("flip", (0, 1))
def test_a_tie_is_inter(codec, oracle, flip):
    from test_mixed_frame_ref import first_intra
    w, h = 64, 64
    free = M.coded(oracle, w, h, flip, 0)
    ctu, e = first_intra(free)
    inter, intra = (int(x) for x in free.costs[ctu, e])
    cur, pred = M.pred_planes(w, h, flip)
    f = Frame(codec, oracle, cur, pred, w, h, 660)
    tie, less = f.code(penalty=inter - intra), f.code(penalty=inter - intra - 1)
    f.check(tie, f.want(qp=QP, rounding=ROUNDING, penalty=inter - intra), "tie")
    f.check(less, f.want(qp=QP, rounding=ROUNDING, penalty=inter - intra - 1), "one less")
    r = 6 * ctu + e
    assert tuple(tie["cost"][2 * r:2 * r + 2]) == (inter, intra) and tuple(less["cost"][2 * r:2 * r + 2]) == (inter, intra)
    assert tie["kind"][r] == 0 and tie["mode"][r] == 255 and less["kind"][r] == 1 and less["mode"][r] == free.modes[ctu, e]


# ---- 6. captured into a graph, on a created stream: search -> refine -> motion compensation -> the call -> deblock ------------------------
@gpu
def test_the_chain_eagerly_and_from_one_graph(codec, oracle):
    w, h, rng, qp = 128, 128, 4, 32
    n, nb = codec.ctu_count(w, h), (w // 8) * (h // 8)
    cur_y, ref_y = me_frames(w, h, 0, 801, mv=(2, -1), noise=3)
    cur_u, ref_u = me_frames(w // 2, h // 2, 0, 802, mv=(1, 0), noise=3)
    cur_v, ref_v = me_frames(w // 2, h // 2, 0, 803, mv=(1, 0), noise=3)
    cur_y = cur_y.copy()
    cur_y[:64, 64:] = R.case("oriented", 64, 64)[0]                         # a CTU with no counterpart in the reference
    ct, rt = R.tiles(oracle, (cur_y, cur_u, cur_v), 804), R.tiles(oracle, (ref_y, ref_u, ref_v), 805)
    start, fills = noise(w * h * 2, 806), noise(w * h * 2, 807)
    dc, dr, dp, drec, dout = dev(codec, ct), dev(codec, rt), dev(codec, start), dev(codec, fills), dev(codec, fills)
    d_int, d_best = codec.alloc(nb * 8), codec.alloc(nb * 8)
    outs = {"level": codec.alloc(n * 12288), "nnz": codec.alloc(n * 24), "kind": codec.alloc(16 * n), "mode": codec.alloc(16 * n), "cost": codec.alloc(n * 48)}
    st = codec.stream_create()
    try:
        codec._check(codec.L.xHipMeScratchReserve(codec.ctx, st, w, h), "xHipMeScratchReserve")
        p = codec.mixed_params(w, h, qp, ROUNDING, 0, d_cur=dc.ptr, d_pred=dp.ptr, d_level=outs["level"].ptr, d_nnz=outs["nnz"].ptr, d_kind=outs["kind"].ptr,
                               d_mode=outs["mode"].ptr, d_cost=outs["cost"].ptr, d_recon=drec.ptr)
        dbk = codec.deblock_params(d_intra=outs["kind"].ptr, d_nnz=outs["nnz"].ptr, d_mv=d_best.ptr, qp=qp)

        def enqueue():
            codec.satd_search_from_tiles_dev(dc.ptr, dr.ptr, w, h, rng, d_int.ptr, stream=st)
            codec.satd_refine_qpel_from_tiles_dev(dc.ptr, dr.ptr, w, h, d_int.ptr, d_best.ptr, stream=st)
            codec.motion_comp_qpel_dev(dr.ptr, d_best.ptr, w, h, dp.ptr, stream=st)
            codec.dct32_code_mixed_frame_dev(p, stream=st)
            codec.deblock_dev(drec.ptr, w, h, dbk, dout.ptr, stream=st)

        def results():
            sync_or_exit(codec, 0, st)
            return ([dp.download(np.uint8, w * h * 2), drec.download(np.uint8, w * h * 2), dout.download(np.uint8, w * h * 2), d_best.download(np.uint8, nb * 8)] +
                    [outs[k].download(np.uint8, n * per) for k, per in Frame.OUT])

        codec.graph_begin(st)
        enqueue()
        graph = codec.graph_end(st)
        try:
            enqueue()
            eager = results()
            # the eager chain against the statements, from the prediction the device made
            want = M.code_frame(oracle, Q._planes(ct, w, h), Q._planes(eager[0], w, h), w, h, None, qp, ROUNDING, 0)
            assert set(want.kinds.ravel()) == {0, 1} and want.kinds[1, :4].any()      # intra where the reference has nothing (the search may still match a part)
            assert np.array_equal(eager[1], want.recon_tiles(oracle, fills))
            assert np.array_equal(eager[4].view(np.int16).reshape(n, 6, 1024), want.levels) and np.array_equal(eager[6].reshape(n, 6), want.kinds)
            assert np.array_equal(eager[8].view(np.uint32).reshape(n, 6, 2), want.costs)
            mv = eager[3].view(np.int16).reshape(nb, 4)[:, :2]
            assert np.array_equal(eager[2], D.deblock_tiles(oracle, eager[1], w, h, D.Side(intra=want.kinds, nnz=want.nnz, mv=mv, qp=qp), base=fills))
            for buf in [d_int, d_best] + list(outs.values()):
                buf.upload(np.zeros(buf.nbytes, np.uint8))
            dp.upload(start)
            drec.upload(fills)
            dout.upload(fills)
            for _ in range(2):
                codec.graph_launch(graph, st)
                for x, y in zip(eager, results()):
                    assert np.array_equal(x, y)
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 7. minimum alignment, inside guard bands ---------------------------------------------------------------------------------------------
AW, AH = 128, 128
PTRS = {"d_cur": 16, "d_pred": 16, "d_qp": 1, "d_kind_in": 1, "d_mode_in": 1, "d_level": 16, "d_nnz": 4, "d_kind": 1, "d_mode": 1, "d_cost": 4, "d_recon": 16}
OUTPUTS = ("d_level", "d_nnz", "d_kind", "d_mode", "d_cost", "d_recon")


@pytest.fixture(scope="module")
def arena_case(oracle):
    cur, pred = M.pred_planes(AW, AH, 0)
    n = (AW // 64) * (AH // 64)
    qps, kinds, modes = _qps(n, 68), M.kinds_mixed(n, 15), _modes(n, 69)
    want = M.code_frame(oracle, cur, pred, AW, AH, qps, 0, ROUNDING, 32, kinds, modes)
    return {"d_cur": R.tiles(oracle, cur, 70), "d_pred": R.tiles(oracle, pred, 71), "d_qp": qps, "d_kind_in": kinds, "d_mode_in": modes,
            "d_level": want.levels.ravel(), "d_nnz": want.nnz.ravel(), "d_kind": want.kinds.ravel(), "d_mode": want.modes.ravel(),
            "d_cost": want.costs.ravel(), "coded": want, "oracle": oracle}


def _arena(codec, arena_case, disp, guard_seed):
    return arena_slots(codec, PTRS, OUTPUTS, arena_case, disp, guard_seed, written={"d_recon": tile_written(AW * AH // 256, "both")},
                       sizes={"d_recon": AW * AH * 2})


def _call_arena(codec, s):
    p = codec.mixed_params(AW, AH, 0, ROUNDING, 32, **{name: slot.ptr for name, slot in s.items()})
    rc = codec.L.xDct32CodeMixedFrameGpu(codec.ctx, p, None)
    sync_or_exit(codec, rc)
    return rc


@gpu
def test_minimum_alignment(codec, arena_case):
    results = []
    for guard_seed in (31, 51):
        a, s = _arena(codec, arena_case, displacements(PTRS), guard_seed)
        assert _call_arena(codec, s) == 0, codec.L.xHipLastError(codec.ctx)
        got = a.check()                                                     # guards, m_I of d_recon, inputs
        for p in OUTPUTS:
            if p == "d_recon":
                want = arena_case["coded"].recon_tiles(arena_case["oracle"], s[p].image[s[p].start:][:AW * AH * 2])
            else:
                want = np.ascontiguousarray(arena_case[p]).view(np.uint8)
            assert np.array_equal(got[p], want), p
        results.append([got[p] for p in OUTPUTS])
    for x, y in zip(*results):
        assert np.array_equal(x, y)                                         # the garbage around the inputs reaches no output byte


@gpu
@pytest.mark.parametrize("ptr", [p for p in PTRS if PTRS[p] > 1])
def test_half_alignment_is_rejected(codec, arena_case, ptr):
    a, s = _arena(codec, arena_case, displacements(PTRS, halved=ptr), 33)
    assert _call_arena(codec, s) == EINVAL
    assert CALL.encode() in codec.L.xHipLastError(codec.ctx)
    a.check_untouched()


# ---- 8. arguments ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_argument_errors(codec):
    """one refused call per rule of the header; a refused call launches nothing and names itself"""
    L, ctx = codec.L, codec.ctx
    buf = codec.alloc(8 << 20)
    fill = noise(8 << 20, 95)
    buf.upload(fill)
    # 64x64: tile arrays of 8 KiB, 12 KiB of levels; 24, 6, 6, 48, 6, 6, 6 bytes
    cur, prd, rec, lvl = (buf.ptr + (i << 20) for i in (1, 2, 3, 4))
    nnz, kind, mode, cost, qps, kin, min_ = (buf.ptr + (5 << 20) + 4096 * i for i in range(7))
    top, top4, top1 = 2 ** 64 - 4096, 2 ** 64 - 4, 2 ** 64 - 1              # aligned, and nothing of theirs fits behind them

    def P(w=64, h=64, qp=QP, rounding=ROUNDING, penalty=0, **kw):
        ptrs = dict(d_cur=cur, d_pred=prd, d_level=lvl, d_nnz=nnz, d_kind=kind, d_mode=mode, d_cost=cost, d_recon=rec)
        ptrs.update(kw)
        return codec.mixed_params(w, h, qp, rounding, penalty, **ptrs)

    assert L.xDct32CodeMixedFrameGpu(None, P(), None) == EINVAL
    assert L.xDct32CodeMixedFrameGpu(ctx, None, None) == EINVAL and CALL.encode() in L.xHipLastError(ctx)
    refusals = [P(d_cur=0), P(d_pred=0), P(d_level=0), P(d_kind=0), P(d_mode=0), P(d_recon=0),
                P(d_cur=cur + 8), P(d_pred=prd + 8), P(d_level=lvl + 8), P(d_recon=rec + 8), P(d_nnz=nnz + 2), P(d_cost=cost + 2),
                P(w=0), P(h=-64), P(w=32), P(w=96), P(h=80),
                P(qp=52), P(qp=-1), P(rounding=-1), P(rounding=512), P(d_qp=qps, rounding=512), P(penalty=-1), P(penalty=(1 << 24) + 1),
                P(d_cur=top), P(d_pred=top), P(d_recon=top), P(d_level=top), P(d_nnz=top4), P(d_cost=top4), P(d_kind=top1), P(d_mode=top1), P(d_qp=top1),
                P(d_kind_in=top1), P(d_mode_in=top1),
                P(d_recon=cur), P(d_recon=cur + 4096), P(d_recon=cur - 8176), P(d_recon=prd + 16), P(d_recon=prd - 8176),   # only d_recon == d_pred itself
                P(d_level=cur + 16), P(d_level=prd + 16), P(d_level=rec - 12272), P(d_nnz=cur + 8188), P(d_nnz=rec), P(d_nnz=lvl + 12284), P(d_nnz=prd),
                P(d_cost=cur), P(d_cost=prd + 8188), P(d_cost=rec), P(d_cost=lvl), P(d_cost=nnz + 20), P(d_cost=kind + 4), P(d_cost=mode - 44),
                P(d_kind=cur), P(d_kind=prd), P(d_kind=rec + 8191), P(d_kind=lvl + 100), P(d_kind=nnz + 23), P(d_kind=mode + 5), P(d_kind=cost + 47),
                P(d_mode=cur), P(d_mode=prd + 1), P(d_mode=rec), P(d_mode=lvl + 12287), P(d_mode=nnz), P(d_mode=kind - 5), P(d_mode=cost),
                P(d_qp=qps, d_mode=qps + 5), P(d_qp=qps, d_kind=qps), P(d_qp=rec + 17), P(d_qp=lvl - 5), P(d_qp=nnz - 5), P(d_qp=cost + 47),
                P(d_kind_in=kin, d_kind=kin + 1), P(d_kind_in=kin, d_kind=kin - 5), P(d_kind_in=kin, d_mode=kin), P(d_kind_in=rec), P(d_kind_in=lvl + 12287),
                P(d_kind_in=nnz + 23), P(d_kind_in=cost), P(d_kind_in=mode + 1),                                            # only d_kind == d_kind_in itself
                P(d_mode_in=min_, d_mode=min_ + 1), P(d_mode_in=min_, d_mode=min_ - 5), P(d_mode_in=min_, d_kind=min_), P(d_mode_in=rec), P(d_mode_in=lvl + 1),
                P(d_mode_in=nnz + 23), P(d_mode_in=cost + 47), P(d_mode_in=kind + 1)]
    for p in refusals:
        assert L.xDct32CodeMixedFrameGpu(ctx, p, None) == EINVAL, [(f[0], getattr(p, f[0])) for f in p._fields_]
        assert CALL.encode() in L.xHipLastError(ctx)
    assert np.array_equal(buf.download(np.uint8, 8 << 20), fill)            # nothing was launched
    # the edges of what is accepted: the scalars at both ends, qp out of range under d_qp, every optional pointer NULL or given, the three
    # allowed overlaps, one frame as both inputs
    buf.upload(np.zeros(8 << 20, np.uint8))                                 # mode bytes above 34 are undefined input
    for p in (P(qp=0, rounding=0, d_nnz=0, d_cost=0), P(qp=51, rounding=511, penalty=1 << 24), P(d_qp=qps, qp=99, d_kind_in=kin, d_mode_in=min_),
              P(d_recon=prd), P(d_kind_in=kin, d_kind=kin), P(d_mode_in=min_, d_mode=min_), P(d_pred=cur)):
        rc = L.xDct32CodeMixedFrameGpu(ctx, p, None)
        sync_or_exit(codec, rc)
        assert rc == 0, L.xHipLastError(ctx)
