"""Sample adaptive offset on tiled frames: xSaoStatsGpu / DecideGpu / SearchGpu / ApplyGpu against the reference statement of
tests/_sao_ref.py (the header's arithmetic in numpy int64, checked against plain loops by tests/test_sao_ref.py).  Every comparison
is bit-exact; every test but the export test is marked gpu."""
import ctypes
import subprocess

import numpy as np
import pytest

import _deblock_ref as D
import _sao_ref as R
import x266_amd
from _dev import EINVAL, arena_slots, dev, displacements, noise, records, run, sync_or_exit, tile_written, tiles
from _util import me_frames, splitmix64

gpu = pytest.mark.gpu
NAMES = ("xSaoStatsGpu", "xSaoDecideGpu", "xSaoSearchGpu", "xSaoApplyGpu")


# ---- the export test (CPU) ------------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_four_calls():
    x266_amd.build_library()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode().split()
    lib = x266_amd.load_library()
    for name in NAMES:
        assert name in exported, name
        assert getattr(lib, name).argtypes, name                            # bound by _lib.py, with its argument types
    for method in ("sao_stats_dev", "sao_decide_dev", "sao_search_dev", "sao_apply_dev", "sao_stats", "sao_decide", "sao_search", "sao_apply"):
        assert callable(getattr(x266_amd.Codec, method)), method


# ---- 1. each call against the statement -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", R.SIZES)
def test_each_call_against_the_statement(codec, oracle, w, h):
    """every kind of the recipe, three lambdas: statistics, the decision on them, the fused search with and without d_stats, and apply
    over a random pre-fill (m_I and everything outside the planes untouched); all inputs unchanged"""
    n = codec.ctu_count(w, h)
    base = noise(w * h * 2, 77)
    for kind in R.KINDS:
        org_p, dec_p = R.case(kind, w, h)
        org, dec = tiles(oracle, org_p, 60 + h), tiles(oracle, dec_p, 61 + h)
        want_stats = R.stats(org_p, dec_p)
        words = R.stats_words(want_stats)
        d_org, d_dec, d_stats = dev(codec, org), dev(codec, dec), dev(codec, noise(n * 1152, 78))
        run(codec, codec.sao_stats_dev, d_org.ptr, d_dec.ptr, w, h, d_stats.ptr)
        assert np.array_equal(d_stats.download(np.int32, n * 288), words), kind
        for lam in R.LAMBDAS:
            want = R.decide(want_stats, lam).ravel()
            d_par, d_par2, d_par3 = (dev(codec, noise(n * 24, 79 + i)) for i in range(3))
            d_stats2 = dev(codec, noise(n * 1152, 83))
            run(codec, codec.sao_decide_dev, d_stats.ptr, n, lam, d_par.ptr)
            run(codec, codec.sao_search_dev, d_org.ptr, d_dec.ptr, w, h, lam, d_par2.ptr, d_stats2.ptr)
            run(codec, codec.sao_search_dev, d_org.ptr, d_dec.ptr, w, h, lam, d_par3.ptr, 0)
            for d in (d_par, d_par2, d_par3):
                assert np.array_equal(d.download(np.uint8, n * 24), want), (kind, lam)
            assert np.array_equal(d_stats2.download(np.int32, n * 288), words), (kind, lam)
            d_out = dev(codec, base)
            run(codec, codec.sao_apply_dev, d_dec.ptr, w, h, d_par.ptr, d_out.ptr)
            assert np.array_equal(d_out.download(np.uint8, base.size), R.apply_tiles(oracle, dec, want, w, h, base)), (kind, lam)
            assert np.array_equal(d_par.download(np.uint8, n * 24), want), (kind, lam)
        assert np.array_equal(d_org.download(np.uint8, org.size), org) and np.array_equal(d_dec.download(np.uint8, dec.size), dec), kind
        assert np.array_equal(d_stats.download(np.int32, n * 288), words), kind
    # the host-array forms are the same calls
    st = codec.sao_stats(org, dec, w, h)
    par, st2 = codec.sao_search(org, dec, w, h, 37, want_stats=True)
    assert np.array_equal(st.ravel(), words) and np.array_equal(st2, st) and np.array_equal(codec.sao_decide(st, 37), par)
    assert np.array_equal(codec.sao_apply(dec, w, h, par, base=base), R.apply_tiles(oracle, dec, par, w, h, base))


# ---- 2. parameters the decision never emits -------------------------------------------------------------------------------------------
def _record(typ, arg, offs):
    return np.array([typ, arg] + [o & 255 for o in offs] + [0, 0], np.uint8)


@gpu
def test_hand_written_parameters(codec, oracle):
    """a band position that wraps, +-127 on samples near 0 and 255 (the clip), types that mean "copy", class bits under garbage, and
    U and V with records of their own"""
    w, h = 144, 80
    _, dec_p = R.case("sharp2", w, h)
    planes = []
    for m, p in enumerate(dec_p):
        r = splitmix64(300 + m, 0, p.size).reshape(p.shape)
        pick = ((r >> np.uint64(8)) & np.uint64(7)).astype(np.int64)
        ends = ((r >> np.uint64(16)) & np.uint64(15)).astype(np.uint8)
        planes.append(np.where(pick == 0, ends, np.where(pick == 1, 255 - ends, p)).astype(np.uint8))
    dec = tiles(oracle, planes, 90)
    params = np.zeros((6, 3, 8), np.uint8)
    params[0] = [_record(1, 30, (127, -127, 5, -128)), _record(2, 0xFE, (127, -128, 100, -100)), _record(1, 0xFF, (-7, 7, -127, 127))]
    params[1] = [_record(2, 0x47, (-128, 127, -3, 3)), _record(1, 29, (1, 2, 3, 4)), _record(2, 0x81, (9, -9, 9, -9))]
    params[2] = [_record(3, 1, (5, 5, 5, 5)), _record(255, 2, (7, 7, 7, 7)), _record(2, 0, (1, 1, -1, -1))]
    params[3] = [_record(2, 1, (127, 127, -128, -128)), _record(0, 3, (9, 9, 9, 9)), _record(1, 0, (127, 127, 127, 127))]
    params[4] = [_record(1, 31, (-128, -128, -128, -128)), _record(2, 3, (2, 1, -1, -2)), _record(4, 0, (1, 1, 1, 1))]
    params[5] = [_record(2, 2, (6, 0, 0, -6)), _record(2, 0xFC, (127, 0, 0, -128)), _record(2, 0x07, (0, 127, -128, 0))]
    params[:, :, 6:] = 0xA5                                                 # zero[] is not read
    base = noise(w * h * 2, 91)
    want = R.apply_tiles(oracle, dec, params, w, h, base)
    changed = (want.reshape(-1, 512)[:, :384] != dec.reshape(-1, 512)[:, :384])
    assert changed.any() and (want.reshape(-1, 512)[:, :384][changed] == 0).any() and (want.reshape(-1, 512)[:, :384][changed] == 255).any()
    d_in, d_par, d_out = dev(codec, dec), dev(codec, params), dev(codec, base)
    run(codec, codec.sao_apply_dev, d_in.ptr, w, h, d_par.ptr, d_out.ptr)
    assert np.array_equal(d_out.download(np.uint8, base.size), want)
    assert np.array_equal(d_in.download(np.uint8, dec.size), dec) and np.array_equal(d_par.download(np.uint8, params.size), params.ravel())


# ---- 3. behind the coding call and the deblocking filter, eagerly and in a graph ----------------------------------------------------------
def _coding_inputs(oracle, w, h, seed):
    cur_y, ref_y = me_frames(w, h, 0, seed, mv=(-3, 2), noise=5)
    cur_u, ref_u = me_frames(w // 2, h // 2, 0, seed + 1, mv=(-1, 1), noise=5)
    cur_v, ref_v = me_frames(w // 2, h // 2, 0, seed + 2, mv=(-1, 1), noise=5)
    return tiles(oracle, (cur_y, cur_u, cur_v), seed + 3), tiles(oracle, (ref_y, ref_u, ref_v), seed + 4)


@gpu
def test_chain_behind_coding_and_deblocking(codec, oracle):
    """xDct32CodeCtuTilesGpu, xDeblockGpu in place, xSaoSearchGpu with the current frame as org, xSaoApplyGpu into a fresh frame: the
    statement on the downloaded deblocked frame; xMotionCompQpelGpu accepts the result as d_ref"""
    w, h, n = 128, 64, codec.ctu_count(128, 64)
    cur, pred = _coding_inputs(oracle, w, h, 900)
    side = D.case("blocks", w, h)[3]
    dc, dp, dl, dn = dev(codec, cur), dev(codec, pred), codec.alloc(n * 12288), codec.alloc(n * 24)
    d_intra, d_mv = dev(codec, side.intra), dev(codec, records(side.mv))
    run(codec, codec.dct32_code_ctu_tiles_dev, dc.ptr, dp.ptr, w, h, 0, 44, 171, dl.ptr, dn.ptr, dp.ptr)
    run(codec, codec.deblock_dev, dp.ptr, w, h, codec.deblock_params(0, d_intra.ptr, dn.ptr, 0, d_mv.ptr, 44, 0, 0), dp.ptr)
    deblocked = dp.download(np.uint8, w * h * 2)
    base = noise(w * h * 2, 92)
    d_par, d_sao = codec.alloc(n * 24), dev(codec, base)
    run(codec, codec.sao_search_dev, dc.ptr, dp.ptr, w, h, 4, d_par.ptr, 0)
    run(codec, codec.sao_apply_dev, dp.ptr, w, h, d_par.ptr, d_sao.ptr)
    want_par = R.decide(R.stats_tiles(oracle, cur, deblocked, w, h), 4)
    assert want_par[:, :, 0].any()                                          # the chain does filter something
    assert np.array_equal(d_par.download(np.uint8, n * 24), want_par.ravel())
    got = d_sao.download(np.uint8, w * h * 2)
    assert np.array_equal(got, R.apply_tiles(oracle, deblocked, want_par, w, h, base))
    assert np.array_equal(dp.download(np.uint8, w * h * 2), deblocked) and np.array_equal(dc.download(np.uint8, w * h * 2), cur)
    d_next = codec.alloc(w * h * 2)
    run(codec, codec.motion_comp_qpel_dev, d_sao.ptr, d_mv.ptr, w, h, d_next.ptr)


@gpu
def test_code_deblock_and_sao_in_one_graph(codec, oracle):
    """the same linear chain captured as one graph and replayed twice on fresh inputs: the eager results"""
    w, h, n = 128, 64, codec.ctu_count(128, 64)
    frames = [_coding_inputs(oracle, w, h, 910 + 10 * i) for i in range(3)]
    side = D.case("steps", w, h)[3]
    d_intra, d_mv = dev(codec, side.intra), dev(codec, records(side.mv))
    dc, dp, dl, dn = codec.alloc(w * h * 2), codec.alloc(w * h * 2), codec.alloc(n * 12288), codec.alloc(n * 24)
    d_par, d_stats, d_sao = codec.alloc(n * 24), codec.alloc(n * 1152), codec.alloc(w * h * 2)
    params = codec.deblock_params(0, d_intra.ptr, dn.ptr, 0, d_mv.ptr, 44, 0, 0)
    st = codec.stream_create()
    try:
        def enqueue():
            codec.dct32_code_ctu_tiles_dev(dc.ptr, dp.ptr, w, h, 0, 44, 171, dl.ptr, dn.ptr, dp.ptr, stream=st)
            codec.deblock_dev(dp.ptr, w, h, params, dp.ptr, stream=st)
            codec.sao_search_dev(dc.ptr, dp.ptr, w, h, 4, d_par.ptr, d_stats.ptr, stream=st)
            codec.sao_apply_dev(dp.ptr, w, h, d_par.ptr, d_sao.ptr, stream=st)

        def load(i):
            dc.upload(frames[i][0])
            dp.upload(frames[i][1])
            d_sao.upload(np.zeros(w * h * 2, np.uint8))

        def results():
            sync_or_exit(codec, 0, st)
            return d_sao.download(np.uint8, w * h * 2), d_par.download(np.uint8, n * 24), d_stats.download(np.int32, n * 288)

        eager = []
        for i in range(3):
            load(i)
            enqueue()
            eager.append(results())
        assert not np.array_equal(eager[1][0], eager[2][0]) and eager[1][1].reshape(-1, 8)[:, 0].any()
        load(0)
        codec.graph_begin(st)
        enqueue()
        graph = codec.graph_end(st)
        try:
            for i in (1, 2):
                load(i)
                codec.graph_launch(graph, st)
                for x, y in zip(eager[i], results()):
                    assert np.array_equal(x, y), i
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 4. arguments and alignment -------------------------------------------------------------------------------------------------------
AW, AH, ALAM = 80, 48, 37
PTRS = {"xSaoStatsGpu": {"d_org": 16, "d_dec": 16, "d_stats": 4},
        "xSaoDecideGpu": {"d_stats": 4, "d_param": 8},
        "xSaoSearchGpu": {"d_org": 16, "d_dec": 16, "d_param": 8, "d_stats": 4},
        "xSaoApplyGpu": {"d_in": 16, "d_param": 8, "d_out": 16}}
OUTPUTS = {"xSaoStatsGpu": ("d_stats",), "xSaoDecideGpu": ("d_param",), "xSaoSearchGpu": ("d_param", "d_stats"), "xSaoApplyGpu": ("d_out",)}


@pytest.fixture(scope="module")
def arena_case(oracle):
    org_p, dec_p = R.case("sharp3", AW, AH)
    org, dec = tiles(oracle, org_p, 804), tiles(oracle, dec_p, 805)
    st = R.stats(org_p, dec_p)
    par = R.decide(st, ALAM)
    return {"d_org": org, "d_dec": dec, "d_in": dec, "d_stats": R.stats_words(st), "d_param": par.ravel(), "oracle": oracle}


def _arena(codec, arena_case, name, disp, guard_seed):
    return arena_slots(codec, PTRS[name], OUTPUTS[name], arena_case, disp, guard_seed, written={"d_out": tile_written(AW * AH // 256, "both")},
                       sizes={"d_out": AW * AH * 2})


def _call_arena(codec, name, s):
    L, n = codec.L, codec.ctu_count(AW, AH)
    if name == "xSaoStatsGpu":
        rc = L.xSaoStatsGpu(codec.ctx, s["d_org"].ptr, s["d_dec"].ptr, AW, AH, s["d_stats"].ptr, None)
    elif name == "xSaoDecideGpu":
        rc = L.xSaoDecideGpu(codec.ctx, s["d_stats"].ptr, n, ALAM, s["d_param"].ptr, None)
    elif name == "xSaoSearchGpu":
        rc = L.xSaoSearchGpu(codec.ctx, s["d_org"].ptr, s["d_dec"].ptr, AW, AH, ALAM, s["d_param"].ptr, s["d_stats"].ptr, None)
    else:
        rc = L.xSaoApplyGpu(codec.ctx, s["d_in"].ptr, AW, AH, s["d_param"].ptr, s["d_out"].ptr, None)
    sync_or_exit(codec, rc)
    return rc


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_minimum_alignment(codec, arena_case, name):
    results = []
    for guard_seed in (31, 51):
        a, s = _arena(codec, arena_case, name, displacements(PTRS[name]), guard_seed)
        assert _call_arena(codec, name, s) == 0, codec.L.xHipLastError(codec.ctx)
        got = a.check()                                                     # guards, m_I of d_out, inputs
        for p in OUTPUTS[name]:
            if p == "d_out":
                base = s[p].image[s[p].start:][:AW * AH * 2]
                want = R.apply_tiles(arena_case["oracle"], arena_case["d_in"], arena_case["d_param"], AW, AH, base)
            else:
                want = arena_case[p].view(np.uint8)
            assert np.array_equal(got[p], want), p
        results.append([got[p] for p in OUTPUTS[name]])
    for x, y in zip(*results):
        assert np.array_equal(x, y)                                         # the garbage around the inputs reaches no output byte


@gpu
@pytest.mark.parametrize("name,ptr", [(n, p) for n in NAMES for p in PTRS[n]])
def test_half_alignment_is_rejected(codec, arena_case, name, ptr):
    a, s = _arena(codec, arena_case, name, displacements(PTRS[name], halved=ptr), 33)
    assert _call_arena(codec, name, s) == EINVAL
    assert name.encode() in codec.L.xHipLastError(codec.ctx)
    a.check_untouched()


@gpu
def test_argument_errors(codec):
    """one refused call per rule, for every call; a refused call launches nothing and names itself"""
    L, ctx = codec.L, codec.ctx
    buf = codec.alloc(8 << 20)
    fill = noise(8 << 20, 95)
    buf.upload(fill)
    o, d, out = buf.ptr + (1 << 20), buf.ptr + (2 << 20), buf.ptr + (3 << 20)    # 64x64 tile arrays (8 KiB each)
    st, par = buf.ptr + (4 << 20), buf.ptr + (5 << 20)                      # 1152 and 24 bytes per CTU
    top, top8, top4 = 2 ** 64 - 4096, 2 ** 64 - 8, 2 ** 64 - 4             # aligned, and nothing fits behind them
    V = ctypes.c_void_p

    def refused(name, *args):
        assert getattr(L, name)(ctx, *args, None) == EINVAL, (name, args)
        assert name.encode() in L.xHipLastError(ctx), (name, args)

    for name in NAMES:
        fn = getattr(L, name)
        null_ctx = {"xSaoStatsGpu": (V(o), V(d), 64, 64, V(st)), "xSaoDecideGpu": (V(st), 1, 0, V(par)),
                    "xSaoSearchGpu": (V(o), V(d), 64, 64, 0, V(par), V(st)), "xSaoApplyGpu": (V(d), 64, 64, V(par), V(out))}[name]
        assert fn(None, *null_ctx, None) == EINVAL
    for a in ((None, d, 64, 64, st), (o, None, 64, 64, st), (o, d, 64, 64, None), (o + 8, d, 64, 64, st), (o, d + 8, 64, 64, st), (o, d, 64, 64, st + 2),
              (o, d, 56, 64, st), (o, d, 64, 8, st), (o, d, 0, 64, st), (o, d, 64, -16, st),
              (top, d, 64, 64, st), (o, top, 64, 64, st), (o, d, 64, 64, top4),
              (o, d, 64, 64, o + 100), (o, d, 64, 64, d - 1000), (o, d, 64, 64, d + 8188)):
        refused("xSaoStatsGpu", *a)
    for a in ((None, 1, 0, par), (st, 1, 0, None), (st + 2, 1, 0, par), (st, 1, 0, par + 4), (st, 1, -1, par), (st, 1, 65536, par),
              (st, 2 ** 31, 0, par), (st, 2 ** 62, 0, par), (top4, 1, 0, par), (st, 1, 0, top8),
              (st, 1, 0, st), (st, 1, 0, st + 1144), (st, 4, 0, st - 88)):
        refused("xSaoDecideGpu", *a)
    for a in ((None, d, 64, 64, 0, par, st), (o, None, 64, 64, 0, par, st), (o, d, 64, 64, 0, None, st), (o + 8, d, 64, 64, 0, par, st),
              (o, d + 8, 64, 64, 0, par, st), (o, d, 64, 64, 0, par + 4, st), (o, d, 64, 64, 0, par, st + 2),
              (o, d, 72, 64, 0, par, st), (o, d, 64, 0, 0, par, st), (o, d, 64, 64, -1, par, st), (o, d, 64, 64, 65536, par, st),
              (top, d, 64, 64, 0, par, st), (o, top, 64, 64, 0, par, st), (o, d, 64, 64, 0, top8, st), (o, d, 64, 64, 0, par, top4),
              (o, d, 64, 64, 0, o + 8, st), (o, d, 64, 64, 0, d - 16, None), (o, d, 64, 64, 0, par, d + 4), (o, d, 64, 64, 0, par, par - 1148),
              (o, d, 64, 64, 0, st + 16, st)):
        refused("xSaoSearchGpu", *a)
    for a in ((None, 64, 64, par, out), (d, 64, 64, None, out), (d, 64, 64, par, None), (d + 8, 64, 64, par, out), (d, 64, 64, par + 4, out),
              (d, 64, 64, par, out + 8), (d, 56, 64, par, out), (d, 64, 24, par, out), (d, -64, 64, par, out),
              (top, 64, 64, par, out), (d, 64, 64, top8, out), (d, 64, 64, par, top),
              (d, 64, 64, par, d), (d, 64, 64, par, d + 4096), (d, 64, 64, par, d - 8176), (d, 64, 64, out + 8184, out), (d, 64, 64, out - 16, out)):
        refused("xSaoApplyGpu", *a)
    assert np.array_equal(buf.download(np.uint8, 8 << 20), fill)            # nothing was launched
    # the edges of what is accepted: no CTUs, lambda at both ends, d_org == d_dec, search without d_stats
    buf.upload(np.zeros(8 << 20, np.uint8))
    for rc in (L.xSaoDecideGpu(ctx, V(st), 0, 0, V(par), None), L.xSaoDecideGpu(ctx, V(st), 1, 65535, V(par), None),
               L.xSaoStatsGpu(ctx, V(o), V(o), 64, 64, V(st), None), L.xSaoSearchGpu(ctx, V(o), V(o), 64, 64, 65535, V(par), None, None),
               L.xSaoApplyGpu(ctx, V(d), 64, 64, V(par), V(out), None)):
        sync_or_exit(codec, rc)
        assert rc == 0, L.xHipLastError(ctx)
