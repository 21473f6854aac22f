"""GPU: randomised differential tests of the frame-chain calls.  One test per family runs the family's case list of tests/_frame_cases.py
(tests/test_frame_cases.py holds the same lists against the coverage conditions on the CPU) through every call of the family, each over
a seeded pre-fill, and compares bit for bit with the statement the family's own tests use: the bytes a call owns, every other byte of
its outputs (m_I included) still the pre-fill, the inputs unchanged.  Where a call may run in place the case's draw decides which form
runs.  The drivers are the family tests' own (imported from their modules); a device error ends the session, and no case is retried.
Two more tests decode the packed level stream of the two frame coding calls
with tests/_decode_ref.py and compare the rebuilt frame with d_recon.  X266_FUZZ_SCALE=k runs k-fold lists."""
import contextlib

import numpy as np
import pytest

import _alf_ref as A
import _aq_ref as Q
import _bipred_ref as B
import _decode_ref
import _deblock_ref as D
import _frame_cases as F
import _intra_frame_ref as I
import _la_ref as L
import _mixed_frame_ref as M
import _quant_ref as QR
import _rdoq_ref as RQ
import _sao_ref as S
import _seeded_ref as E
import _subpel_ref as P
from _dev import dev, noise, records, run, same, sentinels
from _dev import tiles as _tiles                                       # `tiles` is what the tests here call their tile arrays
import test_gpu_aq as TQ
import test_gpu_deblock as TD
import test_gpu_intra_frame as TI
import test_gpu_la as TL
import test_gpu_levels as TV
import test_gpu_mixed_frame as TM
import test_gpu_rdoq as TR
import test_gpu_bipred as TB
import test_gpu_seeded as TE
import test_gpu_subpel as TP
import test_gpu_tdecide as TT

pytestmark = pytest.mark.gpu
TAIL = 64                                                                   # bytes behind an output array that must stay the pre-fill



def _same(got, want, what):
    bad = np.flatnonzero(np.asarray(got).ravel() != np.asarray(want).ravel())
    assert bad.size == 0, (what, bad[:8], np.asarray(got).ravel()[bad[:8]], np.asarray(want).ravel()[bad[:8]])


def _output(codec, nbytes, seed):
    """a device array of nbytes + TAIL seeded bytes, and those bytes"""
    fill = noise(nbytes + TAIL, seed)
    return dev(codec, fill), fill


def _owned(d, fill, nbytes, dtype, want, what):
    """the first nbytes of an output equal `want`, the tail is still the pre-fill"""
    got = d.download(np.uint8, fill.size)
    _same(got[:nbytes].view(dtype), want, what)
    _same(got[nbytes:], fill[nbytes:], (what, "behind the array"))


def _unchanged(pairs, what):
    for d, host in pairs:
        host = np.ascontiguousarray(host).view(np.uint8).ravel()
        _same(d.download(np.uint8, host.size), host, (what, "an input changed"))


# ---- deblocking ---------------------------------------------------------------------------------------------------------------------------
def test_deblock(codec, oracle):
    for c in F.cases("deblock"):
        w, h, what = c["w"], c["h"], F.tag(c)
        y, u, v, side = F.deblock_content(c)
        tiles = _tiles(oracle, (y, u, v), c["seed"] + 1)
        base = sentinels(w, h, c["seed"] + 2)
        ds = TD.DevSide(codec, side)
        for planes in ("luma", "chroma", "both"):
            d_in = dev(codec, tiles)
            d_out = d_in if c["inplace"] else dev(codec, base)
            run(codec, TD._call, codec, planes, d_in, w, h, ds, d_out)
            _same(d_out.download(np.uint8, tiles.size), D.deblock_tiles(oracle, tiles, w, h, side, None if c["inplace"] else base, planes), (what, planes))
            if not c["inplace"]:
                _unchanged([(d_in, tiles)], (what, planes))
        ds.assert_unchanged()


# ---- sample adaptive offset ---------------------------------------------------------------------------------------------------------------
def test_sao(codec, oracle):
    for c in F.cases("sao"):
        w, h, lam, seed, what = c["w"], c["h"], c["lam"], c["seed"], F.tag(c)
        n = codec.ctu_count(w, h)
        assert n == F.ctu_count(w, h)
        org_p, dec_p = F.sao_content(c)
        org, dec = _tiles(oracle, org_p, seed + 1), _tiles(oracle, dec_p, seed + 2)
        st = S.stats(org_p, dec_p)
        words, want = S.stats_words(st), S.decide(st, lam).ravel()
        d_org, d_dec = dev(codec, org), dev(codec, dec)
        d_stats, f_stats = _output(codec, n * 1152, seed + 3)
        run(codec, codec.sao_stats_dev, d_org.ptr, d_dec.ptr, w, h, d_stats.ptr)
        _owned(d_stats, f_stats, n * 1152, np.int32, words, (what, "stats"))
        d_par, f_par = _output(codec, n * 24, seed + 4)
        run(codec, codec.sao_decide_dev, d_stats.ptr, n, lam, d_par.ptr)
        _owned(d_par, f_par, n * 24, np.uint8, want, (what, "decide"))
        d_par2, f_par2 = _output(codec, n * 24, seed + 5)
        d_stats2, f_stats2 = _output(codec, n * 1152, seed + 6)
        with_stats = "d_stats" not in c["null"]
        run(codec, codec.sao_search_dev, d_org.ptr, d_dec.ptr, w, h, lam, d_par2.ptr, d_stats2.ptr if with_stats else 0)
        _owned(d_par2, f_par2, n * 24, np.uint8, want, (what, "search"))
        _owned(d_stats2, f_stats2, n * 1152 if with_stats else 0, np.int32, words if with_stats else words[:0], (what, "search's stats"))
        base = noise(w * h * 2, seed + 7)
        d_out = dev(codec, base)
        run(codec, codec.sao_apply_dev, d_dec.ptr, w, h, d_par.ptr, d_out.ptr)
        _same(d_out.download(np.uint8, base.size), S.apply_tiles(oracle, dec, want, w, h, base), (what, "apply"))
        _owned(d_stats, f_stats, n * 1152, np.int32, words, (what, "stats after decide"))
        _owned(d_par, f_par, n * 24, np.uint8, want, (what, "params after apply"))
        _unchanged([(d_org, org), (d_dec, dec)], what)


# ---- adaptive loop filter -----------------------------------------------------------------------------------------------------------------
def test_alf(codec, oracle):
    words_per_ctu = A.CTU_WORDS
    for c in F.cases("alf"):
        w, h, lam, seed, what = c["w"], c["h"], c["lam"], c["seed"], F.tag(c)
        n, nb = codec.ctu_count(w, h), (w // 4) * (h // 4)
        org_p, dec_p = F.alf_content(c)
        org, dec = _tiles(oracle, org_p, seed + 1), _tiles(oracle, dec_p, seed + 2)
        own_map = "d_class" not in c["null"]
        cmap = F.alf_class_map(c) if own_map else None
        st = A.stats(org_p, dec_p, cmap)
        luma, chroma, ctrl, mask = F.alf_sets(c, st)
        n_luma, n_chroma = c["n_luma"], c["n_chroma"]
        d_org, d_dec = dev(codec, org), dev(codec, dec)
        d_cls, f_cls = _output(codec, nb, seed + 3)
        run(codec, codec.alf_classify_dev, d_dec.ptr, w, h, d_cls.ptr)
        _owned(d_cls, f_cls, nb, np.uint8, A.classify(dec_p[0]), (what, "classify"))
        d_map = dev(codec, cmap) if own_map else None
        d_stats, f_stats = _output(codec, n * words_per_ctu * 4, seed + 4)
        run(codec, codec.alf_stats_dev, d_org.ptr, d_dec.ptr, w, h, d_map.ptr if own_map else 0, d_stats.ptr)
        words = A.stats_words(st)
        assert np.array_equal(words.astype(np.int64), st.ravel()), what       # the statement's sums fit int32
        _owned(d_stats, f_stats, n * words_per_ctu * 4, np.int32, words, (what, "stats"))
        d_total, f_total = _output(codec, words_per_ctu * 8, seed + 5)
        d_mask = None if mask is None else dev(codec, mask)
        run(codec, codec.alf_sum_stats_dev, d_stats.ptr, n, 0 if mask is None else d_mask.ptr, d_total.ptr)
        _owned(d_total, f_total, words_per_ctu * 8, np.int64, A.sum_stats(st, mask), (what, "sum"))
        d_luma, d_chroma = (dev(codec, luma) if n_luma else None), (dev(codec, chroma) if n_chroma else None)
        p_luma, p_chroma = d_luma.ptr if n_luma else 0, d_chroma.ptr if n_chroma else 0
        d_pick, f_pick = _output(codec, 3 * n, seed + 6)
        run(codec, codec.alf_decide_dev, d_stats.ptr, n, p_luma, n_luma, p_chroma, n_chroma, lam, d_pick.ptr)
        _owned(d_pick, f_pick, 3 * n, np.uint8, A.decide(st, luma, chroma, lam), (what, "decide"))
        base = noise(w * h * 2, seed + 7)
        d_ctrl, d_out = dev(codec, ctrl), dev(codec, base)
        run(codec, codec.alf_apply_dev, d_dec.ptr, w, h, d_map.ptr if own_map else 0, p_luma, n_luma, p_chroma, n_chroma, d_ctrl.ptr, d_out.ptr)
        _same(d_out.download(np.uint8, base.size), A.apply_tiles(oracle, dec, w, h, cmap, luma, chroma, ctrl, base), (what, "apply"))
        _owned(d_stats, f_stats, n * words_per_ctu * 4, np.int32, words, (what, "stats after the calls that read them"))
        inputs = [(d_org, org), (d_dec, dec), (d_ctrl, ctrl)] + ([(d_map, cmap)] if own_map else []) + ([(d_mask, mask)] if mask is not None else [])
        _unchanged(inputs + ([(d_luma, luma)] if n_luma else []) + ([(d_chroma, chroma)] if n_chroma else []), what)


# ---- source analysis ----------------------------------------------------------------------------------------------------------------------
def test_aq(codec):
    """the family's drivers hold every buffer between guard bands and check the guards and the inputs after each call"""
    for c in F.cases("aq"):
        w, h = c["w"], c["h"]
        tiles = F.aq_content(c)
        rec, tot = TQ.stats(codec, tiles, w, h, Q.tile_stats(tiles), guard_seed=c["seed"] % 1000)
        TQ.decide(codec, rec, tot, w, h, c["mode"], c["strength_q8"], c["qp"], c["chroma_qp_offset"], offset="d_offset" not in c["null"],
                  qps="d_qp" not in c["null"], guard_seed=c["seed"] % 1000 + 1)


# ---- lookahead ----------------------------------------------------------------------------------------------------------------------------
def test_la(codec):
    """the family's drivers hold every buffer between guard bands and check the guards and the inputs after each call"""
    for c in F.cases("la"):
        w, h, null = c["w"], c["h"], c["null"]
        tiles = F.la_content(c)
        low = L.downscale(tiles, w, h)
        cost, mode = L.intra_costs(low, w, h)
        got_low = TL.downscale(codec, tiles, w, h, low, guard_seed=c["seed"] % 1000)
        TL.intra_costs(codec, got_low, w, h, cost, mode, with_mode="d_mode" not in null)
        l0, l1, prop, aq = F.la_side(c, cost)
        rec, _ = TL.frame_cost(codec, cost, None if "d_mode" in null else mode, l0, l1, w, h, c["intra_penalty"])
        TL.propagate(codec, rec, prop, *F.la_accumulators(c, rec.size), w, h)
        TL.tree_qp(codec, rec, prop, aq, w, h, c["strength_q8"], c["qp"], c["chroma_qp_offset"], offset="d_offset" not in null, qps="d_qp" not in null)


# ---- quantiser and fused coding -----------------------------------------------------------------------------------------------------------
def test_quant(codec, oracle):
    for c in F.cases("quant"):
        w, h, seed, qp, rounding, null, what = c["w"], c["h"], c["seed"], c["qp"], c["rounding"], c["null"], F.tag(c)
        coef, lev, cls, qps = F.quant_content(c)
        n = coef.shape[0]
        cls, qps = (None if "d_class" in null else cls), (None if "d_qp" in null else qps)
        d_cls, d_qps = (None if cls is None else dev(codec, cls)), (None if qps is None else dev(codec, qps))
        p_cls, p_qps = (d_cls.ptr if d_cls else 0), (d_qps.ptr if d_qps else 0)
        for inverse, x in ((0, coef), (1, lev)):
            want = QR.quant_regions(x, bool(inverse), cls, qps, qp, rounding)
            want, want_nnz = (want, None) if inverse else want
            d_in = dev(codec, x)
            d_out, f_out = (d_in, None) if c["inplace"] else _output(codec, n * 2048, seed + 10 + inverse)
            with_nnz = not inverse and "d_nnz" not in null
            d_nnz, f_nnz = _output(codec, 4 * n, seed + 12)
            run(codec, codec.quant_regions_dev, inverse, d_in.ptr, d_out.ptr, n, p_cls, p_qps, qp, rounding, d_nnz.ptr if with_nnz else 0)
            if c["inplace"]:
                _same(d_in.download(np.int16, n * 1024), want, (what, inverse, "in place"))
            else:
                _owned(d_out, f_out, n * 2048, np.int16, want, (what, inverse))
                _unchanged([(d_in, x)], (what, inverse))
            _owned(d_nnz, f_nnz, 4 * n if with_nnz else 0, np.uint32, want_nnz if with_nnz else np.zeros(0, np.uint32), (what, inverse, "nnz"))
        _unchanged(([(d_cls, cls)] if d_cls else []) + ([(d_qps, qps)] if d_qps else []), what)
        # the fused coding call on a frame of the case's size
        cur, pred, base, frame_qps = F.quant_frames(c)
        nc = codec.ctu_count(w, h)
        frame_qps = None if "d_qp" in null else frame_qps
        want_level, want_nnz, want_recon = QR.code_ctu_tiles(oracle, cur, pred, w, h, frame_qps, qp, rounding, base=pred if c["inplace"] else base)
        d_cur, d_pred, d_fq = dev(codec, cur), dev(codec, pred), (None if frame_qps is None else dev(codec, frame_qps))
        d_recon = d_pred if c["inplace"] else dev(codec, base)
        d_level, f_level = _output(codec, nc * 12288, seed + 13)
        d_nnz, f_nnz = _output(codec, nc * 24, seed + 14)
        with_nnz = "d_nnz" not in null
        run(codec, codec.dct32_code_ctu_tiles_dev, d_cur.ptr, d_pred.ptr, w, h, d_fq.ptr if d_fq else 0, qp, rounding, d_level.ptr, d_nnz.ptr if with_nnz else 0,
             d_recon.ptr)
        _owned(d_level, f_level, nc * 12288, np.int16, want_level, (what, "fused levels"))
        _owned(d_nnz, f_nnz, nc * 24 if with_nnz else 0, np.uint32, want_nnz if with_nnz else np.zeros(0, np.uint32), (what, "fused nnz"))
        _same(d_recon.download(np.uint8, w * h * 2), want_recon, (what, "fused recon"))
        _unchanged([(d_cur, cur)] + ([] if c["inplace"] else [(d_pred, pred)]) + ([(d_fq, frame_qps)] if d_fq else []), what)


# ---- level stream -------------------------------------------------------------------------------------------------------------------------
def test_levels(codec):
    """the family's drivers hold every buffer between guard bands and check the guards, the unwritten words and the inputs"""
    for c in F.cases("levels"):
        lv, cls = F.levels_content(c)
        n, null = lv.shape[0], c["null"]
        cls = None if "d_class" in null else cls
        counts = (lv != 0).sum(1).astype(np.uint32)
        nnz = None
        if "d_nnz" not in null:                                             # counts given; every fifth one zero over whatever levels are there
            nnz = counts.copy()
            nnz[c["seed"] % 5::5] = 0
        kept = lv if nnz is None else np.where((nnz != 0)[:, None], lv, np.int16(0))
        rec, words, total = TV.pack(codec, lv, cls, nnz)
        assert int(total[1]) == n, F.tag(c)
        TV.unpack(codec, rec, words, n, cls, with_nnz="d_nnz of unpack" not in null, guard_seed=c["seed"] % 1000,
                  want=(kept, (kept != 0).sum(1).astype(np.uint32)))
        if c["cap_q8"] is not None and int(total[0]) > 0:                   # a stream too short for the frame, and what can be read back from it
            cap = max(int(total[0]) * c["cap_q8"] // 256, 1)
            rec2, words2, _ = TV.pack(codec, lv, cls, nnz, cap=cap)
            assert np.array_equal(rec2, rec), F.tag(c)
            short = np.where(TV._written_words(rec, cap), words2, np.uint16(0))
            TV.unpack(codec, rec, short, n, cls, cap=cap)
        if c["count_only"]:
            rec3, _, total3 = TV.pack(codec, lv, cls, nnz, cap=0, null_stream=True)
            assert np.array_equal(rec3, rec) and int(total3[0]) == int(total[0]), F.tag(c)


# ---- intra frame --------------------------------------------------------------------------------------------------------------------------
def _intra_case(oracle, c):
    w, h = c["w"], c["h"]
    planes = I.case(c["kind"], w, h, c["seed"] % 100000)
    qps, modes, _ = F.frame_side(c)
    return planes, I.tiles(oracle, planes, c["seed"] + 1), (None if "d_qp" in c["null"] else qps), (None if "d_mode_in" in c["null"] else modes)


def test_intra_frame(codec, oracle):
    for c in F.cases("intra_frame"):
        w, h, what = c["w"], c["h"], F.tag(c)
        planes, cur, qps, modes = _intra_case(oracle, c)
        d_cur = dev(codec, cur)
        for comp in range(3):
            want = I.refs_from_planes(planes, w, h, comp)
            d_refs, f_refs = _output(codec, want.size, c["seed"] + 2 + comp)
            run(codec, codec.intra32_refs_from_tiles_dev, d_cur.ptr, w, h, comp, d_refs.ptr)
            _owned(d_refs, f_refs, want.size, np.uint8, want, (what, "refs", comp))
        _unchanged([(d_cur, cur)], what)
        want = I.code_frame(oracle, planes, w, h, qps, c["qp"], c["rounding"], modes)
        f = TI.Frame(codec, cur, w, h, c["seed"] % 1000)
        d_qps, d_modes = (None if qps is None else dev(codec, qps)), (None if modes is None else dev(codec, modes))
        kw = dict(qps=d_qps.ptr if d_qps else 0, qp=c["qp"], rounding=c["rounding"], nnz="d_nnz" not in c["null"])
        if modes is not None and c["inplace"]:                              # d_mode == d_mode_in
            f.reset()
            f.d_mode.upload(modes)
            run(codec, f.enqueue, mode_in=f.d_mode.ptr, **kw)
            f.check(oracle, f.results(), want, what, nnz=kw["nnz"])
        else:
            f.check(oracle, f.code(mode_in=d_modes.ptr if d_modes else 0, **kw), want, what, nnz=kw["nnz"])
        _unchanged(([(d_qps, qps)] if d_qps else []) + ([(d_modes, modes)] if d_modes else []), what)


# ---- mixed frame --------------------------------------------------------------------------------------------------------------------------
def _mixed_case(codec, oracle, c):
    """(frame, keyword arguments of the statement, the input arrays or None)"""
    w, h, null = c["w"], c["h"], c["null"]
    qps, modes, kinds = F.frame_side(c)
    qps, modes, kinds = (None if "d_qp" in null else qps), (None if "d_mode_in" in null else modes), (None if "d_kind_in" in null else kinds)
    cur, pred = M.pred_planes(w, h, c["flip"], c["kind"], c["seed"] % 100000)
    f = TM.Frame(codec, oracle, cur, pred, w, h, c["seed"] % 1000)
    return f, dict(qps=qps, qp=c["qp"], rounding=c["rounding"], penalty=c["intra_penalty"], kinds_in=kinds, modes_in=modes), (qps, modes, kinds)


def test_mixed(codec, oracle):
    for c in F.cases("mixed"):
        what, null = F.tag(c), c["null"]
        f, stated, (qps, modes, kinds) = _mixed_case(codec, oracle, c)
        want = f.want(**stated)
        d_qps, d_modes, d_kinds = (None if a is None else dev(codec, a) for a in (qps, modes, kinds))
        kw = dict(qps=d_qps.ptr if d_qps else 0, qp=c["qp"], rounding=c["rounding"], penalty=c["intra_penalty"], nnz="d_nnz" not in null, cost="d_cost" not in null)
        if c["inplace"]:                                                    # d_recon == d_pred, d_kind == d_kind_in, d_mode == d_mode_in
            f.reset()
            if kinds is not None:
                f.d["kind"].upload(kinds)
            if modes is not None:
                f.d["mode"].upload(modes)
            run(codec, f.enqueue, kind_in=f.d["kind"].ptr if kinds is not None else 0, mode_in=f.d["mode"].ptr if modes is not None else 0, recon=f.d_pred.ptr, **kw)
            f.check(f.results(recon=f.d_pred), want, what, nnz=kw["nnz"], cost=kw["cost"], base=f.pred, pred_kept=False)
            _same(f.d_recon.download(np.uint8, f.base.size), f.base, (what, "the separate reconstruction buffer"))
        else:
            got = f.code(kind_in=d_kinds.ptr if d_kinds else 0, mode_in=d_modes.ptr if d_modes else 0, **kw)
            f.check(got, want, what, nnz=kw["nnz"], cost=kw["cost"])
        _unchanged([(d, a) for d, a in ((d_qps, qps), (d_modes, modes), (d_kinds, kinds)) if d is not None], what)


# ---- the level stream decodes to the reconstruction ---------------------------------------------------------------------------------------
def _decodes(codec, oracle, c, level, nnz, kinds, modes, qps, pred_planes, recon):
    """xLevelsPackGpu on the coding call's dense levels, then the numpy decoder on the records and the stream alone"""
    w, h, n = c["w"], c["h"], codec.ctu_count(c["w"], c["h"])
    rec, words, total = TV.pack(codec, level.reshape(-1, 1024), None, nnz)
    assert int(total[1]) == 6 * n, F.tag(c)
    planes, levels = _decode_ref.decode(oracle, rec, words, w, h, kinds, modes, qps, c["qp"], pred_planes)
    _same(levels, level, (F.tag(c), "the unpacked levels"))
    _same(oracle.conv_input_fmt(*planes).reshape(-1, 512)[:, :384], recon.reshape(-1, 512)[:, :384], (F.tag(c), "the rebuilt frame"))


def test_mixed_level_stream_decodes_to_the_reconstruction(codec, oracle):
    for c in F.cases("mixed"):
        f, _, (qps, modes, kinds) = _mixed_case(codec, oracle, c)
        d_qps, d_modes, d_kinds = (None if a is None else dev(codec, a) for a in (qps, modes, kinds))
        got = f.code(qps=d_qps.ptr if d_qps else 0, qp=c["qp"], rounding=c["rounding"], penalty=c["intra_penalty"], kind_in=d_kinds.ptr if d_kinds else 0,
                     mode_in=d_modes.ptr if d_modes else 0)
        _decodes(codec, oracle, c, got["level"], got["nnz"] if c["index"] % 2 else None, got["kind"], got["mode"], qps, f.pred_planes, got["recon"])


def test_intra_level_stream_decodes_to_the_reconstruction(codec, oracle):
    for c in F.cases("intra_frame"):
        planes, cur, qps, modes = _intra_case(oracle, c)
        f = TI.Frame(codec, cur, c["w"], c["h"], c["seed"] % 1000)
        d_qps, d_modes = (None if qps is None else dev(codec, qps)), (None if modes is None else dev(codec, modes))
        level, nnz, mode, recon = f.code(qps=d_qps.ptr if d_qps else 0, qp=c["qp"], rounding=c["rounding"], mode_in=d_modes.ptr if d_modes else 0)
        _decodes(codec, oracle, c, level, nnz.ravel() if c["index"] % 2 else None, np.ones_like(mode), mode, qps, None, recon)


# ---- quarter-sample motion compensation and refinement ------------------------------------------------------------------------------------
def test_qpel(codec, oracle):
    for c in F.cases("qpel"):
        w, h, seed, what = c["w"], c["h"], c["seed"], F.tag(c)
        nb = (w // 8) * (h // 8)
        (planes, mv), refine = F.qpel_content(c, oracle)
        rt, base, rec = _tiles(oracle, planes, seed + 1), sentinels(w, h, seed + 2), records(mv, 0xFFFFFFFF)   # the cost field is ignored
        d_ref, d_mv = dev(codec, rt), dev(codec, rec)
        for name, fn in (("luma", codec.motion_comp_qpel_luma_dev), ("chroma", codec.motion_comp_qpel_chroma_dev), ("both", codec.motion_comp_qpel_dev)):
            d_out = dev(codec, base)
            run(codec, fn, d_ref.ptr, d_mv.ptr, w, h, d_out.ptr)
            _same(d_out.download(np.uint8, base.size), P.mc_tiles(oracle, rt, mv, w, h, base, name), (what, name))
        _unchanged([(d_ref, rt), (d_mv, rec)], what)
        if refine is None:
            continue
        cur, ref, mv_int = refine
        want_mv, want_cost, want_costs = P.refine(oracle, cur, ref, mv_int)
        ct, rt = _tiles(oracle, (cur, *TP._chroma_for(w, h, seed + 3)), seed + 4), _tiles(oracle, (ref, *TP._chroma_for(w, h, seed + 5)), seed + 6)
        rec = records(mv_int, 0xFFFFFFFF)
        d_cur, d_ref, d_int = dev(codec, ct), dev(codec, rt), dev(codec, rec)
        d_best, f_best = (d_int, None) if c["inplace"] else _output(codec, nb * 8, seed + 7)
        d_costs, f_costs = _output(codec, nb * 196, seed + 8)
        with_costs = "d_costs" not in c["null"]
        run(codec, codec.satd_refine_qpel_from_tiles_dev, d_cur.ptr, d_ref.ptr, w, h, d_int.ptr, d_best.ptr, d_costs.ptr if with_costs else 0)
        got_mv, got_cost = TP._unpack(d_best.download(np.uint8, nb * 8), nb)
        _same(got_mv, want_mv, (what, "refined vectors"))
        _same(got_cost, want_cost, (what, "refined costs"))
        if not c["inplace"]:
            _same(d_best.download(np.uint8, f_best.size)[nb * 8:], f_best[nb * 8:], (what, "behind d_best"))
            _unchanged([(d_int, rec)], what)
        _owned(d_costs, f_costs, nb * 196 if with_costs else 0, np.uint32, want_costs if with_costs else np.zeros(0, np.uint32), (what, "d_costs"))
        _unchanged([(d_cur, ct), (d_ref, rt)], what)


# ---- bi-prediction ------------------------------------------------------------------------------------------------------------------------
def test_bipred(codec, oracle):
    for c in F.cases("bipred"):
        w, h, seed, null, what = c["w"], c["h"], c["seed"], c["null"], F.tag(c)
        nb = (w // 8) * (h // 8)
        d = F.bipred_content(c)
        wp = TB._wp(codec, d["wp"])
        # motion compensation from two references: each plane selection over a seeded pre-fill
        t0, t1, base = _tiles(oracle, d["p0"], seed + 1), _tiles(oracle, d["p1"], seed + 2), sentinels(w, h, seed + 3)
        rec0, rec1 = records(d["mv0"], 0xFFFFFFFF), records(d["mv1"], 0xFFFFFFFF)          # the cost field is ignored
        d_t0, d_t1, d_m0, d_m1 = (dev(codec, a) for a in (t0, t1, rec0, rec1))
        d_dir = None if d["direction"] is None else dev(codec, d["direction"])
        full = B.bi_tiles(oracle, t0, t1, d["mv0"], d["mv1"], d["direction"], d["wp"], w, h, base)
        for planes in (1, 2, 3):
            d_pred = dev(codec, base)
            run(codec, codec.motion_comp_bi_qpel_dev, d_t0.ptr, d_t1.ptr, d_m0.ptr, d_m1.ptr, w, h, d_pred.ptr, d_dir.ptr if d_dir else 0, wp, planes)
            _same(d_pred.download(np.uint8, base.size), TB._only(full, base, planes), (what, "planes", planes))
        _unchanged([(d_t0, t0), (d_t1, t1), (d_m0, rec0), (d_m1, rec1)] + ([(d_dir, d["direction"])] if d_dir else []), (what, "mc"))
        # the three costs and the direction; either output alone where the case draws it
        cur, ref0, ref1, mv0, mv1 = d["decision"]
        ct, r0, r1 = (_tiles(oracle, (p, *TB._chroma_for(w, h, seed + 4 + i)), seed + 7 + i) for i, p in enumerate((cur, ref0, ref1)))
        rec0, rec1 = records(mv0, 0xFFFFFFFF), records(mv1, 0xFFFFFFFF)
        want_costs, want_dir = B.costs3(oracle, cur, ref0, ref1, mv0, mv1, d["wp"], c["bi_penalty"])
        d_c, d_r0, d_r1, d_m0, d_m1 = (dev(codec, a) for a in (ct, r0, r1, rec0, rec1))
        with_costs, with_dir = "d_costs of the cost call" not in null, "d_dir of the cost call" not in null
        d_k, f_k = _output(codec, nb * 12, seed + 10)
        d_d, f_d = _output(codec, nb, seed + 11)
        run(codec, codec.satd8x8_bi_costs_dev, d_c.ptr, d_r0.ptr, d_r1.ptr, w, h, d_m0.ptr, d_m1.ptr, d_k.ptr if with_costs else 0, d_d.ptr if with_dir else 0, wp,
             c["bi_penalty"])
        _owned(d_k, f_k, nb * 12 if with_costs else 0, np.uint32, want_costs if with_costs else np.zeros(0, np.uint32), (what, "costs"))
        _owned(d_d, f_d, nb if with_dir else 0, np.uint8, want_dir if with_dir else np.zeros(0, np.uint8), (what, "direction"))
        _unchanged([(d_c, ct), (d_r0, r0), (d_r1, r1), (d_m0, rec0), (d_m1, rec1)], (what, "costs"))
        if d["refine"] is None:
            continue
        # the refinement of one list against the other; in place (d_best == d_int) where the case draws it
        cur, fix, ref, mv_fix, mv_int = d["refine"]
        want_mv, want_cost, want_all = B.refine_bi(oracle, cur, fix, mv_fix, ref, mv_int, c["list"], d["wp"])
        ct, ft, rt = (_tiles(oracle, (p, *TB._chroma_for(w, h, seed + 12 + i)), seed + 15 + i) for i, p in enumerate((cur, fix, ref)))
        rec_fix, rec_int = records(mv_fix, 0xFFFFFFFF), records(mv_int, 0xFFFFFFFF)
        d_c, d_f, d_r, d_mf, d_int = (dev(codec, a) for a in (ct, ft, rt, rec_fix, rec_int))
        d_best, f_best = (d_int, None) if c["inplace"] else _output(codec, nb * 8, seed + 18)
        d_all, f_all = _output(codec, nb * 196, seed + 19)
        with_all = "d_costs" not in null
        run(codec, codec.satd8x8_refine_bi_qpel_dev, d_c.ptr, d_f.ptr, d_mf.ptr, d_r.ptr, d_int.ptr, c["list"], w, h, d_best.ptr, d_all.ptr if with_all else 0, wp)
        got_mv, got_cost = TP._unpack(d_best.download(np.uint8, nb * 8), nb)
        _same(got_mv, want_mv, (what, "refined vectors"))
        _same(got_cost, want_cost, (what, "refined costs"))
        if not c["inplace"]:
            _same(d_best.download(np.uint8, f_best.size)[nb * 8:], f_best[nb * 8:], (what, "behind d_best"))
            _unchanged([(d_int, rec_int)], (what, "refine"))
        _owned(d_all, f_all, nb * 196 if with_all else 0, np.uint32, want_all if with_all else np.zeros(0, np.uint32), (what, "d_costs"))
        _unchanged([(d_c, ct), (d_f, ft), (d_r, rt), (d_mf, rec_fix)], (what, "refine"))


# ---- seeded search ------------------------------------------------------------------------------------------------------------------------
def test_seeded(codec, oracle):
    """the family's driver holds every buffer between guard bands and checks the guards and the inputs"""
    for c in F.cases("seeded"):
        w, h, what = c["w"], c["h"], F.tag(c)
        cur, ref, seeds = F.seeded_content(c)
        best, j, _ = E.search(oracle, cur, ref, seeds, c["seed_scale"], c["centres"], c["range"], c["lam"])
        got, got_j = TE.seeded(codec, E.tiles_of(oracle, cur, 1), E.tiles_of(oracle, ref, 2), w, h, seeds, c["seed_scale"], c["centres"], c["range"], c["lam"],
                               with_j="d_j" not in c["null"], guard_seed=c["seed"] % 1000)
        same(got, best, (what, "d_best"))
        if got_j is not None:
            same(got_j, j, (what, "d_j"))


# ---- RDOQ and the level rate ----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _case(what):
    """names the case in a failure of a family driver's own comparison"""
    try:
        yield
    except AssertionError as e:
        raise AssertionError((what,) + e.args) from None


def _same_stat(got, want, what, fields=("dist", "bits", "n_nz")):
    for field in fields:
        _same(got[field], want[field], (what, field))


def test_rdoq(codec):
    """the family's drivers hold every buffer between guard bands at its minimum alignment and check the guards and the inputs"""
    for c in F.cases("rdoq"):
        null, what = c["null"], F.tag(c)
        coef, cls, qps = F.rdoq_content(c)
        cls, qps = (None if "d_class" in null else cls), (None if "d_qp" in null else qps)
        want, want_stat, _ = RQ.rdo_quant(coef, cls, qps, c["qp"], c["lam"])
        with _case(what):
            level, nnz, stat = TR.rdoq(codec, coef, cls, qps, c["qp"], c["lam"], in_place=c["inplace"], with_nnz="d_nnz" not in null, with_stat="d_stat" not in null)
        _same(level, want, (what, "levels"))
        if nnz is not None:
            _same(nnz, want_stat["n_nz"], (what, "d_nnz"))
        if stat is not None:
            _same_stat(stat, want_stat, what)
        # the rate estimate on the levels the call produced: without counts, and with counts of which every fifth is zero over whatever levels
        counts = want_stat["n_nz"].copy()
        counts[c["seed"] % 5::5] = 0
        arbitrary = [(coef, None)] if c["kind"] in ("fullrange", "ends") else []      # the coefficients taken as levels: any int16
        for lv, given in [(level, None), (level, counts)] + arbitrary:
            with _case(what):
                got = TR.levels_bits(codec, lv, cls, given)
            _same_stat(got, RQ.levels_bits(lv, cls, given), (what, "xLevelsBitsGpu", "its own levels" if lv is level else "any int16", given is not None))


# ---- the transform decision -----------------------------------------------------------------------------------------------------------------
def test_tdecide(codec, oracle):
    """all five outputs against the composition of the two device calls it replaces on every region, and against the statement on the
    regions of F.tdecide_sample; the family's driver holds every buffer between guard bands at its minimum alignment"""
    for c in F.cases("tdecide"):
        w, h, what = c["w"], c["h"], F.tag(c)
        d = F.tdecide_content(c, oracle)
        cur, pred, kw = d["cur"], (d["cur"] if c["same_frame"] else d["pred"]), F.tdecide_args(c, d)
        sel = F.tdecide_sample(w, h)
        with _case(what):
            got = TT.decide(codec, cur, pred, w, h, without=tuple(n for n in ("d_nnz", "d_stat", "d_cost") if n in c["null"]), same_frame=c["same_frame"], **kw)
            TT._same(got, TT.compose(codec, cur, pred, w, h, **kw))
            TT._same(got, TT._ref(oracle, cur, pred, w, h, sel, **kw), sel)
