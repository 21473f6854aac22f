"""The numpy convenience methods of Codec, run on the CPU against a recording stand-in for the library: which entry point each
one calls, with which scalars, which buffers (and what was uploaded to them), which NULLs, and what it hands back from what it
downloads.  The expectation, tests/golden/binding_trace.json, was recorded with this file from the x266_amd/_lib.py that wrote
every method out by hand (commit 1ccea83), so it holds the binding to those bytes whatever helpers the methods are built from.

`python tests/test_binding_trace.py --record` rewrites the golden file from the _lib.py that is checked out: do that only to add
cases for a new method, never to make a changed method pass."""
import ctypes
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from x266_amd import _lib                                                                    # noqa: E402
from x266_amd._lib import Codec, LEVEL_REGION_DTYPE, AQ_TILE_DTYPE, LA_BLOCK_DTYPE           # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_trace.json")
_BASE, _STEP = 1 << 40, 1 << 28             # fake device addresses: allocation i starts at _BASE + i * _STEP


def _digest(data):
    return hashlib.sha1(bytes(data)).hexdigest()[:12]


def _stream(tag, n):
    """n bytes that depend on `tag` alone (SHAKE-256: the same on every numpy and every machine)"""
    return hashlib.shake_256(tag.encode()).digest(n)


class _Buf:
    def __init__(self, addr, nbytes):
        self.addr, self.nbytes, self.digest, self.freed = addr, nbytes, None, False


class FakeLib:
    """Stands where Codec.L does.  Allocation, copies and the sync are played; every other x... call is written to `trace`."""

    def __init__(self, scripted=None):
        self.bufs, self.trace, self.roles, self.synced = [], [], {}, True
        self.scripted = scripted or {}          # role -> the bytes a download of that role answers with

    def _find(self, addr, nbytes):
        i = (addr - _BASE) // _STEP
        assert 0 <= i < len(self.bufs), "0x%x is no address this stand-in handed out" % addr
        off = addr - self.bufs[i].addr
        assert not self.bufs[i].freed, "allocation %d was freed (its DeviceBuffer dropped) before this use" % i
        assert off + nbytes <= self.bufs[i].nbytes, "%d bytes at offset %d of an allocation of %d" % (nbytes, off, self.bufs[i].nbytes)
        return i, off

    def xHipMalloc(self, ctx, ref, nbytes):
        self.bufs.append(_Buf(_BASE + len(self.bufs) * _STEP, int(nbytes)))
        assert 0 <= self.bufs[-1].nbytes < _STEP
        ref._obj.value = self.bufs[-1].addr
        return 0

    def xHipFree(self, ctx, ptr):
        self.bufs[self._find(ptr, 0)[0]].freed = True
        return 0

    def xHipStreamSync(self, ctx, stream):
        self.synced = True
        return 0

    def xHipLastError(self, ctx):
        return b"the stand-in has no errors"

    def xHipMemcpyH2D(self, ctx, dst, src, nbytes):
        i, off = self._find(dst, nbytes)
        assert off == 0
        self.bufs[i].digest = _digest(ctypes.string_at(src, nbytes))
        return 0

    def xHipMemcpyD2H(self, ctx, dst, src, nbytes):
        assert self.synced, "a download with no sync after the last call"
        i, off = self._find(src, nbytes)
        assert off == 0
        role = self.roles.get(i, "not in the last call")
        ctypes.memmove(dst, self.scripted.get(role) or _stream("%s/%d" % (role, nbytes), nbytes), nbytes)
        return 0

    def __getattr__(self, name):
        if not name.startswith("x"):
            raise AttributeError(name)
        return lambda *args: self._entry(name, args)

    def _entry(self, name, args):
        seen, roles = {}, {}

        def pointer(v, role):
            if v is None:
                return None
            i, off = self._find(v, 0)
            roles.setdefault(i, "%s.%s" % (name, role))
            out = {"buf": seen.setdefault(i, len(seen)), "up": self.bufs[i].digest}
            if off:
                out["off"] = off
            return out

        def field(ftype, v, role):
            if ftype is ctypes.c_void_p:
                return pointer(v, role)
            if issubclass(ftype, ctypes.Array):
                return [field(ftype._type_, e, role) for e in v]
            return int(v)

        def arg(k, a):
            if a is None:
                return None
            if isinstance(a, ctypes.c_void_p):
                return "ctx" if k == 0 else pointer(a.value, "arg%d" % k)
            if hasattr(a, "_obj"):                                              # ctypes.byref(struct)
                return {f[0]: field(f[1], getattr(a._obj, f[0]), f[0]) for f in a._obj._fields_}
            assert isinstance(a, (int, np.integer)), (name, k, a)
            return pointer(int(a), "arg%d" % k) if a >= _BASE else int(a)

        self.trace.append([name] + [arg(k, a) for k, a in enumerate(args)])
        self.roles, self.synced = roles, False
        return 0


def _value(v):
    """what a method returned, as JSON: containers by kind, arrays by dtype, shape and a digest of their bytes"""
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, np.ndarray):
        return {"dtype": str(v.dtype), "shape": list(v.shape), "sha": _digest(np.ascontiguousarray(v).tobytes())}
    if isinstance(v, ctypes.Structure):
        return {type(v).__name__: {f[0]: _value(getattr(v, f[0])) for f in v._fields_}}
    if isinstance(v, ctypes.Array):
        return [_value(e) for e in v]
    if isinstance(v, dict):
        return {"dict": {k: _value(e) for k, e in v.items()}}
    if isinstance(v, (tuple, list)):
        return {type(v).__name__: [_value(e) for e in v]}
    raise TypeError(type(v))


def _codec(lib):
    c = Codec.__new__(Codec)                    # as Codec.borrowed: no xHipCodecInit, and close() frees nothing
    c.L, c.ctx, c._borrowed = lib, ctypes.c_void_p(0xC0DEC), True
    return c


def _run(fn, scripted=None):
    lib = FakeLib(scripted)
    res = fn(_codec(lib))
    return {"trace": lib.trace, "result": _value(res)}


# ---- inputs: every array from its tag alone -----------------------------------------------------------------------------
def _arr(tag, dtype, *shape):
    dtype = np.dtype(dtype)
    return np.frombuffer(_stream(tag, int(np.prod(shape)) * dtype.itemsize), dtype).reshape(shape).copy()


def _tiles(tag, w, h):
    return _arr(tag, np.uint8, w * h // 256, 512)


def _wide(tag, dtype, *shape):
    """values of `dtype` held as int64, so that the method's own conversion decides what is uploaded"""
    return _arr(tag, dtype, *shape).astype(np.int64)


SIZES = ((64, 64), (96, 80))
NR = 3                                          # regions of the region-batch methods
WP = dict(w=((3, 5, 7), (9, 11, 13)), o=((-1, 2, -3), (4, -5, 6)), log2_denom=(5, 6))
TOTAL = np.array([40, 7], np.uint64).tobytes()  # levels_pack(cap_words=None) sizes its stream from this


def _cases():
    """[(case id, method name, function of a codec, scripted downloads or None)]"""
    out = []

    def add(method, variant, fn, scripted=None):
        out.append(("%s/%s" % (method, variant), method, fn, scripted))

    # -- region batches and the oldest methods
    refs, modes, src, ridx = _arr("refs", "u1", NR, 129), _arr("modes", "u1", NR), _arr("src", "u1", NR, 1024), _wide("ridx", "<u4", NR)
    add("intra32_predict", "plain", lambda c: c.intra32_predict(refs, modes))
    add("intra32_predict", "ref_index", lambda c: c.intra32_predict(refs[:2], modes, ridx))
    add("intra32_residual_dct32", "plain", lambda c: c.intra32_residual_dct32(refs, modes, src))
    add("intra32_residual_dct32", "ref_index", lambda c: c.intra32_residual_dct32(refs[:2], modes, src, ref_index=ridx))
    add("intra32_costs", "plain", lambda c: c.intra32_costs(refs, src))
    x = _arr("x", "<i2", NR, 1024)
    for size in (4, 32):
        for ttype in (0, 1):
            add("transform_fwd", "t%d-s%d" % (ttype, size), lambda c, t=ttype, s=size: c.transform_fwd(t, s, x))
            add("transform_inv", "t%d-s%d" % (ttype, size), lambda c, t=ttype, s=size: c.transform_inv(t, s, x))
    add("transform_fwd", "offsets", lambda c: c.transform_fwd(1, 8, x.ravel(), offsets=_wide("offs", "<u2", 5)))
    for edge in (8, 16):
        add("sad", "e%d" % edge, lambda c, e=edge: c.sad(e, _arr("sa", "u1", NR, e * e), _arr("sb", "u1", NR, e * e)))
    add("dct32_pass", "s7", lambda c: c.dct32_pass(x, 7))
    add("dct32_pass", "s12", lambda c: c.dct32_pass(x.ravel(), 12))
    cls, qps, nnz = _wide("cls", "u1", NR), _wide("qps", "u1", NR), _wide("nnz", "<u4", NR)
    for inverse in (False, True):
        add("quant_regions", "inv%d-plain" % inverse, lambda c, i=inverse: c.quant_regions(x, inverse=i))
        add("quant_regions", "inv%d-tabs" % inverse, lambda c, i=inverse: c.quant_regions(x, i, cls, qps, qp=31, rounding=2))
    add("quant_regions", "classes", lambda c: c.quant_regions(x, classes=cls))
    add("quant_regions", "qps", lambda c: c.quant_regions(x, qps=qps))
    for n in (0, NR):
        tabs = ((None, None), (cls[:n], None), (None, nnz[:n]), (cls[:n], nnz[:n])) if n else ((None, None),)
        for k, (tc, tz) in enumerate(tabs):
            v = "n%d-tabs%d" % (n, k)
            add("levels_pack", v + "-count", lambda c, n=n, tc=tc, tz=tz: c.levels_pack(x[:n], tc, tz), {"xLevelsPackGpu.d_total": TOTAL})
            add("levels_pack", v + "-cap", lambda c, n=n, tc=tc, tz=tz: c.levels_pack(x[:n], tc, tz, cap_words=24 * n))
            add("levels_bits", v, lambda c, n=n, tc=tc, tz=tz: c.levels_bits(x[:n], tc, tz))
        recs = _arr("lrec", "u1", 32 * n).view(LEVEL_REGION_DTYPE)
        add("levels_unpack", "n%d-plain" % n, lambda c, n=n, r=recs: c.levels_unpack(r, _arr("words", "<u2", 9 * n), n))
        add("levels_unpack", "n%d-classes" % n, lambda c, n=n, r=recs: c.levels_unpack(r, _arr("words", "<u2", 9 * n), n, classes=cls[:n]))
        add("rdo_quant", "n%d-plain" % n, lambda c, n=n: c.rdo_quant(x[:n]))
        add("rdo_quant", "n%d-tabs" % n, lambda c, n=n: c.rdo_quant(x[:n], cls[:n], qps[:n], qp=29, lam=400))
    add("rdo_quant", "classes", lambda c: c.rdo_quant(x, classes=cls))
    add("rdo_quant", "qps", lambda c: c.rdo_quant(x, qps=qps))
    add("sao_decide", "plain", lambda c: c.sao_decide(_arr("sst", "<i4", NR, 3, 48, 2), 37))
    st = _arr("ast", "<i4", NR, Codec.ALF_CTU_WORDS)
    add("alf_sum_stats", "plain", lambda c: c.alf_sum_stats(st))
    add("alf_sum_stats", "mask", lambda c: c.alf_sum_stats(st, _wide("mask", "u1", NR)))
    luma, chroma = _arr("luma", "u1", 2, 600), _arr("chroma", "u1", 3, 16)
    for k, (fl, fc) in enumerate(((None, None), (luma, None), (None, chroma), (luma, chroma))):
        add("alf_decide", "sets%d" % k, lambda c, fl=fl, fc=fc: c.alf_decide(st, fl, fc, 41))
    add("alf_pack_filters", "none", lambda c: c.alf_pack_filters())
    add("alf_pack_filters", "all", lambda c: c.alf_pack_filters(_arr("lc", "i1", 2, 25, 12), _arr("lk", "u1", 2, 25, 12) & 3, _arr("cc", "i1", 1, 6),
                                                                 _arr("ck", "u1", 1, 6) & 3))
    add("alf_pack_filters", "noclip", lambda c: c.alf_pack_filters(_arr("lc", "i1", 2, 25, 12), None, _arr("cc", "i1", 1, 6)))

    # -- the struct builders
    add("wp_params", "default", lambda c: c.wp_params())
    add("wp_params", "given", lambda c: c.wp_params(**WP))
    add("deblock_params", "default", lambda c: c.deblock_params())
    add("deblock_params", "given", lambda c: c.deblock_params(1, 2, 3, 4, 5, 6, 7, 8))
    add("levels_params", "default", lambda c: c.levels_params())
    add("levels_params", "given", lambda c: c.levels_params(1, 2, 3, 4, 5, 6, 7, 8))
    add("rdoq_params", "default", lambda c: c.rdoq_params())
    add("rdoq_params", "given", lambda c: c.rdoq_params(1, 2, 3, 4, 5, 6, 7, 8, 9))
    add("tdecide_params", "default", lambda c: c.tdecide_params())
    add("tdecide_params", "given", lambda c: c.tdecide_params(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, range(16, 30)))
    add("aq_params", "default", lambda c: c.aq_params())
    add("aq_params", "given", lambda c: c.aq_params(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11))
    for name, struct, scalars in (("la_params", _lib.LaParams, 6), ("seed_params", _lib.SeedParams, 6), ("mixed_params", _lib.MixedParams, 5)):
        ptrs = {f[0]: 100 + k for k, f in enumerate(struct._fields_) if f[1] is ctypes.c_void_p}
        add(name, "default", lambda c, name=name: getattr(c, name)())
        add(name, "given", lambda c, name=name, ptrs=ptrs, s=scalars: getattr(c, name)(*range(1, s + 1), **ptrs))
        add(name, "some", lambda c, name=name, ptrs=ptrs: getattr(c, name)(5, **dict(list(ptrs.items())[1::2])))
    add("ctu_count", "sizes", lambda c: [c.ctu_count(w, h) for w, h in ((64, 64), (96, 80), (65, 1), (1920, 1080))])

    # -- frames (a function, so that each size's cases keep their own arrays)
    def frames(w, h):
        sz = "%dx%d" % (w, h)
        nb, n_ctu, n16 = (w // 8) * (h // 8), Codec.ctu_count(w, h), (w // 16) * (h // 16)
        cur, ref, ref1, pred, base = (_tiles(t + sz, w, h) for t in ("cur", "ref", "ref1", "pred", "base"))
        mv, mv1 = _wide("mv" + sz, "<i2", nb, 2), _wide("mv1" + sz, "<i2", nb, 2)
        q6, k6, m6, c6 = (_wide(t + sz, "u1", n_ctu, 6) for t in ("q6", "k6", "m6", "c6"))
        z6 = _wide("z6" + sz, "<u4", n_ctu, 6)

        def add_f(method, variant, fn, scripted=None, sz=sz):
            add(method, sz + "/" + variant, fn, scripted)

        for comp in (0, 1, 2):
            add_f("intra32_refs_from_tiles", "c%d" % comp, lambda c, k=comp: c.intra32_refs_from_tiles(cur, w, h, k))
            nset = n_ctu * (4 if comp == 0 else 1)
            add_f("intra32_refs_from_tiles", "c%d-base" % comp, lambda c, k=comp, n=nset: c.intra32_refs_from_tiles(cur, w, h, k, _arr("rb" + sz, "u1", n, 144)))
        add_f("intra32_code_frame", "plain", lambda c: c.intra32_code_frame(cur, w, h))
        add_f("intra32_code_frame", "all", lambda c: c.intra32_code_frame(cur, w, h, q6, 30, 1, m6, base))
        add_f("intra32_code_frame", "qps", lambda c: c.intra32_code_frame(cur, w, h, qps=q6))
        add_f("intra32_code_frame", "modes", lambda c: c.intra32_code_frame(cur, w, h, modes_in=m6, qp=22))
        plane, refp = _arr("plane" + sz, "u1", h, w), _arr("refp" + sz, "u1", h + 8, w + 8)
        for metric in ("satd", "sad"):
            for costs in (False, True):
                v = "%s-costs%d" % (metric, costs)
                add_f("satd_search", v, lambda c, m=metric, k=costs: c.satd_search(plane, refp, 4, 2, k, m))
                add_f("search_tiles", v, lambda c, m=metric, k=costs: c.search_tiles(cur, ref, w, h, 3, k, m))
        add_f("motion_comp_luma", "plain", lambda c: c.motion_comp_luma(ref, mv, w, h))
        add_f("motion_comp_luma", "base", lambda c: c.motion_comp_luma(ref, mv, w, h, base))
        for planes in ("both", "chroma"):
            add_f("motion_comp", planes, lambda c, p=planes: c.motion_comp(ref, mv, w, h, planes=p))
            add_f("motion_comp", planes + "-base", lambda c, p=planes: c.motion_comp(ref, mv, w, h, base, p))
        for planes in ("both", "luma", "chroma"):
            add_f("motion_comp_qpel", planes, lambda c, p=planes: c.motion_comp_qpel(ref, mv, w, h, planes=p))
            add_f("motion_comp_qpel", planes + "-base", lambda c, p=planes: c.motion_comp_qpel(ref, mv, w, h, base, p))
        for costs in (False, True):
            add_f("refine_qpel_tiles", "costs%d" % costs, lambda c, k=costs: c.refine_qpel_tiles(cur, ref, w, h, mv, k))
            for wp in (False, True):
                add_f("satd8x8_refine_bi_qpel", "costs%d-wp%d" % (costs, wp),
                      lambda c, k=costs, wp=wp: c.satd8x8_refine_bi_qpel(cur, ref, mv, ref1, mv1, 1, w, h, c.wp_params(**WP) if wp else None, k))
        dirs = _wide("dirs" + sz, "u1", nb) & 3
        add_f("motion_comp_bi_qpel", "plain", lambda c: c.motion_comp_bi_qpel(ref, ref1, mv, mv1, w, h))
        add_f("motion_comp_bi_qpel", "one-ref", lambda c: c.motion_comp_bi_qpel(ref, None, mv, mv1, w, h))
        add_f("motion_comp_bi_qpel", "all", lambda c: c.motion_comp_bi_qpel(ref, ref1, mv, mv1, w, h, dirs, c.wp_params(**WP), 1, base))
        add_f("motion_comp_bi_qpel", "one-ref-base", lambda c: c.motion_comp_bi_qpel(ref, None, mv, mv1, w, h, planes=2, base=base))
        add_f("motion_comp_bi_qpel", "direction", lambda c: c.motion_comp_bi_qpel(ref, ref1, mv, mv1, w, h, direction=dirs))
        add_f("motion_comp_bi_qpel", "wp", lambda c: c.motion_comp_bi_qpel(ref, ref1, mv, mv1, w, h, wp=c.wp_params(**WP)))
        add_f("satd8x8_bi_costs", "plain", lambda c: c.satd8x8_bi_costs(cur, ref, ref1, w, h, mv, mv1))
        add_f("satd8x8_bi_costs", "wp", lambda c: c.satd8x8_bi_costs(cur, ref, ref1, w, h, mv, mv1, c.wp_params(**WP), 19))
        side = dict(cls=c6, intra=k6, nnz=z6, qps=q6, mv=mv)
        for planes in ("both", "luma", "chroma"):
            add_f("deblock", planes, lambda c, p=planes: c.deblock(cur, w, h, p))
            add_f("deblock", planes + "-all", lambda c, p=planes: c.deblock(cur, w, h, p, False, base, qp=33, beta_offset_div2=-2, tc_offset_div2=3, **side))
            add_f("deblock", planes + "-in-place", lambda c, p=planes: c.deblock(cur, w, h, p, in_place=True))
        add_f("deblock", "in-place-all", lambda c: c.deblock(cur, w, h, in_place=True, base=base, qp=27, **side))
        add_f("deblock", "base", lambda c: c.deblock(cur, w, h, base=base))
        for name in side:
            add_f("deblock", name, lambda c, name=name: c.deblock(cur, w, h, **{name: side[name]}))
        add_f("sao_stats", "plain", lambda c: c.sao_stats(cur, ref, w, h))
        add_f("sao_search", "plain", lambda c: c.sao_search(cur, ref, w, h, 45))
        add_f("sao_search", "stats", lambda c: c.sao_search(cur, ref, w, h, 45, want_stats=True))
        sao = _arr("sao" + sz, "u1", n_ctu, 3, 8)
        add_f("sao_apply", "plain", lambda c: c.sao_apply(cur, w, h, sao))
        add_f("sao_apply", "base", lambda c: c.sao_apply(cur, w, h, sao, base))
        amap, ctrl = _wide("amap" + sz, "u1", h // 4, w // 4), _wide("ctrl" + sz, "u1", n_ctu, 3)
        add_f("alf_classify", "plain", lambda c: c.alf_classify(cur, w, h))
        add_f("alf_stats", "plain", lambda c: c.alf_stats(cur, ref, w, h))
        add_f("alf_stats", "classes", lambda c: c.alf_stats(cur, ref, w, h, amap))
        for k, (fl, fc) in enumerate(((None, None), (luma, None), (None, chroma), (luma, chroma))):
            add_f("alf_apply", "sets%d" % k, lambda c, fl=fl, fc=fc: c.alf_apply(cur, w, h, fl, fc, ctrl))
        add_f("alf_apply", "all", lambda c: c.alf_apply(cur, w, h, luma, chroma, ctrl, amap, base))
        add_f("alf_apply", "classes", lambda c: c.alf_apply(cur, w, h, luma, chroma, ctrl, classes=amap))
        add_f("alf_apply", "base", lambda c: c.alf_apply(cur, w, h, luma, chroma, ctrl, base=base))
        coef = _arr("coef" + sz, "<i2", n_ctu, 6, 1024)
        add_f("transform_ctu_from_tiles", "plain", lambda c: c.transform_ctu_from_tiles(cur, pred, w, h, c6))
        add_f("transform_ctu_to_tiles", "plain", lambda c: c.transform_ctu_to_tiles(coef, c6, pred, w, h))
        add_f("transform_ctu_to_tiles", "base", lambda c: c.transform_ctu_to_tiles(coef, c6, pred, w, h, base))
        add_f("code_ctu_tiles", "plain", lambda c: c.code_ctu_tiles(cur, pred, w, h))
        add_f("code_ctu_tiles", "all", lambda c: c.code_ctu_tiles(cur, pred, w, h, q6, 28, 2, base))
        add_f("code_ctu_tiles", "qps", lambda c: c.code_ctu_tiles(cur, pred, w, h, qps=q6))
        add_f("code_ctu_tiles", "base", lambda c: c.code_ctu_tiles(cur, pred, w, h, qp=24, base=base))
        cand = _wide("cand" + sz, "<u2", 6 * n_ctu)
        add_f("transform_decide", "plain", lambda c: c.transform_decide(cur, pred, w, h))
        add_f("transform_decide", "all", lambda c: c.transform_decide(cur, pred, w, h, q6, 26, 500, 0x7, 0x70, cand, list(range(3, 16))))
        add_f("transform_decide", "qps", lambda c: c.transform_decide(cur, pred, w, h, qps=q6))
        add_f("transform_decide", "cand", lambda c: c.transform_decide(cur, pred, w, h, cand=cand))
        add_f("aq_stats", "plain", lambda c: c.aq_stats(cur, w, h))
        aq_rec, aq_tot = _arr("aqrec" + sz, "u1", 32 * n16).view(AQ_TILE_DTYPE), _arr("aqtot" + sz, "<i8", 8)
        add_f("aq_decide", "plain", lambda c: c.aq_decide(aq_rec, aq_tot, w, h))
        add_f("aq_decide", "all", lambda c: c.aq_decide(aq_rec, aq_tot, w, h, 2, 300, 35, -3))
        low = _arr("low" + sz, "u1", w * h // 2)
        h32 = h - h % 32                        # the lowres frame is handed back in whole tiles: 96 x 64 for 96 x 80
        add_f("la_downscale", "h%d" % h32, lambda c: c.la_downscale(cur[:w * h32 // 256], w, h32))
        add_f("la_intra_costs", "plain", lambda c: c.la_intra_costs(low, w, h))
        la_intra, la_mode = _wide("laintra" + sz, "<u4", n16), _wide("lamode" + sz, "u1", n16)
        in0, in1 = _arr("in0" + sz, "u1", n16, 8), _arr("in1" + sz, "<u4", n16, 2)
        add_f("la_frame_cost", "all", lambda c: c.la_frame_cost(la_intra, la_mode, in0, in1, w, h, 77))
        add_f("la_frame_cost", "intra", lambda c: c.la_frame_cost(la_intra, None, None, None, w, h))
        add_f("la_frame_cost", "mode-inter0", lambda c: c.la_frame_cost(la_intra, la_mode, in0, None, w, h))
        add_f("la_frame_cost", "inter1", lambda c: c.la_frame_cost(la_intra, None, None, in1, w, h))
        blocks = _arr("blocks" + sz, "u1", 16 * n16).view(LA_BLOCK_DTYPE)
        prop, acc0, acc1 = (_arr(t + sz, "<u8", n16) for t in ("prop", "acc0", "acc1"))
        aqo = _wide("aqo" + sz, "<i2", n16)
        add_f("la_propagate", "all", lambda c: c.la_propagate(blocks, prop, acc0, acc1, w, h))
        add_f("la_propagate", "ref0", lambda c: c.la_propagate(blocks, None, acc0, None, w, h))
        add_f("la_propagate", "prop-ref1", lambda c: c.la_propagate(blocks, prop, None, acc1, w, h))
        add_f("la_tree_qp", "all", lambda c: c.la_tree_qp(blocks, prop, aqo, w, h, 200, 34, 2))
        add_f("la_tree_qp", "plain", lambda c: c.la_tree_qp(blocks, None, None, w, h))
        add_f("la_tree_qp", "prop", lambda c: c.la_tree_qp(blocks, prop, None, w, h))
        add_f("la_tree_qp", "aq", lambda c: c.la_tree_qp(blocks, None, aqo, w, h))
        add_f("seeded_search_tiles", "plain", lambda c: c.seeded_search_tiles(cur, ref, w, h, mv))
        add_f("seeded_search_tiles", "all", lambda c: c.seeded_search_tiles(cur, ref, w, h, mv[:nb >> 2], 1, 2, 3, 21))
        add_f("code_mixed_frame", "plain", lambda c: c.code_mixed_frame(cur, pred, w, h))
        add_f("code_mixed_frame", "all", lambda c: c.code_mixed_frame(cur, pred, w, h, q6, 25, 1, 90, k6, m6, base))
        for name, tab in (("qps", q6), ("kinds_in", k6), ("modes_in", m6)):
            add_f("code_mixed_frame", name, lambda c, name=name, tab=tab: c.code_mixed_frame(cur, pred, w, h, **{name: tab}))
        add_f("code_mixed_frame", "base", lambda c: c.code_mixed_frame(cur, pred, w, h, base=base))

    for w, h in SIZES:
        frames(w, h)
    return out


CASES = _cases()

# Public callables of Codec that are no array method and have no case above.  A method whose docstring starts with "numpy
# convenience" or "Host convenience" may not stand here (test_every_method_is_covered).
NOT_TRACED = {
    "borrowed", "close", "device_info", "set_option", "get_option", "autotune_report",                       # the context, info, options
    "set_transform_matrix", "use_transform_preset", "transform_preset", "get_transform_matrix",              # options of the transforms
    "stream_create", "stream_destroy", "stream_sync", "graph_begin", "graph_end", "graph_launch", "graph_free", "time_kernel",
    "event_create", "event_destroy", "event_record", "event_elapsed_ms", "alloc", "host_alloc",
    "dct32_fwd", "dct32_inv", "satd8x8",                        # the host-pointer batch calls: no device buffer passes through Python
    "level_scan", "level_bits", "last_pos_bits", "cg_flag_bits", "weights_from_totals",                      # host-only, need the real library
}


@functools.lru_cache(None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_case_ids_are_unique_and_golden_has_no_others():
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids))
    assert set(ids) == set(_golden())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_trace_and_result_match_golden(case):
    cid, _, fn, scripted = case
    got = json.loads(json.dumps(_run(fn, scripted)))
    want = _golden()[cid]
    assert got["trace"] == want["trace"]
    assert got["result"] == want["result"]


@pytest.mark.parametrize("builder", ["la_params", "seed_params", "mixed_params"])
def test_keyword_builders_refuse_unknown_fields(builder):
    with pytest.raises(TypeError) as e:
        getattr(Codec, builder)(bogus=1, d_zzz=2)
    assert str(e.value) == "%s: no such field: ['bogus', 'd_zzz']" % builder


def test_every_method_is_covered():
    covered = {c[1] for c in CASES}
    public = {n for n in dir(Codec) if not n.startswith("_") and callable(getattr(Codec, n)) and not n.endswith("_dev")}
    assert not covered & NOT_TRACED
    assert (covered | NOT_TRACED) <= public, sorted((covered | NOT_TRACED) - public)
    assert not public - covered - NOT_TRACED, "no case and not listed: %s" % sorted(public - covered - NOT_TRACED)
    for name in NOT_TRACED:
        doc = (getattr(Codec, name).__doc__ or "").lstrip().lower()
        assert not doc.startswith(("numpy convenience", "host convenience")), name


def test_stand_in_refuses_what_does_not_fit():
    c = _codec(FakeLib())
    d = c.alloc(16)
    with pytest.raises(AssertionError):
        c.L.xHipMemcpyH2D(c.ctx, d.ptr, np.zeros(17, np.uint8).ctypes.data, 17)
    with pytest.raises(AssertionError):
        c.L.xHipMemcpyD2H(c.ctx, np.zeros(17, np.uint8).ctypes.data, d.ptr, 17)
    c.L.xSomeCallGpu(c.ctx, d.ptr, 0)
    with pytest.raises(AssertionError):                                  # no sync since the call
        d.download(np.uint8, 16)
    with pytest.raises(AssertionError):                                  # the buffer is freed with the DeviceBuffer
        c.L.xSomeCallGpu(c.ctx, c.alloc(16).ptr, 0)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(c[0]), json.dumps(_run(c[2], c[3]), separators=(",", ":"))) for c in CASES) + "\n}\n")
    print("%d cases -> %s" % (len(CASES), GOLDEN))
