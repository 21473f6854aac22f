"""GPU (-m gpu): rate-distortion optimised quantisation and the level rate estimate (xRdoQuantRegionsGpu, xLevelsBitsGpu) against
tests/_rdoq_ref.py, bit-exact: levels, non-zero counts, distortion and bits.  Every buffer of every call sits between the guard bands
of tests/_arena.py at exactly its documented alignment; guards and inputs are checked after every call.  Before a batch is compared
with the device, the reference's own counters must show that all three steps of the optimisation fired in it (lambda > 0), so a
kernel that skips a step cannot pass."""
import ctypes
import functools

import numpy as np
import pytest

import _levels_ref as LR
import _quant_ref as Q
import _rdoq_ref as R
import x266_amd
from _arena import Arena
from _dev import EINVAL, call_struct, dev, sync_or_exit

pytestmark = pytest.mark.gpu

PTRS = {"d_coef": 16, "d_level": 16, "d_class": 1, "d_qp": 1, "d_nnz": 4, "d_stat": 8}
DISP = {name: align * (2 * i + 1) for i, (name, align) in enumerate(PTRS.items())}          # exactly the documented alignment, no more


# ---- the batches, and the reference computed once per batch -----------------------------------------------------------------------------
@functools.lru_cache(None)
def batch(n, tables, qp, lam, seed=0):
    """(coef, classes or None, qps or None, qp, lam, want levels, want stats, counters).  tables "mixed": the four classes in turn from
    32x32 down (garbage above the low two bits) and qp bytes that include 0, 51 and 200 (clamped); "none": d_class and d_qp NULL."""
    cls = qps = None
    if tables == "mixed":
        cls = ((3 - np.arange(n) % 4) | (np.arange(n) * 52 & 0xFC)).astype(np.uint8)
        qps = np.array([32, 22, 37, 27, 0, 51, 200, 30, 35], np.uint8)[np.arange(n) % 9]
    coef = R.laplacian(n, cls, qps, qp, dc_levels=3.0 if lam <= 368 else 10.0, seed=1000 * n + seed)
    want, stat, counters = R.rdo_quant(coef, cls, qps, qp, lam)
    for a in (coef, want, stat):
        a.setflags(write=False)
    return coef, cls, qps, qp, lam, want, stat, counters


def _all_steps_fired(b):
    counters, lam = b[7], b[4]
    if lam == 0:                                                            # cost = distortion: no step has anything to trade
        return
    assert counters["changed"] > 0 and counters["cg_zeroed"] > 0 and counters["last_moved"] > 0, counters


def rdoq(codec, coef, cls, qps, qp, lam, in_place=False, with_nnz=True, with_stat=True, stream=None):
    """the call inside an arena -> (levels [n, 1024], nnz or None, stats or None)"""
    coef = np.ascontiguousarray(coef, np.int16).reshape(-1, 1024)
    n = coef.shape[0]
    a, s = Arena(codec), {}
    if in_place:
        s["d_level"] = a.output("d_level", 2048 * n, 16, DISP["d_level"])
        image = s["d_level"].image.copy()                                    # the coefficients where the levels will be, between the same guards
        image[s["d_level"].start:s["d_level"].start + 2048 * n] = coef.view(np.uint8).ravel()
        s["d_level"].buf.upload(image)
        s["d_coef"] = s["d_level"]
    else:
        s["d_coef"] = a.input("d_coef", coef, 16, DISP["d_coef"], 41)
        s["d_level"] = a.output("d_level", 2048 * n, 16, DISP["d_level"])
    if cls is not None:
        s["d_class"] = a.input("d_class", np.asarray(cls, np.uint8), 1, DISP["d_class"], 42)
    if qps is not None:
        s["d_qp"] = a.input("d_qp", np.asarray(qps, np.uint8), 1, DISP["d_qp"], 43)
    if with_nnz:
        s["d_nnz"] = a.output("d_nnz", 4 * n, 4, DISP["d_nnz"])
    if with_stat:
        s["d_stat"] = a.output("d_stat", 16 * n, 8, DISP["d_stat"])
    p = codec.rdoq_params(*[s[name].ptr if name in s else 0 for name in PTRS], n_regions=n, qp=qp, lam=lam)
    call_struct(codec, "xRdoQuantRegionsGpu", p, stream)
    got = a.check()                                                         # guard bands and inputs
    return (got["d_level"].view(np.int16).reshape(n, 1024), got["d_nnz"].view(np.uint32) if with_nnz else None,
            got["d_stat"].view(R.STAT_DTYPE) if with_stat else None)


def _same(level, nnz, stat, want, want_stat):
    bad = np.flatnonzero((level != want).any(1))
    assert bad.size == 0, (bad[:8], [np.flatnonzero(level[r] != want[r])[:6] for r in bad[:2]])
    if nnz is not None:
        assert np.array_equal(nnz, want_stat["n_nz"])
    if stat is not None:
        bad = np.flatnonzero(stat != want_stat)
        assert bad.size == 0, (bad[:4], stat[bad[:4]], want_stat[bad[:4]])


BATCHES = [(1, "mixed", 0, 368), (3, "mixed", 0, 368), (4, "mixed", 0, 368), (5, "mixed", 0, 368), (257, "mixed", 0, 368),
           (5, "none", 0, 8192), (4, "none", 51, 368), (5, "mixed", 0, 0), (3, "mixed", 0, 8192), (5, "none", 30, 0)]


# ---- 1. the call against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tables,qp,lam", BATCHES)
def test_rdoq_against_the_reference(codec, n, tables, qp, lam):
    b = batch(n, tables, qp, lam)
    _all_steps_fired(b)
    coef, cls, qps, qp, lam, want, want_stat, _ = b
    level, nnz, stat = rdoq(codec, coef, cls, qps, qp, lam)
    _same(level, nnz, stat, want, want_stat)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_edge_regions(codec, k):
    """all zero, every coefficient -32768, every coefficient +32767, a single non-zero at u = v = N - 1, a single non-zero at DC: at qp 0,
    30 and 51, and at lambda 368, 0 and 8192"""
    coef = np.concatenate([R.edge_regions(k)] * 3)
    cls = np.full(15, k, np.uint8)
    qps = np.repeat(np.array([0, 30, 51], np.uint8), 5)
    for lam in (368, 0, 8192):
        want, want_stat, _ = R.rdo_quant(coef, cls, qps, 0, lam)
        assert not want[0].any() and want[1].any() and want[2].any()
        assert want[3].any() and want[4].any() and int(want_stat["n_nz"][3]) == 1 and int(want_stat["n_nz"][4]) == 1
        level, nnz, stat = rdoq(codec, coef, cls, qps, 0, lam)
        _same(level, nnz, stat, want, want_stat)


def test_ties_worked_by_hand(codec):
    """the exact ties of tests/test_rdoq_ref.py on the device, each beside its neighbour one lambda further: step 1 (the smaller level),
    step 2 (Jz == Jc stays coded), step 3 (the larger p; p over none)"""
    order32, order4 = LR.region_order(3), LR.region_order(0)
    cases = []                                                              # (class, qp, lambda, {index in the region: coefficient}, surviving levels)
    for lam, keep in ((8191, 1), (8192, 0)):
        cases.append((3, 4, lam, {order32[0, 0]: 5, order32[0, 1]: 400}, 1 + keep))   # J(1) == J(0) at DC at 8192; a later level holds the last position
    for lam, keep in ((3072, 1), (3073, 0)):
        cases.append((3, 9, lam, {order32[1, 0]: 23, order32[0, 0]: 400, order32[2, 0]: 4000}, 2 + keep))   # CG 1 between a DC and a later CG
    for lam, keep in ((1024, 2), (1025, 1)):
        cases.append((3, 4, lam, {order32[0, 0]: 4, order32[0, 2]: -4}, keep))
    for lam, keep in ((1129, 1), (1130, 0)):
        cases.append((0, 4, lam, {order4[5, 0]: 32}, keep))
    for k, qp, lam, at, keep in cases:
        coef = np.zeros((1, 1024), np.int16)
        for idx, v in at.items():
            coef[0, idx] = v
        cls = np.array([k], np.uint8)
        want, want_stat, _ = R.rdo_quant(coef, cls, None, qp, lam)
        assert int(want_stat["n_nz"][0]) == keep, (k, qp, lam, want_stat)
        _same(*rdoq(codec, coef, cls, None, qp, lam), want, want_stat)


def test_in_place_and_optional_outputs(codec):
    b = batch(5, "mixed", 0, 368)
    _all_steps_fired(b)
    coef, cls, qps, qp, lam, want, want_stat, _ = b
    out = rdoq(codec, coef, cls, qps, qp, lam)
    inp = rdoq(codec, coef, cls, qps, qp, lam, in_place=True)
    for x, y in zip(out, inp):
        assert x.tobytes() == y.tobytes()
    _same(*inp, want, want_stat)
    _same(*rdoq(codec, coef, cls, qps, qp, lam, with_nnz=False), want, want_stat)
    _same(*rdoq(codec, coef, cls, qps, qp, lam, with_stat=False), want, want_stat)
    _same(*rdoq(codec, coef, cls, qps, qp, lam, with_nnz=False, with_stat=False), want, want_stat)


def test_two_runs_on_two_streams_give_identical_bytes(codec):
    b = batch(257, "mixed", 0, 368)
    coef, cls, qps, qp, lam = b[:5]
    streams = [codec.stream_create(), codec.stream_create()]
    try:
        runs = [rdoq(codec, coef, cls, qps, qp, lam, stream=st) for st in streams]
    finally:
        for st in streams:
            codec.stream_destroy(st)
    for x, y in zip(runs[0], runs[1]):
        assert x.tobytes() == y.tobytes()


def test_both_calls_in_one_graph(codec):
    batches = [batch(5, "mixed", 0, 368), batch(5, "mixed", 0, 368, seed=1)]
    n = 5
    d_coef, d_level, d_cls, d_qp = codec.alloc(n * 2048), codec.alloc(n * 2048), codec.alloc(16), codec.alloc(16)
    d_nnz, d_stat, d_stat2 = codec.alloc(n * 4), codec.alloc(n * 16), codec.alloc(n * 16)
    p_rdoq = codec.rdoq_params(d_coef.ptr, d_level.ptr, d_cls.ptr, d_qp.ptr, d_nnz.ptr, d_stat.ptr, n, 0, 368)
    p_bits = codec.rdoq_params(0, d_level.ptr, d_cls.ptr, 0, d_nnz.ptr, d_stat2.ptr, n)
    st = codec.stream_create()
    try:
        d_coef.upload(batches[0][0])
        d_cls.upload(batches[0][1])
        d_qp.upload(batches[0][2])
        codec.graph_begin(st)
        codec.rdo_quant_dev(p_rdoq, stream=st)
        codec.levels_bits_dev(p_bits, stream=st)
        graph = codec.graph_end(st)
        try:
            for i in (1, 0):                                                 # replayed twice, on other data than it was captured with
                coef, cls, qps, _, _, want, want_stat, _ = batches[i]
                d_coef.upload(coef)
                d_cls.upload(cls)
                d_qp.upload(qps)
                d_level.upload(np.full(n * 1024, 0x5A5A, np.int16))
                codec.graph_launch(graph, st)
                sync_or_exit(codec, 0, st)
                stat2 = d_stat2.download(np.uint8, 16 * n).view(R.STAT_DTYPE)
                _same(d_level.download(np.int16, n * 1024).reshape(n, 1024), d_nnz.download(np.uint32, n),
                      d_stat.download(np.uint8, 16 * n).view(R.STAT_DTYPE), want, want_stat)
                assert np.array_equal(stat2["bits"], want_stat["bits"]) and np.array_equal(stat2["n_nz"], want_stat["n_nz"]) and not stat2["dist"].any()
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 2. the rate estimate on its own --------------------------------------------------------------------------------------------------------
def levels_bits(codec, lv, cls=None, nnz=None):
    lv = np.ascontiguousarray(lv, np.int16).reshape(-1, 1024)
    n = lv.shape[0]
    a, s = Arena(codec), {}
    s["d_level"] = a.input("d_level", lv, 16, DISP["d_level"], 51)
    if cls is not None:
        s["d_class"] = a.input("d_class", np.asarray(cls, np.uint8), 1, DISP["d_class"], 52)
    if nnz is not None:
        s["d_nnz"] = a.input("d_nnz", np.asarray(nnz, np.uint32), 4, DISP["d_nnz"], 53)
    s["d_stat"] = a.output("d_stat", 16 * n, 8, DISP["d_stat"])
    # d_coef, d_qp, qp and lambda are ignored: garbage there changes nothing
    p = codec.rdoq_params(8, s["d_level"].ptr, s["d_class"].ptr if cls is not None else 0, 3, s["d_nnz"].ptr if nnz is not None else 0, s["d_stat"].ptr,
                          n, 99, -5)
    rc = codec.L.xLevelsBitsGpu(codec.ctx, ctypes.byref(p), None)
    sync_or_exit(codec, rc)
    assert rc == 0, codec.L.xHipLastError(codec.ctx)
    return a.check()["d_stat"].view(R.STAT_DTYPE)


def test_levels_bits_on_the_calls_own_output(codec):
    coef, cls, qps, qp, lam, want, want_stat, _ = batch(257, "mixed", 0, 368)
    got = levels_bits(codec, want, cls)
    assert np.array_equal(got["bits"], want_stat["bits"]) and np.array_equal(got["n_nz"], want_stat["n_nz"]) and not got["dist"].any()
    got = levels_bits(codec, want, cls, want_stat["n_nz"])                     # with the counts the call wrote
    assert np.array_equal(got["bits"], want_stat["bits"]) and np.array_equal(got["n_nz"], want_stat["n_nz"])


def test_levels_bits_on_other_producers_levels(codec):
    coef, cls, qps = batch(5, "mixed", 0, 368)[:3]
    plain, nnz = Q.quant_regions(coef, False, cls, qps, 0, 171)
    assert np.array_equal(levels_bits(codec, plain, cls), R.levels_bits(plain, cls))
    lv, cls = LR.sparse()                                                    # any int16 level, -32768 and 32767 included, all-zero regions
    want = R.levels_bits(lv, cls)
    assert int(want["bits"].max()) > 0 and np.array_equal(levels_bits(codec, lv, cls), want)
    assert np.array_equal(levels_bits(codec, lv), R.levels_bits(lv))          # d_class NULL
    dense = LR.dense()
    assert np.array_equal(levels_bits(codec, dense, np.array([0, 1, 2], np.uint8)), R.levels_bits(dense, np.array([0, 1, 2], np.uint8)))
    # a region with d_nnz[r] == 0 is skipped and reports zeros, whatever its levels are
    counts = (lv != 0).sum(1).astype(np.uint32)
    counts[7] = 0
    assert lv[7].any()
    got = levels_bits(codec, lv, cls, counts)
    assert np.array_equal(got, R.levels_bits(lv, cls, counts)) and got[7].tolist() == (0, 0, 0)


# ---- 3. the inter chain with RDOQ in the quantiser's place --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(64, 64), (128, 64)])
def test_chain(codec, oracle, w, h):
    """xDct32FwdCtuFromTilesDev -> xRdoQuantRegionsGpu -> xQuantRegionsGpu(1) -> xDct32InvCtuToTilesDev -> xLevelsPackGpu -> xLevelsUnpackGpu
    against the numpy chain of _quant_ref, _levels_ref and _rdoq_ref; the call's d_nnz is what xDeblockGpu takes"""
    qp, lam = 30, 368
    n = codec.ctu_count(w, h)
    cur, pred = near_tiles(w, h)
    base = Q._tiles_mix(w, h, 0x7700 + w)
    coef = Q.ctu_coefficients(oracle, cur, pred, w, h)
    want, want_stat, counters = R.rdo_quant(coef, None, None, qp, lam)
    assert want.any() and counters["changed"] > 0
    want_recon = Q.recon_of_coefficients(oracle, Q.quant_regions(want, True, None, None, qp), pred, base, w, h)
    dc, dp, dr = dev(codec, cur), dev(codec, pred), dev(codec, base)
    dz, dn, ds = codec.alloc(n * 12288), codec.alloc(n * 24), codec.alloc(n * 96)
    codec.dct32_fwd_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dz.ptr)
    codec.rdo_quant_dev(codec.rdoq_params(dz.ptr, dz.ptr, 0, 0, dn.ptr, ds.ptr, 6 * n, qp, lam))
    codec.stream_sync()
    level, nnz = dz.download(np.int16, n * 6144).reshape(-1, 1024), dn.download(np.uint32, 6 * n)
    _same(level, nnz, ds.download(np.uint8, 96 * n).view(R.STAT_DTYPE), want, want_stat)
    codec.quant_regions_dev(1, dz.ptr, dz.ptr, 6 * n, 0, 0, qp, 0)
    codec.dct32_inv_ctu_to_tiles_dev(dz.ptr, dp.ptr, w, h, dr.ptr)
    codec.stream_sync()
    recon = dr.download(np.uint8, w * h * 2)
    assert np.array_equal(recon, want_recon)
    want_rec, want_words, want_total = LR.pack(want, None, want_stat["n_nz"])
    rec, words, total = codec.levels_pack(level, None, nnz)
    assert np.array_equal(rec, want_rec) and np.array_equal(words, want_words) and total.tolist() == want_total.tolist()
    back, back_nnz = codec.levels_unpack(rec, words, 6 * n)
    assert np.array_equal(back, want) and np.array_equal(back_nnz, want_stat["n_nz"])
    # the deblocking call reads the very array the call wrote
    d_out = dev(codec, recon)
    codec.deblock_dev(dr.ptr, w, h, codec.deblock_params(d_nnz=dn.ptr, qp=qp), d_out.ptr)
    codec.stream_sync()
    assert np.array_equal(d_out.download(np.uint8, w * h * 2), codec.deblock(recon, w, h, base=recon, nnz=want_stat["n_nz"], qp=qp))


def near_tiles(w, h):
    """a current frame and a prediction a few levels away from it: residuals of a useful size at qp 30"""
    rng = np.random.RandomState(w + h)
    cur = Q._tiles_mix(w, h, 0x7600 + w).reshape(-1, 512).copy()
    pred = cur.copy()
    noise = np.rint(rng.laplace(0.0, 6.0, (cur.shape[0], 384)))
    pred[:, :384] = np.clip(cur[:, :384].astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return cur.ravel(), pred.ravel()


def test_numpy_conveniences(codec):
    coef, cls, qps, qp, lam, want, want_stat, _ = batch(5, "mixed", 0, 368)
    level, nnz, stat = codec.rdo_quant(coef, cls, qps, qp, lam)
    _same(level, nnz, stat.view(R.STAT_DTYPE), want, want_stat)
    got = codec.levels_bits(level, cls, nnz).view(R.STAT_DTYPE)
    assert np.array_equal(got["bits"], want_stat["bits"]) and np.array_equal(got["n_nz"], want_stat["n_nz"])
    assert x266_amd.RDOQ_REGION_DTYPE == R.STAT_DTYPE
    assert codec.rdo_quant(np.zeros((0, 1024), np.int16))[0].shape == (0, 1024)        # n_regions == 0: nothing launched


# ---- 4. refusals through the ABI --------------------------------------------------------------------------------------------------------------
def test_argument_errors(codec):
    """every rule once per call: X266HIP_EINVAL, the call named in the error text, nothing launched, the outputs untouched"""
    L, ctx = codec.L, codec.ctx
    M = 1 << 20
    buf = codec.alloc(8 * M)
    fill = np.random.RandomState(9).randint(1, 255, 8 * M).astype(np.uint8)
    buf.upload(fill)
    n = 7
    coef, lvl, cls, qps, nnz, stat = (buf.ptr + i * M for i in range(1, 7))
    top = 2 ** 64 - 4096
    good = dict(d_coef=coef, d_level=lvl, d_class=cls, d_qp=qps, d_nnz=nnz, d_stat=stat, n_regions=n, qp=30, lam=368)
    extent = dict(d_coef=2048 * n, d_level=2048 * n, d_class=n, d_qp=n, d_nnz=4 * n, d_stat=16 * n)

    def refused(name, **change):
        p = codec.rdoq_params(**dict(good, **change))
        assert getattr(L, name)(ctx, ctypes.byref(p), None) == EINVAL, (name, change)
        assert name.encode() in L.xHipLastError(ctx), (name, change)

    for name in ("xRdoQuantRegionsGpu", "xLevelsBitsGpu"):
        assert getattr(L, name)(ctx, None, None) == EINVAL and name.encode() in L.xHipLastError(ctx)    # NULL p
        assert getattr(L, name)(None, ctypes.byref(codec.rdoq_params(**good)), None) == EINVAL
        refused(name, d_level=0)
        for field, half in (("d_level", 8), ("d_nnz", 2), ("d_stat", 4)):
            refused(name, **{field: good[field] + half})
        for field, at in (("d_level", top), ("d_class", 2 ** 64 - 1), ("d_nnz", 2 ** 64 - 4), ("d_stat", 2 ** 64 - 8)):
            refused(name, **{field: at})                                     # aligned, and the extent does not fit behind it
        refused(name, n_regions=2 ** 53)                                     # n_regions * 2048 wraps
        for other in ("d_level", "d_class", "d_nnz"):
            refused(name, d_stat=good[other] + (extent[other] - 1) // 8 * 8)   # onto the other's last bytes
            refused(name, d_stat=good[other])
    refused("xLevelsBitsGpu", d_stat=0)
    refused("xRdoQuantRegionsGpu", d_coef=0)
    refused("xRdoQuantRegionsGpu", d_coef=coef + 8)
    refused("xRdoQuantRegionsGpu", d_coef=top)
    refused("xRdoQuantRegionsGpu", d_qp=2 ** 64 - 1)
    for change in (dict(lam=-1), dict(lam=8193), dict(d_qp=0, qp=-1), dict(d_qp=0, qp=52)):
        refused("xRdoQuantRegionsGpu", **change)
    refused("xRdoQuantRegionsGpu", d_level=coef + 16)                        # any overlap other than d_level == d_coef
    refused("xRdoQuantRegionsGpu", d_level=coef + 2048 * n - 16)
    for field, other in (("d_level", "d_class"), ("d_level", "d_qp"), ("d_nnz", "d_coef"), ("d_nnz", "d_level"), ("d_nnz", "d_qp"), ("d_stat", "d_coef"),
                         ("d_stat", "d_qp"), ("d_nnz", "d_stat")):
        refused("xRdoQuantRegionsGpu", **{field: good[other] + (extent[other] - 1) // PTRS[field] * PTRS[field]})
        refused("xRdoQuantRegionsGpu", **{field: good[other]})
    sync_or_exit(codec, 0)
    assert np.array_equal(buf.download(np.uint8, 8 * M), fill)             # nothing was launched
    # the edges of what is accepted: no regions (nothing is looked at), a qp out of range beside d_qp, garbage in what xLevelsBitsGpu ignores
    for rc in (L.xRdoQuantRegionsGpu(ctx, ctypes.byref(codec.rdoq_params(n_regions=0, qp=99, lam=-1)), None),
               L.xLevelsBitsGpu(ctx, ctypes.byref(codec.rdoq_params(n_regions=0)), None)):
        sync_or_exit(codec, rc)
        assert rc == 0, L.xHipLastError(ctx)
    assert np.array_equal(buf.download(np.uint8, 8 * M), fill)
    rc = L.xRdoQuantRegionsGpu(ctx, ctypes.byref(codec.rdoq_params(**dict(good, qp=99))), None)     # qp is not looked at beside d_qp
    sync_or_exit(codec, rc)
    assert rc == 0, L.xHipLastError(ctx)
