"""GPU (-m gpu): the per-context bin statistics (xEntropyStatsLevelsGpu, xEntropyStatsSideGpu) against tests/_entropy_stats_ref.py, whose
counts are counted off the bin lists of the two coders' references -- the sum of xEntropyCountRegion / xEntropyCountSideCtu, which
tests/test_entropy_stats_ref.py holds against the same lists.  Every buffer of every call sits between the guard bands of tests/_arena.py
at exactly its documented alignment; guards, inputs and what a call must not write are checked after every call, and the stream is
synchronised (or the session ended) after every call.

The counts of regions are those of the level kernel's shape: a row is R = 32 regions, 8 to each of a workgroup's four waves: 1, 3 and 5
leave waves without a region, R + 1 a second row of one region, 2 R + 3 a third row.  Those of CTUs are lanes of a one-wave row of C = 64."""
import ctypes
import functools

import numpy as np
import pytest

import _entropy_ref as E
import _entropy_side_ref as S
import _entropy_stats_ref as R
import x266_amd.entropy as XE
from _arena import Arena
from _dev import EINVAL, call_struct, dev, same, sync_or_exit

pytestmark = pytest.mark.gpu

LEVELS, SIDE = "xEntropyStatsLevelsGpu", "xEntropyStatsSideGpu"
RR, CC = R.REGIONS_PER_ROW, R.CTUS_PER_ROW
LPTRS = {"d_level": 16, "d_class": 1, "d_nnz": 4, "d_counts": 8, "d_part": 16}
SPTRS = {"d_kind": 1, "d_mode": 1, "d_class": 1, "d_qp": 1, "d_nnz": 4, "d_counts": 8, "d_part": 16}
LDISP = {name: align * (2 * i + 1) for i, (name, align) in enumerate(LPTRS.items())}       # exactly the documented alignment, no more
SDISP = {name: align * (2 * i + 1) for i, (name, align) in enumerate(SPTRS.items())}
ARRAYS = ("d_kind", "d_mode", "d_class", "d_qp", "d_nnz")
REGION_COUNTS = [0, 1, 3, 5, RR, RR + 1, 2 * RR + 3]
CTU_COUNTS = [0, 1, 63, 64, 65, CC + 1, 2 * CC + 3]
QP, OFF = 30, -2


# ---- levels ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def level_case(n, classes, flags):
    """(levels, class bytes or None, d_nnz or None, the reference's (d_counts, d_part)), computed once, shared and left unchanged.
    flags: "none" (d_nnz NULL), "true" (the counts of non-zero levels) or "zeros" (every third region that holds levels marked empty)"""
    lv, cls, nnz = R.level_frame(n)
    cls = cls if classes else None
    if flags == "none":
        nnz = None
    elif flags == "zeros":
        nnz = nnz.copy()
        nnz[1::3] = 0
        assert n < 2 or lv[1::3].any()
        nnz.setflags(write=False)
    want = R.levels_stats(lv, cls, nnz)
    for a in want:
        a.setflags(write=False)
    return lv, cls, nnz, want


def stats_levels(codec, n, lv, cls, nnz, stream=None, guard_seed=31, encode_too=False):
    """the call inside an arena -> (d_counts [100, 2], d_part [rows, 100, 2]) and, with encode_too, the records of a count-only
    xEntropyEncodeLevelsGpu on the very same input buffers"""
    rows = R.rows(n, RR)
    a = Arena(codec)
    data = {"d_level": lv, "d_class": cls, "d_nnz": nnz}
    slots = {name: a.input(name, d, LPTRS[name], LDISP[name], guard_seed + i) for i, (name, d) in enumerate(data.items()) if n and d is not None}
    d_counts = a.output("d_counts", 1600, 8, LDISP["d_counts"])
    # with no region the call writes d_counts alone: a d_part that is handed over all the same must stay as it is
    d_part = a.output("d_part", 800 * rows, 16, LDISP["d_part"]) if n else a.output("d_part", 800, 16, LDISP["d_part"], written=np.zeros(800, bool))
    p = XE.entropy_stats_params(d_counts=d_counts.ptr, d_part=d_part.ptr, n_regions=n, **{name: s.ptr for name, s in slots.items()})
    call_struct(codec, LEVELS, p, stream)
    records = None
    if encode_too:
        d_region, d_total = a.output("d_region", 32 * n, 8, 8), a.output("d_total", 16, 8, 8)
        call_struct(codec, "xEntropyEncodeLevelsGpu", XE.entropy_params(d_region=d_region.ptr, d_total=d_total.ptr, n_regions=n,
                                                                         **{name: s.ptr for name, s in slots.items()}))
    got = a.check()
    if encode_too:
        records = got["d_region"].view(E.RECORD_DTYPE)
    return got["d_counts"].view(np.uint64).reshape(100, 2), got["d_part"].view(np.uint32).reshape(-1, 100, 2)[:rows], records


@pytest.mark.parametrize("flags", ["none", "true", "zeros"])
@pytest.mark.parametrize("classes", [True, False])
@pytest.mark.parametrize("n", REGION_COUNTS)
def test_levels(codec, n, classes, flags):
    lv, cls, nnz, (want, want_part) = level_case(n, classes, flags)
    counts, part, records = stats_levels(codec, n, lv, cls, nnz, encode_too=n > 0)
    same(counts.ravel(), want.ravel(), ("d_counts", n, classes, flags))
    same(part.ravel(), want_part.ravel(), ("d_part", n, classes, flags))
    if n:
        assert int(counts.sum()) == int(records["ctx_bins"].astype(np.uint64).sum())
    else:
        assert not counts.any() and part.size == 0
    if n == 2 * RR + 3 and classes:
        assert set(cls.tolist()) == set(R.CLASSES) and (counts.reshape(4, 25, 2).sum(axis=(1, 2)) > 0).all()      # all 13 classes, all four sizes
        assert (want > 0).sum() >= 100                                       # the reference's frame reaches most of the counters a size can reach


def test_the_special_regions_at_every_place_of_a_row(codec):
    """every special region of every size first, last and on both sides of the row boundary, one call per size"""
    for k in range(4):
        special = R.special_regions(k)
        lv = np.zeros((RR + 2, 1024), np.int16)
        for j, r in enumerate([0, RR - 1, RR, RR + 1] + list(range(1, 1 + len(special)))):
            lv[r] = special[j % len(special)][1]
        lv[RR // 2] = E.maximal()
        cls = np.full(RR + 2, k + 4 * (k & 1), np.uint8)
        want, want_part = R.levels_stats(lv, cls, None)
        counts, part, records = stats_levels(codec, RR + 2, lv, cls, None, encode_too=True)
        same(counts.ravel(), want.ravel(), ("special d_counts", k))
        same(part.ravel(), want_part.ravel(), ("special d_part", k))
        assert int(counts.sum()) == int(records["ctx_bins"].sum()) and not np.delete(counts, np.s_[25 * k:25 * k + 25], axis=0).any()


def test_levels_twice_and_in_a_graph(codec):
    """two runs between different guards give equal bytes; the call captured once and replayed twice gives them again"""
    n = 2 * RR + 3
    lv, cls, nnz, (want, want_part) = level_case(n, True, "zeros")
    first = stats_levels(codec, n, lv, cls, nnz, guard_seed=31)
    again = stats_levels(codec, n, lv, cls, nnz, guard_seed=77)
    assert first[0].tobytes() == again[0].tobytes() == want.tobytes() and first[1].tobytes() == again[1].tobytes() == want_part.tobytes()
    ins = [dev(codec, a) for a in (lv, cls, nnz)]
    sizes = (1600, 800 * R.rows(n, RR))
    bufs = [codec.alloc(s) for s in sizes]
    p = XE.entropy_stats_params(d_level=ins[0].ptr, d_class=ins[1].ptr, d_nnz=ins[2].ptr, d_counts=bufs[0].ptr, d_part=bufs[1].ptr, n_regions=n)
    fill = lambda: [b.upload(np.full(s, 0x5A, np.uint8)) for b, s in zip(bufs, sizes)]
    grab = lambda: [b.download(np.uint8, s) for b, s in zip(bufs, sizes)]
    st = codec.stream_create()
    try:
        codec.graph_begin(st)
        XE.entropy_stats_levels_dev(codec, p, stream=st)
        graph = codec.graph_end(st)
        try:
            for _ in range(2):
                fill()
                codec.graph_launch(graph, st)
                sync_or_exit(codec, 0, st)
                now = grab()
                assert now[0].tobytes() == want.tobytes() and now[1].tobytes() == want_part.tobytes()
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- side information -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def side_case(n, share):
    """(the five input arrays, the reference's (d_counts, d_part)): random_arrays with junk byte values everywhere and one CTU of the
    values the header's canonical form is stated on (mode 200, class 0xFF, qp 255, nnz 7)"""
    arrays = S.random_arrays(max(n, 1), 300 + n, share)
    arrays = tuple(a[:6 * n].copy() for a in arrays)
    if n > 2 and share < 1:
        c = n // 2
        for a, v in zip(arrays, (1, 200, 0xFF, 255, 7)):
            a[6 * c:6 * c + 6] = v
    want = R.side_stats(n, *arrays, qp=QP, off=OFF)
    for a in arrays + want:
        a.setflags(write=False)
    return arrays, want


def stats_side(codec, n, arrays, qp=QP, off=OFF, stream=None, guard_seed=41):
    rows = R.rows(n, CC)
    a = Arena(codec)
    slots = {name: a.input(name, d, SPTRS[name], SDISP[name], guard_seed + i) for i, (name, d) in enumerate(zip(ARRAYS, arrays)) if n and d is not None}
    d_counts = a.output("d_counts", 256, 8, SDISP["d_counts"])
    d_part = a.output("d_part", 128 * rows, 16, SDISP["d_part"]) if n else a.output("d_part", 128, 16, SDISP["d_part"], written=np.zeros(128, bool))
    p = XE.entropy_side_stats_params(d_counts=d_counts.ptr, d_part=d_part.ptr, n_ctu=n, qp=qp, chroma_qp_offset=off, **{name: s.ptr for name, s in slots.items()})
    call_struct(codec, SIDE, p, stream)
    got = a.check()
    return got["d_counts"].view(np.uint64).reshape(16, 2), got["d_part"].view(np.uint32).reshape(-1, 16, 2)[:rows]


@pytest.mark.parametrize("share", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("n", CTU_COUNTS)
def test_side(codec, n, share):
    arrays, (want, want_part) = side_case(n, share)
    counts, part = stats_side(codec, n, arrays)
    same(counts.ravel(), want.ravel(), ("d_counts", n, share))
    same(part.ravel(), want_part.ravel(), ("d_part", n, share))
    if share == 1.0:
        assert int(counts.sum()) == 11 * n                                   # the flat CTU: 11 zero bins


@pytest.mark.parametrize("missing", ["d_kind", "d_kind d_mode", "d_class", "d_qp", "d_nnz", "d_kind d_mode d_class d_qp d_nnz"])
def test_side_null_arrays(codec, missing):
    n = CC + 1
    arrays, _ = side_case(n, 0.5)
    given = [None if name in missing.split() else a for name, a in zip(ARRAYS, arrays)]
    want, want_part = R.side_stats(n, *given, qp=QP, off=OFF)
    counts, part = stats_side(codec, n, given)
    same(counts.ravel(), want.ravel(), ("d_counts", missing))
    same(part.ravel(), want_part.ravel(), ("d_part", missing))


def test_the_worst_ctu_at_both_ends_of_a_row(codec):
    n = 2 * CC + 3
    K, M, Z, C, Q = S.worst_ctu()
    arrays = [a.copy() for a in side_case(n, 0.5)[0]]
    for c in (0, CC - 1, CC, 2 * CC - 1, n - 1):
        for a, v in zip(arrays, (K, M, C, Q, Z)):
            a[6 * c:6 * c + 6] = v
    want, want_part = R.side_stats(n, *arrays, qp=0, off=0)
    assert int(R.ctu_counts(S.worst_ctu(), 0, 0).sum()) == 64
    counts, part = stats_side(codec, n, arrays, qp=0, off=0)
    same(counts.ravel(), want.ravel(), ("worst d_counts",))
    same(part.ravel(), want_part.ravel(), ("worst d_part",))


def test_side_counts_the_canonical_form(codec):
    """stats(input) == stats(decode(encode(input))) on junk byte values; two runs give equal bytes; a graph replays them"""
    n = 2 * CC + 3
    arrays, (want, want_part) = side_case(n, 0.5)
    coded, words, _ = XE.entropy_encode_side(codec, n, *arrays, qp=QP, chroma_qp_offset=OFF)
    back = XE.entropy_decode_side(codec, coded, words, qp=QP, chroma_qp_offset=OFF)
    assert not back[5].any() and any(not np.array_equal(a, b) for a, b in zip(arrays, back[:5]))     # the input was not canonical
    first = stats_side(codec, n, arrays, guard_seed=41)
    decoded = stats_side(codec, n, back[:5], guard_seed=91)
    assert first[0].tobytes() == decoded[0].tobytes() == want.tobytes() and first[1].tobytes() == decoded[1].tobytes() == want_part.tobytes()
    ins = [dev(codec, a) for a in arrays]
    sizes = (256, 128 * R.rows(n, CC))
    bufs = [codec.alloc(s) for s in sizes]
    p = XE.entropy_side_stats_params(d_counts=bufs[0].ptr, d_part=bufs[1].ptr, n_ctu=n, qp=QP, chroma_qp_offset=OFF, **{name: d.ptr for name, d in zip(ARRAYS, ins)})
    st = codec.stream_create()
    try:
        codec.graph_begin(st)
        XE.entropy_stats_side_dev(codec, p, stream=st)
        graph = codec.graph_end(st)
        try:
            for _ in range(2):
                for b, s in zip(bufs, sizes):
                    b.upload(np.full(s, 0x5A, np.uint8))
                codec.graph_launch(graph, st)
                sync_or_exit(codec, 0, st)
                assert bufs[0].download(np.uint8, sizes[0]).tobytes() == want.tobytes() and bufs[1].download(np.uint8, sizes[1]).tobytes() == want_part.tobytes()
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- closing the loop -----------------------------------------------------------------------------------------------------------------------------
def test_tables_from_the_devices_counts_round_trip(codec):
    """xEntropyInitFromCounts of the device's counts gives legal tables, and both coders round-trip exactly under them.  Nothing is asserted
    about the byte count: with adaptive contexts a frame's own static table winning is an observation, not a theorem"""
    n = 2 * RR + 3
    lv, cls, nnz, (want, _) = level_case(n, True, "true")
    counts, part = XE.entropy_stats_levels(codec, lv, cls, nnz)
    assert np.array_equal(counts, want) and np.array_equal(part.astype(np.uint64).sum(axis=0), want)
    table = XE.entropy_init_from_counts(counts)
    assert table.tolist() == R.init_from_counts(want) and table.min() >= 31 and table.max() <= 2017 and len(set(table.tolist())) > 20
    rec, words, total = XE.entropy_encode_levels(codec, lv, cls, nnz, init=table)
    assert int(total[1]) == n
    back, back_nnz = XE.entropy_decode_levels(codec, rec, words, classes=cls, init=table)
    assert np.array_equal(back, lv) and np.array_equal(back_nnz, nnz)
    m = 2 * CC + 3
    arrays, (swant, _) = side_case(m, 0.5)
    scounts, spart = XE.entropy_stats_side(codec, m, *arrays, qp=QP, chroma_qp_offset=OFF)
    assert np.array_equal(scounts, swant) and np.array_equal(spart.astype(np.uint64).sum(axis=0), swant)
    stable = XE.entropy_init_from_counts(scounts)
    assert stable.tolist() == R.init_from_counts(swant) and stable.min() >= 31 and stable.max() <= 2017
    coded, swords, _ = XE.entropy_encode_side(codec, m, *arrays, qp=QP, chroma_qp_offset=OFF, init=stable)
    got = XE.entropy_decode_side(codec, coded, swords, qp=QP, chroma_qp_offset=OFF, init=stable)
    plain = XE.entropy_decode_side(codec, *XE.entropy_encode_side(codec, m, *arrays, qp=QP, chroma_qp_offset=OFF)[:2], qp=QP, chroma_qp_offset=OFF)
    assert not got[5].any() and all(np.array_equal(a, b) for a, b in zip(got[:5], plain[:5]))
    # the decoder's side: the counts of what it decoded are the counts of what the encoder held
    again, _ = XE.entropy_stats_side(codec, m, *got[:5], qp=QP, chroma_qp_offset=OFF)
    assert np.array_equal(again, scounts) and np.array_equal(XE.entropy_stats_levels(codec, back, cls, back_nnz)[0], counts)


# ---- refusals through the ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", [LEVELS, SIDE])
def test_argument_errors(codec, call):
    """every rule of the header: X266HIP_EINVAL, the call named in the error text, nothing launched, the arena untouched"""
    L, ctx = codec.L, codec.ctx
    fn = getattr(L, call)
    levels = call == LEVELS
    n = RR + 1 if levels else CC + 1
    ptrs, disp = (LPTRS, LDISP) if levels else (SPTRS, SDISP)
    if levels:
        lv, cls, nnz, _ = level_case(n, True, "true")
        data = dict(d_level=lv, d_class=cls, d_nnz=nnz)
        extent = dict(d_level=2048 * n, d_class=n, d_nnz=4 * n, d_counts=1600, d_part=800 * 2)
        make, scalars = XE.entropy_stats_params, dict(n_regions=n)
    else:
        data = dict(zip(ARRAYS, side_case(n, 0.5)[0]))
        extent = dict(d_kind=6 * n, d_mode=6 * n, d_class=6 * n, d_qp=6 * n, d_nnz=24 * n, d_counts=256, d_part=128 * 2)
        make, scalars = XE.entropy_side_stats_params, dict(n_ctu=n, qp=QP, chroma_qp_offset=OFF)
    outputs = ("d_counts", "d_part")
    a = Arena(codec)
    slots = {f: a.output(f, extent[f], ptrs[f], disp[f]) if f in outputs else a.input(f, data[f], ptrs[f], disp[f], 61 + i) for i, f in enumerate(ptrs)}
    good = dict({f: s.ptr for f, s in slots.items()}, **scalars)

    def refused(**change):
        p = make(**dict(good, **change))
        assert fn(ctx, ctypes.byref(p), None) == EINVAL, change
        assert call.encode() in L.xHipLastError(ctx), change

    assert fn(ctx, None, None) == EINVAL and call.encode() in L.xHipLastError(ctx)                  # NULL p
    assert fn(None, ctypes.byref(make(**good)), None) == EINVAL
    for field in outputs + (("d_level",) if levels else ()):
        refused(**{field: 0})
    if not levels:
        refused(d_mode=0)                                                    # kinds without modes
        for v in (-1, 52):
            refused(qp=v)
            refused(qp=v, n_ctu=0)                                           # the scalars are looked at without a CTU, too
        for v in (-13, 13):
            refused(chroma_qp_offset=v)
    for field in ptrs:
        if ptrs[field] > 1:
            refused(**{field: good[field] + ptrs[field] // 2})
        refused(**{field: 2 ** 64 - ptrs[field]})                            # aligned, and the extent does not fit behind it
    refused(**{"n_regions" if levels else "n_ctu": 2 ** 62})
    for field in outputs:                                                    # an output over any other buffer of the call
        for other in ptrs:
            if other != field:
                refused(**{field: good[other] + (extent[other] - 1) // ptrs[field] * ptrs[field]})
                if good[other] % ptrs[field] == 0:
                    refused(**{field: good[other]})
    zero = dict(scalars, **{"n_regions" if levels else "n_ctu": 0})
    refused(**dict({f: 0 for f in ptrs}, **zero))                            # no unit: d_counts is still needed
    refused(**dict({f: 0 for f in ptrs}, d_counts=good["d_counts"] + 4, **zero))
    sync_or_exit(codec, 0)
    a.check_untouched()                                                     # nothing was launched
    # the edge of what is accepted: no unit and nothing but d_counts, which becomes zeros
    call_struct(codec, call, make(**dict({f: 0 for f in ptrs}, d_counts=good["d_counts"], **zero)))
    assert not slots["d_counts"].payload(np.uint64).any()
    for f in ptrs:
        if f != "d_counts":
            slots[f].check_untouched()
    if not levels:                                                           # every array NULL is a call, and modes without kinds
        call_struct(codec, call, make(**dict(good, **{f: 0 for f in ARRAYS})))
        call_struct(codec, call, make(**dict(good, d_kind=0)))


# ---- the plain-C host ------------------------------------------------------------------------------------------------------------------------
def test_plain_c_host_example():
    """host/entropy_stats_example.c: a C host without HIP headers codes two frames, derives the tables of frame 2 from frame 1's DECODED
    arrays on the decoder's side and from its own on the encoder's, and decodes frame 2 under them"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "entropy_stats_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "host"), "--no-print-directory", exe])
    out = subprocess.run([exe, "192", "128"], timeout=120, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASS" in out.stdout
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["as_expected"] is True and d["ctus"] == 6 and d["regions"] == 36 and d["tables_equal"] is True and d["tables_legal"] is True
    for frame in ("frame1", "frame2"):
        for what in ("levels", "counts", "qp", "flags"):
            assert d["%s_%s_equal" % (frame, what)] == d["regions"], (frame, what)
    assert d["frame1_level_bytes"] > 0 and d["frame2_level_bytes_derived"] > 0 and d["frame2_side_bytes_derived"] > 0
