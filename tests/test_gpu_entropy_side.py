"""GPU (-m gpu): the entropy coder of the side information (xEntropyEncodeSideGpu, xEntropyDecodeSideGpu) against
tests/_entropy_side_ref.py, byte for byte.  Every buffer of every call sits between the guard bands of tests/_arena.py at exactly its
documented alignment; guards, inputs and the words a call must not write are checked after every call, and the stream is synchronised
(or the session ended) after every call.

The kernels take one lane per CTU, so the counts are those of lanes: 1; 63 and 64 a wave's last lanes; 65 the first lane of a second
workgroup; 257 a fifth workgroup of one lane; 1025 a second step of the offset scan.  The data: about half flat CTUs, some all intra, qp
swinging between 0 and 51, junk byte values in every array."""
import ctypes
import functools

import numpy as np
import pytest

import _entropy_side_ref as S
import _option_cases as O
import x266_amd.entropy as XE
from _arena import Arena
from _dev import EINVAL, call_struct, dev, same, sync_or_exit

pytestmark = pytest.mark.gpu

ENC, DEC = "xEntropyEncodeSideGpu", "xEntropyDecodeSideGpu"
ARRAYS = ("d_kind", "d_mode", "d_class", "d_qp", "d_nnz")
PTRS = {"d_kind": 1, "d_mode": 1, "d_class": 1, "d_qp": 1, "d_nnz": 4, "d_coded": 8, "d_stream": 16, "d_total": 8, "d_status": 1}
DISP = {name: align * (2 * i + 1) for i, (name, align) in enumerate(PTRS.items())}          # exactly the documented alignment, no more
SLACK = 37
CUSTOM = np.array([200, 1800, 31, 2017, 900, 1500, 640, 1024, 77, 1999, 512, 1300, 333, 1700, 1100, 250], np.uint16)
COUNTS = [1, 63, 64, 65, 257, 1025]
QP, OFF = 30, -2


@functools.lru_cache(None)
def case(n, custom=False):
    """(the five input arrays, the reference's coding of them), computed once, shared and left unchanged"""
    arrays = S.random_arrays(n, 100 + n)
    want = S.encode(n, *arrays, qp=QP, off=OFF, init=CUSTOM if custom else None)
    for a in arrays + want:
        a.setflags(write=False)
    return arrays, want


def canonical(n, arrays):
    """what decode of encode must return: (kind, mode, class, qp, nnz)"""
    out = [np.zeros(6 * n, np.uint8) for _ in range(4)] + [np.zeros(6 * n, np.uint32)]
    for c, (K, M, Z, C, Q) in enumerate(S.canon_arrays(n, *arrays, qp=QP, off=OFF)):
        for a, v in zip(out, (K, M, C, Q, Z)):
            a[6 * c:6 * c + 6] = v
    return out


def encode(codec, n, arrays, cap_words, written, init=None, qp=QP, off=OFF, stream=None, guard_seed=51, unused_words=0):
    """the encode call inside an arena; cap_words None: the count-only call.  arrays: five arrays or None each.  written: boolean mask over
    the words of d_stream the call must write (or a count of leading words).  unused_words: with cap_words 0, a d_stream of that many words
    that must stay untouched.  -> (coded, stream words or None, totals)"""
    a = Arena(codec)
    slots = {name: a.input(name, data, PTRS[name], DISP[name], guard_seed + i) for i, (name, data) in enumerate(zip(ARRAYS, arrays)) if data is not None}
    d_coded = a.output("d_coded", 32 * n, 8, DISP["d_coded"])
    d_total = a.output("d_total", 16, 8, DISP["d_total"])
    d_stream = None
    if unused_words:
        d_stream = a.output("d_stream", 2 * unused_words, 16, DISP["d_stream"], written=np.zeros(2 * unused_words, bool))
    elif cap_words:
        mask = np.zeros(cap_words, bool)
        if isinstance(written, int):
            mask[:written] = True
        else:
            mask[:] = written
        d_stream = a.output("d_stream", 2 * cap_words, 16, DISP["d_stream"], written=np.repeat(mask, 2))
    table = None if init is None else np.ascontiguousarray(init, np.uint16)
    p = XE.entropy_side_params(d_coded=d_coded.ptr, d_stream=d_stream.ptr if d_stream else 0, d_total=d_total.ptr, init=table.ctypes.data if table is not None else 0,
                               n_ctu=n, cap_words=cap_words or 0, qp=qp, chroma_qp_offset=off, **{name: s.ptr for name, s in slots.items()})
    call_struct(codec, ENC, p, stream)
    got = a.check()
    return got["d_coded"].view(S.CODED_DTYPE), got["d_stream"].view(np.uint16) if d_stream else None, got["d_total"].view(np.uint64)


def decode(codec, coded, words, cap_words, init=None, qp=QP, off=OFF, outputs=ARRAYS, status=True, stream=None, guard_seed=71):
    """the decode call inside an arena; `words` may be longer than cap_words.  -> ({array name: what was written}, status or None)"""
    n = len(coded)
    a = Arena(codec)
    d_coded = a.input("d_coded", coded.view(np.uint8), 8, DISP["d_coded"], guard_seed)
    d_stream = a.input("d_stream", np.ascontiguousarray(words, np.uint16), 16, DISP["d_stream"], guard_seed + 1) if len(words) else None
    slots = {name: a.output(name, 6 * n * PTRS[name], PTRS[name], DISP[name]) for name in outputs}
    d_status = a.output("d_status", n, 1, DISP["d_status"]) if status else None
    table = None if init is None else np.ascontiguousarray(init, np.uint16)
    p = XE.entropy_side_params(d_coded=d_coded.ptr, d_stream=d_stream.ptr if d_stream else 0, d_status=d_status.ptr if d_status else 0,
                               init=table.ctypes.data if table is not None else 0, n_ctu=n, cap_words=cap_words, qp=qp, chroma_qp_offset=off,
                               **{name: s.ptr for name, s in slots.items()})
    call_struct(codec, DEC, p, stream)
    got = a.check()
    return {name: got[name].view(np.uint32 if name == "d_nnz" else np.uint8) for name in outputs}, got["d_status"] if status else None


def same_coded(got, want, what):
    for f in S.CODED_DTYPE.names:
        same(got[f], want[f], (f,) + what)


def same_arrays(got, want, what):
    for name, w in zip(ARRAYS, want):
        if name in got:
            same(got[name], w, (name,) + what)


def written_mask(coded, cap):
    mask = np.zeros(cap, bool)
    for off, nw in zip(coded["offset"].tolist(), coded["n_words"].tolist()):
        if off + nw <= cap:
            mask[off:off + nw] = True
    return mask


# ---- 1. encode ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_encode(codec, n):
    arrays, (want, stream, total) = case(n)
    words_total = int(total[0])
    coded, words, tot = encode(codec, n, arrays, words_total + SLACK, words_total)
    same_coded(coded, want, (n,))
    same(tot, total, ("d_total", n))
    same(words[:words_total], stream, ("d_stream", n))
    if n >= 257:
        flat = int((want["n_bytes"] == 0).sum())
        assert 0.35 * n < flat < 0.65 * n and (want["n_intra"] == 6).any() and want["n_bytes"].max() >= 16


@pytest.mark.parametrize("n", [65, 1025])
def test_count_only(codec, n):
    arrays, (want, _, total) = case(n)
    coded, words, tot = encode(codec, n, arrays, None, 0)
    assert words is None
    same_coded(coded, want, (n,))
    same(tot, S.encode(n, *arrays, qp=QP, off=OFF, cap_words=0)[2], ("d_total", n))


@pytest.mark.parametrize("where", ["inside", "boundary", "one word", "zero"])
@pytest.mark.parametrize("n", [65, 1025])
def test_capacity_cut(codec, n, where):
    """cap_words inside the substream of a CTU in the middle, exactly at its end, one word, and 0 with a d_stream that must stay as it is:
    the fitting ones are written, no word at or beyond cap"""
    arrays, (want, stream, total) = case(n)
    c = n // 2
    while int(want["n_words"][c]) < 2:
        c += 1
    end = int(want["offset"][c]) + int(want["n_words"][c])
    cap = {"inside": end - 1, "boundary": end, "one word": 1, "zero": 0}[where]
    _, ref_stream, ref_total = S.encode(n, *arrays, qp=QP, off=OFF, cap_words=cap)
    if where in ("inside", "boundary"):
        assert int(ref_total[1]) == (c if where == "inside" else c + 1)
    mask = written_mask(want, cap)
    coded, words, tot = encode(codec, n, arrays, cap, mask, unused_words=0 if cap else 24)
    same_coded(coded, want, (n, where))
    same(tot, ref_total, ("d_total", n, where))
    if cap:
        same(words[mask], ref_stream[mask], ("d_stream", n, where))


def test_a_maximal_ctu_between_flat_ones(codec):
    """the worst CTU that can be built at qp 0 between two flat ones, under the default table and under a table of 2017s"""
    K, M, Z, C, Q = S.worst_ctu()
    arrays = [np.array([0] * 6 + v + [0] * 6, dt) for v, dt in ((K, np.uint8), ([m if m < 255 else 0 for m in M], np.uint8), (C, np.uint8), (Q, np.uint8))]
    arrays.append(np.array([0] * 6 + Z + [0] * 6, np.uint32))
    for init in (None, np.full(16, 2017, np.uint16)):
        want, stream, total = S.encode(3, *arrays, qp=0, off=0, init=init)
        assert want["n_bytes"].tolist() == [0, 20 if init is None else 43, 0] and want["ctx_bins"][1] == 64 and want["bypass_bins"][1] == 97
        n = int(total[0])
        coded, out, tot = encode(codec, 3, arrays, n, n, init=init, qp=0, off=0)
        same_coded(coded, want, ("maximal",))
        same(out, stream, ("maximal stream",))
        got, status = decode(codec, coded, out, n, init=init, qp=0, off=0)
        same_arrays(got, S.decode(want, stream, qp=0, off=0, init=init)[:5], ("maximal decode",))
        assert not status.any() and got["d_qp"][6:12].tolist() == [51, 0, 51, 0, 51, 0]


# ---- 2. decode ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,custom", [(n, False) for n in COUNTS] + [(65, True), (1025, True)])
def test_decode_of_encode(codec, n, custom):
    """the canonical form of the input, status 0; under the default table and, at two counts, a custom one"""
    init = CUSTOM if custom else None
    arrays, (want, stream, total) = case(n, custom)
    cap = int(total[0])
    coded, words, _ = encode(codec, n, arrays, cap, cap, init=init)
    same_coded(coded, want, (n,))
    got, status = decode(codec, coded, words, cap, init=init)
    same_arrays(got, canonical(n, arrays), (n, custom))
    assert not status.any()


@pytest.mark.parametrize("n", [65, 257])
def test_decode_of_garbage(codec, n):
    """seeded garbage bytes under garbage records whose offsets and lengths lie around and beyond cap_words, the uint64 extremes included:
    every CTU is the reference's, and nothing outside [0, cap_words) is read (what lies behind is poison that would show)"""
    rs = np.random.RandomState(n)
    cap = 700
    coded = np.zeros(n, S.CODED_DTYPE)
    coded["offset"] = rs.randint(0, cap - 50, n)
    coded["n_bytes"] = rs.randint(0, 82, n)
    coded["n_words"] = rs.randint(0, 2 ** 32, n, dtype=np.uint64)           # not trusted
    special = [(cap, 0), (cap, 1), (cap - 1, 2), (cap - 1, 3), (cap + 1, 0), (2 ** 64 - 1, 2 ** 32 - 1), (2 ** 64 - 1, 0), (0, 81), (0, 2 ** 32 - 1),
               (cap - 40, 80), (cap - 39, 79), (cap - 39, 80)]
    for c, (off, nb) in enumerate(special):
        coded["offset"][c], coded["n_bytes"][c] = off, nb
    stream = rs.randint(0, 65536, cap).astype(np.uint16)
    stream[100:140] = 0xFFFF                                                # long runs of ones: the malformed prefix
    want = S.decode(coded, stream, qp=QP, off=OFF, cap_words=cap)
    assert {0, 1, 2} <= set(want[5].tolist())
    for poison in (0x7FFF, 0xFFFF):
        words = np.concatenate([stream, np.full(64, poison, np.uint16)])
        got, status = decode(codec, coded, words, cap, guard_seed=poison)
        same_arrays(got, want[:5], ("garbage", n, poison))
        same(status, want[5], ("garbage status", n, poison))


def test_a_malformed_substream_between_good_ones(codec):
    """CTU 1 of three is sixteen 0xFF bytes: the flat CTU with status 2; its neighbours decode as coded"""
    arrays, _ = case(65)
    three = [a[6 * 60:6 * 63] for a in arrays]
    want, stream, total = S.encode(3, *three, qp=QP, off=OFF)
    rec = want.copy()
    words = np.concatenate([stream[:int(rec["offset"][1])], np.full(8, 0xFFFF, np.uint16), stream[int(rec["offset"][1]) + int(rec["n_words"][1]):]])
    rec["n_bytes"][1], rec["n_words"][1] = 16, 8
    rec["offset"][2] = rec["offset"][1] + 8
    ref = S.decode(rec, words, qp=QP, off=OFF)
    flat = S.flat(QP, OFF)
    assert ref[5].tolist() == [0, 2, 0] and ref[0][6:12].tolist() == flat[0] and ref[3][6:12].tolist() == flat[4] and ref[1][6:12].tolist() == [255] * 6
    got, status = decode(codec, rec, words, len(words))
    same_arrays(got, ref[:5], ("malformed",))
    same(status, ref[5], ("malformed status",))
    got, none = decode(codec, rec, words, len(words), status=False)       # d_status NULL
    same_arrays(got, ref[:5], ("malformed, no status",))
    assert none is None


def test_decode_with_no_capacity(codec):
    """cap_words 0, d_stream NULL: every record with a length lies outside, every CTU is flat"""
    n = 65
    _, (coded, _, _) = case(n)
    ref = S.decode(coded, np.zeros(0, np.uint16), qp=QP, off=OFF, cap_words=0)
    assert set(ref[5][coded["n_bytes"] > 0].tolist()) == {1} and not ref[0].any() and not ref[4].any()
    got, status = decode(codec, coded, np.zeros(0, np.uint16), 0)
    same_arrays(got, ref[:5], ("no capacity",))
    same(status, ref[5], ("no capacity status",))


# ---- 3. NULL arrays ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", ["d_kind", "d_kind d_mode", "d_class", "d_qp", "d_nnz", "d_kind d_mode d_class d_qp d_nnz"])
def test_null_input_arrays(codec, missing):
    n = 65
    arrays, _ = case(n)
    given = [None if name in missing.split() else a for name, a in zip(ARRAYS, arrays)]
    want, stream, total = S.encode(n, *given, qp=QP, off=OFF)
    cap = int(total[0])
    coded, words, tot = encode(codec, n, given, cap, cap)
    same_coded(coded, want, (missing,))
    same(words, stream, ("d_stream", missing))
    same(tot, total, ("d_total", missing))


@pytest.mark.parametrize("asked", [("d_class",), ("d_kind", "d_nnz"), ()])
def test_null_output_arrays(codec, asked):
    n = 65
    arrays, (want, stream, total) = case(n)
    got, status = decode(codec, want, stream, int(total[0]), outputs=asked)
    same_arrays(got, canonical(n, arrays), (asked,))
    assert not status.any() and set(got) == set(asked)


# ---- 4. repeats, the launch options, a graph ------------------------------------------------------------------------------------------------------
def both(codec, n, arrays, total, guard_seed):
    coded, words, tot = encode(codec, n, arrays, total, total, guard_seed=guard_seed)
    got, status = decode(codec, coded, words, total, guard_seed=guard_seed + 9)
    return (coded, words, tot, status) + tuple(got[name] for name in ARRAYS)


def test_two_runs_and_every_launch_option_give_the_same_bytes(codec):
    n = 257
    arrays, (want, _, total) = case(n)
    cap = int(total[0])
    first = both(codec, n, arrays, cap, 51)
    again = both(codec, n, arrays, cap, 97)
    before = {k: codec.get_option(k) for k in O.VALUES}
    setting = {k: max(v for v in O.VALUES[k] if v != O.DEFAULTS[k]) for k in O.VALUES}
    setting[O.ADAPTIVE] = 0
    try:
        for k, v in setting.items():
            codec.set_option(k, v)
        assert all(codec.get_option(k) == v != O.DEFAULTS[k] for k, v in setting.items())
        other = both(codec, n, arrays, cap, 51)
    finally:
        for k, v in before.items():
            codec.set_option(k, v)
    for a, b, c in zip(first, again, other):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    same_coded(first[0], want, ("repeat",))


def test_in_a_graph(codec):
    """encode and decode captured once on one stream, replayed twice: the same bytes as the plain calls, which are the reference's"""
    n = 257
    arrays, (want, stream, total) = case(n)
    cap = int(total[0])
    ins = [dev(codec, a) for a in arrays]
    sizes = (32 * n, 2 * cap, 16, 6 * n, 6 * n, 6 * n, 6 * n, 24 * n, n)
    bufs = [codec.alloc(max(s, 16)) for s in sizes]
    outs = list(zip(bufs, sizes))
    fill = lambda: [b.upload(np.full(s, 0x5A, np.uint8)) for b, s in outs]
    grab = lambda: [b.download(np.uint8, s) for b, s in outs]
    e = XE.entropy_side_params(d_coded=bufs[0].ptr, d_stream=bufs[1].ptr, d_total=bufs[2].ptr, n_ctu=n, cap_words=cap, qp=QP, chroma_qp_offset=OFF,
                               **{name: d.ptr for name, d in zip(ARRAYS, ins)})
    d = XE.entropy_side_params(d_coded=bufs[0].ptr, d_stream=bufs[1].ptr, d_status=bufs[8].ptr, n_ctu=n, cap_words=cap, qp=QP, chroma_qp_offset=OFF,
                               **{name: b.ptr for name, b in zip(ARRAYS, bufs[3:8])})

    def calls(st=0):
        XE.entropy_encode_side_dev(codec, e, stream=st)
        XE.entropy_decode_side_dev(codec, d, stream=st)

    fill()
    calls()
    sync_or_exit(codec, 0)
    plain = grab()
    same_coded(plain[0].view(S.CODED_DTYPE), want, ("plain",))
    same(plain[1].view(np.uint16), stream, ("plain stream",))
    for got, ref in zip(plain[3:8], canonical(n, arrays)):
        same(got.view(ref.dtype), ref, ("plain decode",))
    st = codec.stream_create()
    try:
        codec.graph_begin(st)
        calls(st)
        graph = codec.graph_end(st)
        try:
            for _ in range(2):
                fill()
                codec.graph_launch(graph, st)
                sync_or_exit(codec, 0, st)
                for now, was in zip(grab(), plain):
                    assert now.tobytes() == was.tobytes()
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 5. the chain behind the mixed coding call -----------------------------------------------------------------------------------------------------
def test_the_chain_behind_the_mixed_coding_call(codec, oracle):
    """xDct32CodeMixedFrameGpu at 128 x 128 -> encode side + levels -> decode side -> xEntropyDecodeLevelsGpu with the DECODED classes: the
    levels bit for bit, the kinds and the modes"""
    import _tdecide_ref as T
    w, h, n = 128, 128, 4
    rs = np.random.RandomState(9)
    yy, xx = np.mgrid[0:h, 0:w]
    ref = [((3 * xx + 2 * yy) // 4 % 256).astype(np.uint8)] + [np.full((h // 2, w // 2), v, np.uint8) for v in (100, 140)]
    cur = [np.clip(ref[0].astype(int) + rs.randint(-9, 10, (h, w)), 0, 255).astype(np.uint8)] + \
          [np.clip(p.astype(int) + rs.randint(-6, 7, p.shape), 0, 255).astype(np.uint8) for p in ref[1:]]
    cur[0][64:, :64] = ref[0][64:, :64]                                       # CTU 2 is predicted exactly: nothing coded
    cur[1][32:, :32], cur[2][32:, :32] = ref[1][32:, :32], ref[2][32:, :32]
    kinds_in = np.full((n, 6), 2, np.uint8)
    kinds_in[1] = 1                                                           # CTU 1 all intra, CTU 3 half and half, the others decide
    kinds_in[3] = [1, 0, 0, 1, 0, 0]
    out = codec.code_mixed_frame(T.tiles_of_planes(oracle, *cur), T.tiles_of_planes(oracle, *ref), w, h, qp=QP, kinds_in=kinds_in)
    level, kind, mode, nnz = (np.asarray(out[k]) for k in ("levels", "kinds", "modes", "nnz"))
    assert kind.any() and not kind.all() and (nnz == 0).any()
    levels = level.reshape(-1, 1024)
    lrec, lstream, _ = XE.entropy_encode_levels(codec, levels, None, nnz)
    coded, stream, total = XE.entropy_encode_side(codec, n, kind, mode, None, None, nnz, qp=QP, chroma_qp_offset=0)
    want, want_stream, want_total = S.encode(n, kind, mode, None, None, nnz, qp=QP, off=0)
    same_coded(coded, want, ("chain",))
    same(stream, want_stream, ("chain stream",))
    k2, m2, c2, q2, z2, status = XE.entropy_decode_side(codec, coded, stream, qp=QP, chroma_qp_offset=0)
    K = np.array([x for ctu in S.canon_arrays(n, kind, mode, None, None, nnz, QP, 0) for x in ctu[0]], np.uint8)
    M = np.array([x for ctu in S.canon_arrays(n, kind, mode, None, None, nnz, QP, 0) for x in ctu[1]], np.uint8)
    assert not status.any() and np.array_equal(k2, K) and np.array_equal(m2, M) and np.array_equal(z2, (nnz.ravel() != 0).astype(np.uint32))
    luma = np.arange(6 * n) % 6 < 4
    assert np.array_equal(k2[luma], (kind.ravel()[luma] != 0).astype(np.uint8)) and np.array_equal(m2[luma & (k2 == 1)], mode.ravel()[luma & (k2 == 1)])
    assert set(c2.tolist()) == {3} and set(q2.tolist()) == {QP}
    back, back_nnz = XE.entropy_decode_levels(codec, lrec, lstream, classes=c2)
    assert np.array_equal(back, levels) and np.array_equal(back_nnz != 0, nnz.ravel() != 0)


def test_numpy_convenience(codec):
    n = 63
    arrays, (want, stream, total) = case(n)
    coded, words, tot = XE.entropy_encode_side(codec, n, *arrays, qp=QP, chroma_qp_offset=OFF)
    same_coded(coded, want, ("numpy",))
    assert np.array_equal(words, stream) and tot.tolist() == total.tolist()
    coded2, words2, _ = XE.entropy_encode_side(codec, n, *arrays, qp=QP, chroma_qp_offset=OFF, init=CUSTOM)
    got = XE.entropy_decode_side(codec, coded2, words2, qp=QP, chroma_qp_offset=OFF, init=CUSTOM)
    for a, b in zip(got[:5], canonical(n, arrays)):
        assert np.array_equal(a, b)
    assert not got[5].any()
    c = 7
    data, n_bytes, ctx_bins, bypass_bins = XE.entropy_encode_side_ctu(*[a[6 * c:6 * c + 6] for a in arrays], qp=QP, chroma_qp_offset=OFF)
    off = int(want["offset"][c])
    assert (n_bytes, ctx_bins, bypass_bins) == (want["n_bytes"][c], want["ctx_bins"][c], want["bypass_bins"][c])
    assert data == stream[off:off + int(want["n_words"][c])].astype("<u2").tobytes()[:n_bytes]


# ---- 6. refusals through the ABI ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", [ENC, DEC])
def test_argument_errors(codec, call):
    """every rule of the header: X266HIP_EINVAL, the call named in the error text, nothing launched, the arena untouched"""
    L, ctx = codec.L, codec.ctx
    fn = getattr(L, call)
    n = 65
    arrays, (coded, stream, total) = case(n)
    cap = int(total[0])
    extent = dict(d_kind=6 * n, d_mode=6 * n, d_class=6 * n, d_qp=6 * n, d_nnz=24 * n, d_coded=32 * n, d_stream=2 * cap, d_total=16, d_status=n)
    used = [f for f in PTRS if (call == ENC and f != "d_status") or (call == DEC and f != "d_total")]
    outputs = ("d_coded", "d_stream", "d_total") if call == ENC else ARRAYS + ("d_status",)
    required = ("d_coded", "d_stream", "d_total") if call == ENC else ("d_coded", "d_stream")
    data = dict(zip(ARRAYS, arrays), d_coded=coded.view(np.uint8), d_stream=stream)
    a = Arena(codec)
    slots = {f: a.output(f, extent[f], PTRS[f], DISP[f]) if f in outputs else a.input(f, data[f], PTRS[f], DISP[f], 61 + i) for i, f in enumerate(used)}
    table = CUSTOM.copy()
    good = dict({f: s.ptr for f, s in slots.items()}, init=table.ctypes.data, n_ctu=n, cap_words=cap, qp=QP, chroma_qp_offset=OFF)

    def refused(**change):
        p = XE.entropy_side_params(**dict(good, **change))
        assert fn(ctx, ctypes.byref(p), None) == EINVAL, change
        assert call.encode() in L.xHipLastError(ctx), change

    assert fn(ctx, None, None) == EINVAL and call.encode() in L.xHipLastError(ctx)                  # NULL p
    assert fn(None, ctypes.byref(XE.entropy_side_params(**good)), None) == EINVAL
    for field in required:
        refused(**{field: 0})
    if call == ENC:
        refused(d_mode=0)                                                    # kinds without modes
    for field in used:
        if PTRS[field] > 1:
            refused(**{field: good[field] + PTRS[field] // 2})
        refused(**{field: 2 ** 64 - PTRS[field]})                            # aligned, and the extent does not fit behind it
    for v in (-1, 52):
        refused(qp=v)
    for v in (-13, 13):
        refused(chroma_qp_offset=v)
    refused(cap_words=2 ** 63)
    refused(n_ctu=2 ** 62)
    for at, v in ((0, 30), (15, 2018), (3, 0), (9, 65535)):
        bad = CUSTOM.copy()
        bad[at] = v
        refused(init=bad.ctypes.data)
    for field in outputs:                                                    # an output over any other buffer of the call
        for other in used:
            if other != field:
                refused(**{field: good[other] + (extent[other] - 1) // PTRS[field] * PTRS[field]})
                if good[other] % PTRS[field] == 0:
                    refused(**{field: good[other]})
    sync_or_exit(codec, 0)
    a.check_untouched()                                                     # nothing was launched
    # the edge of what is accepted: no capacity and no stream; decode without d_status and whatever d_total is; no CTU at all
    call_struct(codec, call, XE.entropy_side_params(**dict(good, d_stream=0, cap_words=0)))
    if call == DEC:
        call_struct(codec, call, XE.entropy_side_params(**dict(good, d_total=3, d_status=0)))
        call_struct(codec, call, XE.entropy_side_params(n_ctu=0, qp=QP))
    else:
        call_struct(codec, call, XE.entropy_side_params(d_total=good["d_total"], n_ctu=0, qp=QP))
        assert slots["d_total"].payload(np.uint64).tolist() == [0, 0]
    slots["d_stream"].check_untouched()


# ---- 7. the plain-C host ------------------------------------------------------------------------------------------------------------------------
def test_plain_c_host_example():
    """host/entropy_side_example.c: a C host without HIP headers codes a frame with a moved block under an adaptive qp map, encodes levels
    and side information, copies records and bytes out and in, decodes the side stream, then the levels with the decoded classes, and
    dequantises with the decoded qp"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "entropy_side_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "host"), "--no-print-directory", exe])
    out = subprocess.run([exe, "192", "128"], timeout=120, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASS" in out.stdout
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["as_expected"] is True and d["ctus"] == 6 and d["regions"] == 36
    assert d["levels_equal"] == d["regions"] and d["kinds_equal"] == d["regions"] and d["modes_equal"] == d["regions"] and d["flags_equal"] == d["regions"]
    assert d["qp_equal"] == d["regions"] and d["coef_equal"] is True and d["host_bytes_equal"] == d["ctus"]
    assert d["intra_regions"] > 0 and d["side_bytes"] > 0 and d["level_bytes"] > 0
