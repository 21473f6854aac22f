"""GPU (-m gpu): the compact motion stream (xMotionPackGpu, xMotionUnpackGpu) against tests/_motion_ref.py, byte for byte: every record, the
totals, the stream's written words, and the field and level map that unpack gives back.  Every buffer of every call sits between the guard
bands of tests/_arena.py at exactly its documented alignment; the guards, the inputs and the words a call must not write are checked after
every call, and the stream is synchronised (or the session ended) after every call.

The shapes, each for what can go wrong there: 16 x 16 four existing blocks, only levels 0 and 1; 64 x 64 one whole CTU; 80 x 48 a cut CTU
column; 144 x 112 a predictor spot in another CTU and all four levels; 1104 x 16 every CTU cut; 65664 x 16 1026 CTUs, the offset scan's
second step."""
import ctypes
import functools

import numpy as np
import pytest

import _motion_ref as M
import _option_cases as O
import x266_amd.motion as X
from _arena import Arena
from _dev import EINVAL, call_struct, dev, records, same, sync_or_exit

pytestmark = pytest.mark.gpu

PACK, UNPACK = "xMotionPackGpu", "xMotionUnpackGpu"
PTRS = {"d_mv": 8, "d_level": 1, "d_ctu": 8, "d_stream": 16, "d_total": 8}
DISP = {name: align * (2 * i + 1) for i, (name, align) in enumerate(PTRS.items())}          # exactly the documented alignment, no more
SLACK = 37                                                                 # words of the stream buffer behind the total: they stay as they were


@functools.lru_cache(None)
def case(w, h, kind="tree"):
    """(mv, level, the reference's pack of them), computed once, shared and left unchanged"""
    mv, level = M.field(w, h) if kind == "tree" else M.inconsistent_field(w, h, 21)
    r = M.pack(mv, level, w, h)
    for a in (mv, level, r["ctu"], r["stream"], r["total"], r["mv"], r["level"]):
        a.setflags(write=False)
    return mv, level, r


def junk_records(mv, seed=7):
    """x266_me_result_t records of a field; cost is ignored by pack, so it is garbage"""
    return records(mv, np.random.RandomState(seed).randint(0, 1 << 32, len(mv), dtype=np.uint64).astype(np.uint32))


def pack(codec, mv, level, w, h, cap_words, written, stream=None, guard_seed=51):
    """the pack call inside an arena; cap_words None: the count-only call.  written: the leading words of d_stream the call must write --
    every other byte of the buffer must stay as it was.  -> (records, stream words or None, totals)"""
    n_ctu = M.grid(w, h)[2] * M.grid(w, h)[3]
    a = Arena(codec)
    d_mv = a.input("d_mv", junk_records(mv, guard_seed).view(np.uint8), 8, DISP["d_mv"], guard_seed)
    d_level = a.input("d_level", level, 1, DISP["d_level"], guard_seed + 1)
    d_ctu = a.output("d_ctu", 32 * n_ctu, 8, DISP["d_ctu"])
    d_total = a.output("d_total", 16, 8, DISP["d_total"])
    d_stream = None
    if cap_words:
        mask = np.zeros(2 * cap_words, bool)
        mask[:2 * written] = True
        d_stream = a.output("d_stream", 2 * cap_words, 16, DISP["d_stream"], written=mask)
    p = X.motion_params(d_mv=d_mv.ptr, d_level=d_level.ptr, d_ctu=d_ctu.ptr, d_stream=d_stream.ptr if d_stream else 0, d_total=d_total.ptr, width=w, height=h,
                        cap_words=cap_words or 0)
    call_struct(codec, PACK, p, stream)
    got = a.check()                                                         # guard bands, the inputs, and every word the call must not write
    return got["d_ctu"].view(M.CTU_DTYPE), got["d_stream"].view(np.uint16) if d_stream else None, got["d_total"].view(np.uint64)


def unpack(codec, ctu, words, w, h, cap_words, guard_seed=71):
    """the unpack call inside an arena; `words` may be longer than cap_words (what lies behind must not matter) -> (mv records, level)"""
    nb = (w // 8) * (h // 8)
    a = Arena(codec)
    d_ctu = a.input("d_ctu", ctu.view(np.uint8), 8, DISP["d_ctu"], guard_seed)
    d_stream = a.input("d_stream", np.ascontiguousarray(words, np.uint16), 16, DISP["d_stream"], guard_seed + 1) if len(words) else None
    d_mv = a.output("d_mv", 8 * nb, 8, DISP["d_mv"])
    d_level = a.output("d_level", nb, 1, DISP["d_level"])
    p = X.motion_params(d_mv=d_mv.ptr, d_level=d_level.ptr, d_ctu=d_ctu.ptr, d_stream=d_stream.ptr if d_stream else 0, width=w, height=h, cap_words=cap_words)
    call_struct(codec, UNPACK, p)
    got = a.check()
    return got["d_mv"].view(M.ME_DTYPE), got["d_level"]


def same_records(got, want, what, offsets=True):
    for f in M.CTU_DTYPE.names:
        if f != "offset" or offsets:
            same(got[f], want[f], (f,) + what)


def same_field(got_mv, got_level, mv, level, what):
    same(got_mv["mvx"], mv[:, 0], ("mvx",) + what)
    same(got_mv["mvy"], mv[:, 1], ("mvy",) + what)
    assert not got_mv["cost"].any(), what
    same(got_level, level, ("level",) + what)


# ---- 1. pack ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", M.SIZES)
def test_pack(codec, w, h):
    """d_ctu, d_total and the stream's [0, total) are the reference's; the words behind stay as they were"""
    mv, level, r = case(w, h)
    total = int(r["total"][0])
    ctu, words, tot = pack(codec, mv, level, w, h, total + SLACK, total)
    same_records(ctu, r["ctu"], (w, h))
    same(tot, r["total"], ("d_total", w, h))
    same(words[:total], r["stream"], ("d_stream", w, h))


@pytest.mark.parametrize("w,h", M.SIZES)
def test_count_only(codec, w, h):
    """cap_words == 0 with d_stream == NULL: equal records, and totals that say nothing fits"""
    mv, level, r = case(w, h)
    ctu, words, tot = pack(codec, mv, level, w, h, None, 0)
    assert words is None
    same_records(ctu, r["ctu"], (w, h))
    assert tot.tolist() == [int(r["total"][0]), 0]


@pytest.mark.parametrize("where", ["inside", "boundary"])
@pytest.mark.parametrize("w,h", M.SIZES)
def test_capacity_cut(codec, w, h, where):
    """cap_words inside the payload of the middle CTU, and exactly at its end: d_total[1], the fitting prefix, no word at or beyond cap"""
    mv, level, r = case(w, h)
    c = len(r["ctu"]) // 2
    end = int(r["ctu"]["offset"][c]) + int(r["ctu"]["n_words"][c])
    cap = end - 2 if where == "inside" else end
    fit = c if where == "inside" else c + 1
    assert int(r["ctu"]["n_words"][c]) >= 4 and M.written_words(r["ctu"], cap) == (int(r["ctu"]["offset"][c]) if where == "inside" else end)
    written = M.written_words(r["ctu"], cap)
    ctu, words, tot = pack(codec, mv, level, w, h, cap, written)              # the arena holds cap words: the word at cap is guard band
    same_records(ctu, r["ctu"], (w, h, where))
    assert tot.tolist() == [int(r["total"][0]), fit]
    same(words[:written], r["stream"][:written], ("d_stream", w, h, where))


@pytest.mark.parametrize("w,h", M.SIZES[:5])
def test_inconsistent_field(codec, w, h):
    """random vectors under a valid level map, level bytes with high bits set and bytes that disagree inside a partition: pack reads first
    blocks only, and unpack returns the canonical field"""
    mv, level, r = case(w, h, "inconsistent")
    total = int(r["total"][0])
    ctu, words, tot = pack(codec, mv, level, w, h, total, total)
    same_records(ctu, r["ctu"], (w, h))
    same(tot, r["total"], ("d_total", w, h))
    same(words, r["stream"], ("d_stream", w, h))
    got_mv, got_level = unpack(codec, ctu, words, w, h, total)
    same_field(got_mv, got_level, r["mv"], r["level"], (w, h))


# ---- 2. unpack -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", M.SIZES)
def test_unpack_of_pack(codec, w, h):
    mv, level, r = case(w, h)
    total = int(r["total"][0])
    ctu, words, _ = pack(codec, mv, level, w, h, total, total)
    got_mv, got_level = unpack(codec, ctu, words, w, h, total)
    same_field(got_mv, got_level, mv, level, (w, h))


BAD = {"bit 0 clear": 0, "a bit on a block that does not exist": 2, "heads {0, 2}": 1, "offset beyond cap": 3, "offset + size wraps": 4}


def spoil(ctu, kinds, cap):
    """the hand-made records of 144 x 112: CTU 2 is 2 blocks wide, so its block (7, 0) does not exist"""
    ctu = ctu.copy()
    for kind in kinds:
        c = BAD[kind]
        if kind == "bit 0 clear":
            ctu["head_mask"][c] &= ~np.uint64(1)
        elif kind == "a bit on a block that does not exist":
            ctu["head_mask"][c] |= np.uint64(1 << M.morton(7, 0))
        elif kind == "heads {0, 2}":
            ctu["head_mask"][c] = 0b101
        elif kind == "offset beyond cap":
            ctu["offset"][c] = cap - 3                                      # its first words lie inside, its last behind
        else:
            ctu["offset"][c] = 2 ** 64 - 2
    return ctu


@pytest.mark.parametrize("kinds", [(k,) for k in BAD] + [tuple(BAD)], ids=lambda k: k[0] if len(k) == 1 else "all")
def test_unpack_of_hand_made_records(codec, kinds):
    """each bad CTU is zeroed and the others are unaffected; whatever lies at and behind cap_words does not reach the result"""
    w, h = 144, 112
    mv, level, r = case(w, h)
    cap = int(r["total"][0])
    ctu = spoil(r["ctu"], kinds, cap)
    want_mv, want_level = M.unpack(ctu, r["stream"], w, h, cap)
    bw, cw = w // 8, M.grid(w, h)[2]
    of_block = np.array([((b // bw) >> 3) * cw + ((b % bw) >> 3) for b in range(len(level))])
    bad = np.isin(of_block, [BAD[k] for k in kinds])
    assert not want_mv[bad].any() and not want_level[bad].any() and want_mv[bad].size                # the reference zeroes exactly these ...
    assert np.array_equal(want_mv[~bad], mv[~bad]) and np.array_equal(want_level[~bad], level[~bad]) and level[bad].any()
    for poison in (0x7FFF, 0x8001):
        words = np.concatenate([r["stream"], np.full(64, poison, np.uint16)])
        got_mv, got_level = unpack(codec, ctu, words, w, h, cap, guard_seed=71 + poison)
        same_field(got_mv, got_level, want_mv, want_level, (kinds, poison))


def test_unpack_with_no_capacity(codec):
    """cap_words 0, d_stream NULL: every CTU's payload passes the capacity, the field is all zero"""
    w, h = 80, 48
    _, level, r = case(w, h)
    got_mv, got_level = unpack(codec, r["ctu"], np.zeros(0, np.uint16), w, h, 0)
    same_field(got_mv, got_level, np.zeros((len(level), 2), np.int16), np.zeros(len(level), np.uint8), ("no capacity",))


# ---- 3. the chain behind the partition decision -------------------------------------------------------------------------------------------------
def test_the_chain_behind_the_partition_decision(codec, oracle):
    """xInterPartitionDecideGpu -> pack -> unpack reproduces d_out's vectors and d_level"""
    import _partition_ref as PR
    import _seeded_ref as S
    import x266_amd.partition as P
    w, h = 144, 112
    cur, ref = PR.motion_frames(w, h, 0)
    out_mv, _, level, part_ctu, _ = P.partition_decide(codec, S.tiles_of(oracle, cur, 1).ravel(), S.tiles_of(oracle, ref, 2).ravel(), w, h, PR.motion_field(w, h, 0), 1, 4096)
    assert (np.bincount(level, minlength=4) > 0).all()
    r = M.pack(out_mv, level, w, h)
    assert np.array_equal(r["mv"], out_mv) and np.array_equal(r["level"], level)                        # the decision's field is canonical
    ctu, words, total = X.motion_pack(codec, out_mv, level, w, h)
    same_records(ctu, r["ctu"], ("chain",))
    same(words, r["stream"], ("chain stream",))
    assert total.tolist() == r["total"].tolist() and np.array_equal(ctu["parts"], part_ctu["parts"])
    got_mv, cost, got_level = X.motion_unpack(codec, ctu, words, w, h)
    assert np.array_equal(got_mv, out_mv) and np.array_equal(got_level, level) and not cost.any()
    assert np.array_equal(M.decode_differences(ctu, words, w, h), out_mv)                                # ... and decodes from words 2 and 3


# ---- 4. repeats, the launch options, a graph ----------------------------------------------------------------------------------------------------
def test_two_runs_and_every_launch_option_give_the_same_bytes(codec):
    w, h = 144, 112
    mv, level, r = case(w, h)
    total = int(r["total"][0])
    first = pack(codec, mv, level, w, h, total, total)
    again = pack(codec, mv, level, w, h, total, total, guard_seed=97)        # whatever lies around the buffers must not reach the result
    before = {k: codec.get_option(k) for k in O.VALUES}
    setting = {k: max(v for v in O.VALUES[k] if v != O.DEFAULTS[k]) for k in O.VALUES}
    setting[O.ADAPTIVE] = 0
    try:
        for k, v in setting.items():
            codec.set_option(k, v)
        assert all(codec.get_option(k) == v != O.DEFAULTS[k] for k, v in setting.items())
        other = pack(codec, mv, level, w, h, total, total)
        other_field = unpack(codec, other[0], other[1], w, h, total)
    finally:
        for k, v in before.items():
            codec.set_option(k, v)
    field = unpack(codec, first[0], first[1], w, h, total)
    for a, b, c in zip(first, again, other):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    for a, b in zip(field, other_field):
        assert a.tobytes() == b.tobytes()


def test_in_a_graph(codec):
    """pack and unpack captured once on one stream, replayed twice: the same bytes as the plain calls, which are the reference's"""
    w, h = 144, 112
    mv, level, r = case(w, h)
    nb, n_ctu, total = len(level), len(r["ctu"]), int(r["total"][0])
    d_mv, d_level = dev(codec, junk_records(mv).view(np.uint8)), dev(codec, level)
    d_ctu, d_stream, d_total, d_mv2, d_level2 = (codec.alloc(max(n, 16)) for n in (32 * n_ctu, 2 * total, 16, 8 * nb, nb))
    outs = ((d_ctu, 32 * n_ctu), (d_stream, 2 * total), (d_total, 16), (d_mv2, 8 * nb), (d_level2, nb))
    fill = lambda: [b.upload(np.full(n, 0x5A, np.uint8)) for b, n in outs]
    grab = lambda: [b.download(np.uint8, n) for b, n in outs]
    p = X.motion_params(d_mv=d_mv.ptr, d_level=d_level.ptr, d_ctu=d_ctu.ptr, d_stream=d_stream.ptr, d_total=d_total.ptr, width=w, height=h, cap_words=total)
    u = X.motion_params(d_mv=d_mv2.ptr, d_level=d_level2.ptr, d_ctu=d_ctu.ptr, d_stream=d_stream.ptr, width=w, height=h, cap_words=total)
    fill()
    codec.motion_pack_dev(p)
    codec.motion_unpack_dev(u)
    sync_or_exit(codec, 0)
    plain = grab()
    same_records(plain[0].view(M.CTU_DTYPE), r["ctu"], ("plain",))
    same(plain[1].view(np.uint16), r["stream"], ("plain stream",))
    same_field(plain[3].view(M.ME_DTYPE), plain[4], mv, level, ("plain",))
    st = codec.stream_create()
    try:
        codec.graph_begin(st)
        codec.motion_pack_dev(p, stream=st)
        codec.motion_unpack_dev(u, stream=st)
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


def test_numpy_convenience(codec):
    w, h = 80, 48
    mv, level, r = case(w, h)
    ctu, words, total = X.motion_pack(codec, mv, level, w, h)
    same_records(ctu, r["ctu"], ("numpy",))
    assert np.array_equal(words, r["stream"]) and total.tolist() == r["total"].tolist()
    cut = int(r["ctu"]["offset"][1])
    ctu, words, total = X.motion_pack(codec, mv, level, w, h, cap_words=cut + 1)
    assert total.tolist() == [int(r["total"][0]), 1] and np.array_equal(words[:cut], r["stream"][:cut]) and words[cut] == 0
    got_mv, cost, got_level = X.motion_unpack(codec, r["ctu"], r["stream"], w, h)
    assert np.array_equal(got_mv, mv) and np.array_equal(got_level, level) and not cost.any()


# ---- 5. refusals through the ABI --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", [PACK, UNPACK])
def test_argument_errors(codec, call):
    """every rule of the header: X266HIP_EINVAL, the call named in the error text, nothing launched, the arena untouched"""
    L, ctx = codec.L, codec.ctx
    fn = getattr(L, call)
    w, h = 144, 112
    mv, level, r = case(w, h)
    nb, n_ctu, cap = len(level), len(r["ctu"]), int(r["total"][0])
    extent = dict(d_mv=8 * nb, d_level=nb, d_ctu=32 * n_ctu, d_stream=2 * cap, d_total=16)
    used = [f for f in PTRS if call == PACK or f != "d_total"]
    outputs = ("d_ctu", "d_stream", "d_total") if call == PACK else ("d_mv", "d_level")
    a = Arena(codec)
    data = dict(d_mv=junk_records(mv).view(np.uint8), d_level=level, d_ctu=r["ctu"].view(np.uint8), d_stream=r["stream"])
    slots = {f: a.output(f, extent[f], PTRS[f], DISP[f]) if f in outputs else a.input(f, data[f], PTRS[f], DISP[f], 61 + i) for i, f in enumerate(used)}
    good = dict({f: s.ptr for f, s in slots.items()}, width=w, height=h, cap_words=cap)

    def refused(**change):
        p = X.motion_params(**dict(good, **change))
        assert fn(ctx, ctypes.byref(p), None) == EINVAL, change
        assert call.encode() in L.xHipLastError(ctx), change

    assert fn(ctx, None, None) == EINVAL and call.encode() in L.xHipLastError(ctx)                  # NULL p
    assert fn(None, ctypes.byref(X.motion_params(**good)), None) == EINVAL
    for field in used:
        refused(**{field: 0})                                                # d_stream too: cap_words is not 0
        if PTRS[field] > 1:
            refused(**{field: good[field] + PTRS[field] // 2})
        refused(**{field: 2 ** 64 - PTRS[field]})                            # aligned, and the extent does not fit behind it
    for side in ("width", "height"):
        for v in (0, -16, 8, 24, 152 if side == "width" else 120):
            refused(**{side: v})
    refused(cap_words=2 ** 63)                                               # no stream of that many words fits in the address space
    for field in outputs:                                                    # an output over any other buffer of the call
        for other in used:
            if other != field:
                refused(**{field: good[other] + (extent[other] - 1) // PTRS[field] * PTRS[field]})   # onto the other's last bytes
                if good[other] % PTRS[field] == 0:
                    refused(**{field: good[other]})
    sync_or_exit(codec, 0)
    a.check_untouched()                                                     # nothing was launched
    # the edge of what is accepted: no capacity and no stream
    call_struct(codec, call, X.motion_params(**dict(good, d_stream=0, cap_words=0)))
    if call == UNPACK:
        call_struct(codec, call, X.motion_params(**dict(good, d_total=3)))    # unpack does not look at d_total
    slots["d_stream"].check_untouched()


# ---- 6. the plain-C host ----------------------------------------------------------------------------------------------------------------------------
def test_plain_c_host_example():
    """host/motion_example.c: a C host without HIP headers searches, refines, decides, packs, walks the stream with the host helpers,
    rebuilds every vector from its differences, unpacks and predicts"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "motion_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "host"), "--no-print-directory", exe])
    out = subprocess.run([exe, "208", "144"], timeout=120, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["as_expected"] is True and d["blocks"] == 26 * 18 and d["ctus"] == 12
    assert d["parts"] == d["decision_parts"] < d["blocks"] and d["words"] == 4 * d["parts"] and d["rebuilt"] == d["parts"]
    assert d["unpacked_equal"] == d["blocks"] and d["bits"] > 0 and d["stream_bytes"] < d["dense_bytes"]
