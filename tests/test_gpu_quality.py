"""GPU (-m gpu): frame quality (xQualityStatsGpu, and xQualityFromTotals behind it) against tests/_quality_ref.py, bit-exact.  Every buffer
of every call sits between the guard bands of tests/_arena.py at exactly its documented alignment; the guards and the inputs are checked
after every call."""
import ctypes
import functools

import numpy as np
import pytest

import _quality_ref as R
import x266_amd
from _arena import Arena
from _dev import EINVAL, call_struct, sync_or_exit

pytestmark = pytest.mark.gpu

try:
    import x266_amd.quality as Q
    CHUNK = Q.totals_chunk()                                                # the totals' step, as the implementation exposes it
except (ImportError, x266_amd.X266Error, AttributeError):                   # collected without the feature: the tests then fail on their own
    Q, CHUNK = None, 256
PTRS = {"d_src": 16, "d_dec": 16, "d_ctu": 16, "d_total": 8}
DISP = {name: align * (2 * i + 1) for i, (name, align) in enumerate(PTRS.items())}          # exactly the documented alignment, no more
SIZES = [(16, 16), (48, 80), (64, 64), (144, 80)]
KINDS = ["same", "extremes", "noise", "inverse", "distorted"]
TALL = [(16, 64 * n) for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)]
ALL_KINDS = {(x, y) for x in range(3) for y in range(3)}
LIVE = {R.SSE: ("sse",), R.SSIM: ("ssim", "win_y", "win_c")}


@functools.lru_cache(None)
def case(kind, w, h):
    """(src, dec, records, totals, counters): the reference is computed once per frame pair and shared"""
    src, dec = R.pair(kind, w, h, seed=0xC0 + w + h)
    counters = {}
    rec = R.stats(src, dec, w, h, counters=counters)
    for a in (src, dec, rec):
        a.setflags(write=False)
    return src, dec, rec, R.totals(rec), counters


def stats(codec, src, dec, w, h, flags=3, total=True, stream=None, guard_seed=61):
    """the call inside an arena: (records, totals or None); guards, inputs and -- without d_total -- the totals' buffer are checked"""
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    a = Arena(codec)
    s_src = a.input("d_src", src, 16, DISP["d_src"], guard_seed)
    s_dec = a.input("d_dec", dec, 16, DISP["d_dec"], guard_seed + 1)
    s_ctu = a.output("d_ctu", 48 * n_ctu, 16, DISP["d_ctu"])
    s_tot = a.output("d_total", 64, 8, DISP["d_total"], written=None if total else np.zeros(64, bool))
    p = Q.quality_params(d_src=s_src.ptr, d_dec=s_dec.ptr, d_ctu=s_ctu.ptr, d_total=s_tot.ptr if total else 0, width=w, height=h, flags=flags)
    call_struct(codec, "xQualityStatsGpu", p, stream)
    got = a.check()
    return got["d_ctu"].view(R.CTU_DTYPE), got["d_total"].view(np.int64) if total else None


def same_records(got, want, fields=R.CTU_DTYPE.names):
    for name in fields:
        bad = np.flatnonzero((got[name] != want[name]).reshape(got.size, -1).any(1))
        assert bad.size == 0, (name, bad[:4], got[name][bad[:4]], want[name][bad[:4]])


# ---- 1. sizes and contents -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_sizes_and_contents(codec, kind, w, h):
    src, dec, want, want_tot, counters = case(kind, w, h)
    if kind in ("noise", "inverse"):                                         # what the comparison is worth: truncation and floor differ, every border is crossed
        assert counters["inexact_negative"] > 0
        if (w, h) == (144, 80):
            assert counters["kinds"][0] == ALL_KINDS and counters["kinds"][1] == ALL_KINDS
        if (w, h) == (48, 80):
            assert counters["kinds"][0] == {(x, y) for x in range(2) for y in range(3)}      # tile borders only across, CTU borders down
    for seed in (61, 97):                                                    # whatever lies around the frames must not reach a record
        rec, tot = stats(codec, src, dec, w, h, guard_seed=seed)
        same_records(rec, want)
        assert tot.tolist() == want_tot.tolist(), (tot, want_tot)
    assert tot[6:].tolist() == list(R.window_counts(w, h))
    if kind == "same":
        assert (rec["ssim"][:, 0] == rec["win_y"].astype(np.int64) << 30).all() and not rec["sse"].any()
        assert (rec["ssim"][:, 1] == rec["win_c"].astype(np.int64) << 30).all() and (rec["ssim"][:, 2] == rec["ssim"][:, 1]).all()
    if kind == "extremes":
        assert tot[:3].tolist() == [65025 * w * h, 65025 * w * h // 4, 65025 * w * h // 4] and int(tot[3]) == 1677 * int(tot[6])
    psnr, ssim = Q.from_totals(tot, w, h)
    want_psnr, want_ssim = R.from_totals(want_tot, w, h)
    assert np.allclose(psnr, want_psnr, rtol=1e-12, atol=0) and np.allclose(ssim, want_ssim, rtol=1e-12, atol=0)


def test_one_frame_as_both_inputs(codec):
    """d_dec == d_src, the very same buffer"""
    w, h = 144, 80
    src, _, want, want_tot, _ = case("same", w, h)
    a = Arena(codec)
    s_src = a.input("d_src", src, 16, DISP["d_src"], 61)
    s_ctu, s_tot = a.output("d_ctu", 48 * 6, 16, DISP["d_ctu"]), a.output("d_total", 64, 8, DISP["d_total"])
    call_struct(codec, "xQualityStatsGpu", Q.quality_params(d_src=s_src.ptr, d_dec=s_src.ptr, d_ctu=s_ctu.ptr, d_total=s_tot.ptr, width=w, height=h))
    got = a.check()
    same_records(got["d_ctu"].view(R.CTU_DTYPE), want)
    assert got["d_total"].view(np.int64).tolist() == want_tot.tolist()


# ---- 2. flags, and the call without totals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [R.SSE, R.SSIM])
def test_one_flag_alone(codec, flags):
    w, h = 144, 80
    src, dec, both, _, _ = case("noise", w, h)
    want = R.stats(src, dec, w, h, flags)
    rec, tot = stats(codec, src, dec, w, h, flags=flags)
    same_records(rec, want)
    assert tot.tolist() == R.totals(want).tolist()
    same_records(rec, both, LIVE[flags])                                     # the live fields are the both-flags run's
    for name in LIVE[3 - flags]:
        assert not rec[name].any(), name                                     # the other flag's fields are 0
    assert not rec["reserved"].any()


@pytest.mark.parametrize("flags", [3, R.SSE])
def test_without_totals(codec, flags):
    """d_total NULL: the records are identical and nothing else is written"""
    w, h = 144, 80
    src, dec, both, _, _ = case("noise", w, h)
    rec, tot = stats(codec, src, dec, w, h, flags=flags, total=False)
    assert tot is None
    same_records(rec, both if flags == 3 else R.stats(src, dec, w, h, flags))


@pytest.mark.parametrize("w,h", TALL)
def test_ctu_counts_around_the_totals_step(codec, w, h):
    assert CHUNK == Q.totals_chunk() == codec.L.xQualityTotalsChunk()
    src, dec, want, want_tot, _ = case("noise", w, h)
    assert want.size == h // 64
    rec, tot = stats(codec, src, dec, w, h)
    same_records(rec, want)
    assert tot.tolist() == want_tot.tolist(), (tot, want_tot)


# ---- 3. the same bytes on every run ------------------------------------------------------------------------------------------------------------
def test_two_runs_on_two_streams_give_identical_bytes(codec):
    w, h = 144, 80
    src, dec, want, _, _ = case("noise", w, h)
    streams = [codec.stream_create(), codec.stream_create()]
    try:
        runs = [stats(codec, src, dec, w, h, stream=st) for st in streams]
    finally:
        for st in streams:
            codec.stream_destroy(st)
    for a, b in zip(runs[0], runs[1]):
        assert a.tobytes() == b.tobytes()
    same_records(runs[0][0], want)


def test_numpy_convenience(codec):
    w, h = 48, 80
    src, dec, want, want_tot, _ = case("distorted", w, h)
    rec, tot = Q.quality_stats(codec, src, dec, w, h)
    assert rec.dtype == x266_amd.QUALITY_CTU_DTYPE and np.array_equal(rec, want) and tot.tolist() == want_tot.tolist()
    rec, tot = Q.quality_stats(codec, src, dec, w, h, flags=x266_amd.QUALITY_SSE)
    assert np.array_equal(rec["sse"], want["sse"]) and not rec["ssim"].any() and tot[3:].tolist() == [0] * 5


def test_in_a_graph(codec):
    """captured once, replayed on other frames than it was captured with"""
    w, h, n_ctu = 144, 80, 6
    pairs = [case("noise", w, h), case("distorted", w, h)]
    d_src, d_dec, d_ctu, d_tot = codec.alloc(w * h * 2), codec.alloc(w * h * 2), codec.alloc(48 * n_ctu), codec.alloc(64)
    p = Q.quality_params(d_src=d_src.ptr, d_dec=d_dec.ptr, d_ctu=d_ctu.ptr, d_total=d_tot.ptr, width=w, height=h)
    st = codec.stream_create()
    try:
        d_src.upload(pairs[0][0])
        d_dec.upload(pairs[0][1])
        codec.graph_begin(st)
        codec.quality_stats_dev(p, stream=st)
        graph = codec.graph_end(st)
        try:
            for i in (1, 0):
                src, dec, want, want_tot, _ = pairs[i]
                d_src.upload(src)
                d_dec.upload(dec)
                d_ctu.upload(np.full(48 * n_ctu, 0x5A, np.uint8))
                codec.graph_launch(graph, st)
                sync_or_exit(codec, 0, st)
                assert np.array_equal(d_ctu.download(np.uint8, 48 * n_ctu).view(R.CTU_DTYPE), want)
                assert d_tot.download(np.int64, 8).tolist() == want_tot.tolist()
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 4. refusals through the ABI -----------------------------------------------------------------------------------------------------------------
def test_argument_errors(codec):
    """every rule of the header: X266HIP_EINVAL, the call named in the error text, nothing launched, the arena untouched"""
    L, ctx = codec.L, codec.ctx
    name = "xQualityStatsGpu"
    w, h, n_ctu = 144, 80, 6
    src, dec, _, _, _ = case("noise", w, h)
    a = Arena(codec)
    slots = {"d_src": a.input("d_src", src, 16, DISP["d_src"], 61), "d_dec": a.input("d_dec", dec, 16, DISP["d_dec"], 62),
             "d_ctu": a.output("d_ctu", 48 * n_ctu, 16, DISP["d_ctu"]), "d_total": a.output("d_total", 64, 8, DISP["d_total"])}
    good = dict({f: s.ptr for f, s in slots.items()}, width=w, height=h, flags=3)
    extent = dict(d_src=w * h * 2, d_dec=w * h * 2, d_ctu=48 * n_ctu, d_total=64)

    def refused(**change):
        p = Q.quality_params(**dict(good, **change))
        assert L.xQualityStatsGpu(ctx, ctypes.byref(p), None) == EINVAL, change
        assert name.encode() in L.xHipLastError(ctx), change

    assert L.xQualityStatsGpu(ctx, None, None) == EINVAL and name.encode() in L.xHipLastError(ctx)      # NULL p
    assert L.xQualityStatsGpu(None, ctypes.byref(Q.quality_params(**good)), None) == EINVAL
    for field in ("d_src", "d_dec", "d_ctu"):
        refused(**{field: 0})
    for field in PTRS:
        refused(**{field: good[field] + PTRS[field] // 2})
        refused(**{field: 2 ** 64 - PTRS[field]})                            # aligned, and the extent does not fit behind it
    for side in ("width", "height"):
        for v in (0, -16, 8, 152 if side == "width" else 88):
            refused(**{side: v})
    for flags in (0, 4, 7, -1):
        refused(flags=flags)
    for field, other in (("d_ctu", "d_src"), ("d_ctu", "d_dec"), ("d_ctu", "d_total"), ("d_total", "d_src"), ("d_total", "d_dec"), ("d_total", "d_ctu")):
        refused(**{field: good[other] + (extent[other] - 1) // PTRS[field] * PTRS[field]})    # onto the other's last bytes
        if good[other] % PTRS[field] == 0:
            refused(**{field: good[other]})
    for field, other in (("d_src", "d_ctu"), ("d_dec", "d_ctu"), ("d_src", "d_total"), ("d_dec", "d_total")):   # an input moved onto an output
        refused(**{field: good[other] - (good[other] % 16)})
    sync_or_exit(codec, 0)
    a.check_untouched()                                                     # nothing was launched


# ---- 5. the plain-C host ----------------------------------------------------------------------------------------------------------------------------
def test_plain_c_host_example():
    """host/quality_example.c: a C host without HIP headers codes a small frame twice and measures both reconstructions on the device; the
    squared error a host loop finds beside it is the device's"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "quality_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "host"), "--no-print-directory", exe])
    out = subprocess.run([exe, "192", "128"], timeout=120, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["sse_equal"] is True
    for run in ("plain", "rdoq"):
        assert d[run]["sse_device"] == d[run]["sse_host"] > 0 and 20.0 < d[run]["psnr"] < 100.0 and 0.0 < d[run]["ssim_y"] < 1.0
    assert d["rdoq"]["sse_device"] >= d["plain"]["sse_device"]               # RDOQ trades distortion for rate
