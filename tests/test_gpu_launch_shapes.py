"""GPU (-m gpu): every launch shape of the autotuner's candidate tables (x266_amd/csrc/x266hip_abi.hip: kFwdInvCands, kReconCands,
kSatdCands, kSadCands), forced on purpose and held bit-exactly against the CPU oracle at the smallest sizes where it can go wrong.

"autotune" = 2 + k launches candidate k of every family, untimed, at any batch size (include/x266hip.h; the tests' hook), and
xHipAutotuneReport tells which candidate a family's forced launches took and how many there were: every eligible call below is followed
by a look at that count (so no case can pass on the default shape), every ineligible one by a look that it did not move.

What is pinned here, deterministically, for every table entry: the slot rotation of the DEPTH = 2, 3 and 4 instantiations of the fused
kernel, their refill and drain control flow (the last wave's run walks every value at which the wait formulas and the refill switch
case, next to full waves and a second workgroup), the (DEPTH + 1) x 2 KiB LDS layout, the grid and tail arithmetic of all three
launchers, and stores past the end (outputs sit in guard bands, tests/_arena.py).  What is NOT: that a hand-counted wait is low enough --
a DMA that is waited for too late usually still lands in time (tests/test_gpu_waits.py compares with the wait-for-everything build).

The tables are read from the source, so sizes follow a table that changes; the table SIZES are literals in test_refused_past_the_table."""
import collections
import os
import re

import numpy as np
import pytest

import x266_amd
from _arena import Arena
from _dev import EINVAL, sync_or_exit
from _util import ROOT, extremes_np, fullrange_np, residual_np

pytestmark = pytest.mark.gpu

MIXES = (residual_np, fullrange_np, extremes_np)
N_BIG = 3077                                   # "a few thousand blocks with a ragged tail": 3077 = 5 mod 6, 8, 12, 16, 24 and odd
N_SATD = 2400                                  # blocks of SATD data per mix (the largest case: 2 x 4 waves x 8 groups x 32 + 225 = 2273)


def _tables():
    src = open(os.path.join(ROOT, "x266_amd", "csrc", "x266hip_abi.hip")).read()
    out = {}
    for name in ("kFwdInvCands", "kReconCands", "kSatdCands", "kSadCands"):
        body = re.search(r"const ShapeCand %s\[\]\s*=\s*\{(.*?)\};" % name, src, re.S).group(1)
        out[name] = [tuple(int(v) for v in m.split(",")) for m in re.findall(r"\{([^{}]*)\}", body)]
        assert out[name] and all(len(c) == 4 for c in out[name]), name
    return out


TABLES = _tables()
FUSED = {"dct32_fwd_inv": TABLES["kFwdInvCands"], "dct32_recon_only": TABLES["kReconCands"]}
SATD, SAD = TABLES["kSatdCands"], TABLES["kSadCands"]
SAD_EDGES = (8, 16, 32, 64)
# forced launches per (family, candidate) as read back from the library by the cases of this file
TALLY = collections.Counter()


def _launches(cd, family):
    return cd.autotune_report().get(family, {}).get("launches", 0)


def _counted(cd, family, k, before):
    """the library says this family has taken candidate k once more than `before`"""
    rep = cd.autotune_report()
    assert rep.get(family) == {"forced": k, "launches": before + 1}, (family, k, before, rep)
    TALLY[family, k] += 1


def _force(cd, k):
    cd.set_option("autotune", 2 + k)
    assert cd.autotune_report() == {}                                    # setting the option forgets what was counted


@pytest.fixture
def forced():
    """a context of the test's own (forced state never leaks), the tables' run lengths as they are"""
    cd = x266_amd.Codec(0)
    cd.set_option("adaptive_per_wave", 0)
    yield cd
    cd.close()


@pytest.fixture(scope="module")
def dct_data(oracle):
    """per mix: N_BIG input blocks, their coefficients and their reconstruction by the oracle -- computed once, read-only, cases take windows"""
    out = []
    for i, gen in enumerate(MIXES):
        x = gen(N_BIG * 1024, 0xA100 + i).reshape(N_BIG, 1024)
        z = oracle.dct32_fwd(x, threads=8)
        r = oracle.dct32_inv(z, threads=8)
        for a in (x, z, r):
            a.setflags(write=False)
        out.append((x, z, r))
    return out


@pytest.fixture(scope="module")
def satd_data(oracle):
    out = []
    for i, gen in enumerate(MIXES):
        d = gen(N_SATD * 64, 0xB100 + i).reshape(N_SATD, 64)
        s = oracle.satd8x8(d, threads=8)
        d.setflags(write=False); s.setflags(write=False)
        out.append((d, s))
    return out


def _bad_blocks(got, want):
    return np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[:8].tolist()


def _fused_case(cd, data, family, k, n, mix, salt):
    """one forced launch of the fused call inside guard bands: coefficients and reconstruction equal the oracle, nothing behind block
    n - 1 of either output and nothing of the input changed, and the library counted the launch for candidate k"""
    with_coef = family == "dct32_fwd_inv"
    off = (salt * 131 + n * 7) % (N_BIG - n + 1)
    x, z, r = (a[off:off + n] for a in data[mix])
    arena = Arena(cd)
    s_in = arena.input("d_in", x, 16, 0, 0x1D00 + salt)
    s_co = arena.output("d_coef", n * 2048, 16, 0) if with_coef else None
    s_re = arena.output("d_recon", n * 2048, 16, 0)
    before = _launches(cd, family)
    cd.dct32_fwd_inv_dev(s_in.ptr, s_co.ptr if with_coef else 0, s_re.ptr, n)
    sync_or_exit(cd, 0)
    _counted(cd, family, k, before)
    got = arena.check()                                                  # guard bands of all three, the input unchanged
    where = (family, k, FUSED[family][k], "n", n, "mix", mix)
    if with_coef:
        gz = got["d_coef"].view(np.int16).reshape(n, 1024)
        assert np.array_equal(gz, z), where + ("coefficient blocks", _bad_blocks(gz, z))
    gr = got["d_recon"].view(np.int16).reshape(n, 1024)
    assert np.array_equal(gr, r), where + ("reconstruction blocks", _bad_blocks(gr, r))


def _fused_sizes(cand):
    """(single sizes, ragged sizes) of candidate (blocks per wave, workgroup threads, LDS per wave, DMA depth D): 1, D and one full run; two
    full workgroups plus a last wave whose run is 0, 1, D-1, D, D+1, 2D-1, 2D, 2D+1 blocks (those below a full run) -- every value at
    which the prologue, the steady-state / drain waits and the `i + D < cnt` refill change case; and one large ragged batch"""
    bpw, tpb, _, depth = cand
    waves = tpb // 64
    tails = sorted({r for r in (0, 1, depth - 1, depth, depth + 1, 2 * depth - 1, 2 * depth, 2 * depth + 1) if 0 <= r <= bpw - 1})
    return sorted({1, depth, bpw}), [2 * waves * bpw + r for r in tails] + [N_BIG]


FUSED_PARAMS = [pytest.param(f, k, id="%s-%d" % (f, k)) for f in FUSED for k in range(len(FUSED[f]))]


@pytest.mark.parametrize("family,k", FUSED_PARAMS)
def test_fused_candidate_against_the_oracle(forced, dct_data, family, k):
    """with d_coef the candidates of kFwdInvCands, with d_coef = NULL those of kReconCands: one mix at the single sizes (rotating), all three
    at the ragged ones"""
    _force(forced, k)
    singles, ragged = _fused_sizes(FUSED[family][k])
    for i, n in enumerate(singles):
        _fused_case(forced, dct_data, family, k, n, (i + k) % 3, i)
    for i, n in enumerate(ragged):
        for mix in range(3):
            _fused_case(forced, dct_data, family, k, n, mix, 16 + 3 * i + mix)
    assert _launches(forced, family) == len(singles) + 3 * len(ragged)


def _satd_case(cd, data, k, n, mix, salt):
    off = (salt * 37 + n) % (N_SATD - n + 1)
    d, want = (a[off:off + n] for a in data[mix])
    arena = Arena(cd)
    s_in = arena.input("d_diff", d, 16, 0, 0x2D00 + salt)
    s_out = arena.output("d_out", n * 4, 4, 0)
    before = _launches(cd, "satd8x8")
    cd.satd8x8_dev(s_in.ptr, s_out.ptr, n)
    sync_or_exit(cd, 0)
    _counted(cd, "satd8x8", k, before)
    got = arena.check()["d_out"].view(np.uint32)
    assert np.array_equal(got, want), ("satd8x8", k, SATD[k], "n", n, "mix", mix, np.flatnonzero(got != want)[:8].tolist())


@pytest.mark.parametrize("k", range(len(SATD)))
def test_satd_candidate_against_the_oracle(forced, satd_data, k):
    """the LDS-DMA kernel in every shape of kSatdCands, far below the batch size at which it is otherwise chosen: around one 32-block group, and
    two full workgroups plus a last wave of 0 blocks, 1 block, a group -1 / +0 / +1 and all groups but one + 1"""
    gpw, tpb, _, shape = SATD[k]
    assert shape == 3
    _force(forced, k)
    full = 2 * (tpb // 64) * gpw * 32
    sizes = sorted({1, 31, 32, 33} | {full + r for r in (0, 1, 31, 32, 33, 32 * (gpw - 1) + 1)})
    for i, n in enumerate(sizes):
        _satd_case(forced, satd_data, k, n, (i + k) % 3, i)
    assert _launches(forced, "satd8x8") == len(sizes)


def _sad_want(a, b):
    return np.abs(a.astype(np.int32) - b.astype(np.int32)).sum(axis=1).astype(np.uint32)


def _sad_case(cd, edge, a, b):
    """-> the sums the library gave, from an output in guard bands; inputs checked unchanged"""
    n = a.shape[0]
    arena = Arena(cd)
    s_a = arena.input("d_a", a, 16, 0, 0x3D00 + n)
    s_b = arena.input("d_b", b, 16, 0, 0x3E00 + n)
    s_out = arena.output("d_out", n * 4, 4, 0)
    cd.sad_dev(edge, s_a.ptr, s_b.ptr, s_out.ptr, n)
    sync_or_exit(cd, 0)
    return arena.check()["d_out"].view(np.uint32)


@pytest.mark.parametrize("edge", SAD_EDGES)
@pytest.mark.parametrize("k", range(len(SAD)))
def test_sad_candidate_against_numpy(forced, k, edge):
    """every workgroup size / LDS charge of kSadCands: a wave takes B = 256 / (edge * edge / 16) blocks, so one block, a wave's worth -1 / +0 / +1
    and three full workgroups plus one block; random bytes, and all-0 against all-255 (the largest sums)"""
    family, waves = "sad%d" % edge, SAD[k][1] // 64
    per_wave = 4096 // (edge * edge)
    _force(forced, k)
    rng = np.random.default_rng(0xC000 + 16 * k + edge)
    sizes = sorted({max(1, n) for n in (1, per_wave - 1, per_wave, per_wave + 1, 3 * waves * per_wave + 1)})
    count = 0
    for n in sizes:
        for extreme in (False, True):
            a = rng.integers(0, 256, (n, edge * edge), dtype=np.uint8)
            b = rng.integers(0, 256, (n, edge * edge), dtype=np.uint8)
            if extreme:
                a[:], b[:] = 0, 255
            got = _sad_case(forced, edge, a, b)
            _counted(forced, family, k, count)
            count += 1
            assert np.array_equal(got, _sad_want(a, b)), (family, k, SAD[k], "n", n, extreme)


def test_sad_edge_four_has_no_candidates(forced):
    """4x4 blocks have one launch shape: a forced context still gives the right sums and counts no launch"""
    _force(forced, len(SAD) - 1)
    rng = np.random.default_rng(0xC4)
    for n in (1, 63, 64, 65, 1000):
        a = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        b = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        assert np.array_equal(_sad_case(forced, 4, a, b), _sad_want(a, b)), n
        assert forced.autotune_report() == {}


def test_callers_knobs_and_overlap_keep_the_default_shape(forced, dct_data, satd_data, oracle):
    """forcing keeps the eligibility rules of tuning: a family whose own knobs are set, and a call on overlapping buffers, launch the default
    shape -- right results, and the forced-launch count does not move"""
    cd, n = forced, 205
    _force(cd, 1)                                                        # a DEPTH = 3 shape of both fused tables
    for family in FUSED:
        _fused_case(cd, dct_data, family, 1, n, 0, 1)                    # eligible: counted once
    x, z, r = (a[:n] for a in dct_data[1])
    cd.set_option("dct32_fwdinv_blocks_per_wave", 3)
    try:
        for with_coef in (True, False):
            arena = Arena(cd)
            s_in = arena.input("d_in", x, 16, 0, 0x4D00)
            s_co = arena.output("d_coef", n * 2048, 16, 0) if with_coef else None
            s_re = arena.output("d_recon", n * 2048, 16, 0)
            cd.dct32_fwd_inv_dev(s_in.ptr, s_co.ptr if with_coef else 0, s_re.ptr, n)
            sync_or_exit(cd, 0)
            got = arena.check()
            assert np.array_equal(got["d_recon"].view(np.int16).reshape(n, 1024), r)
            assert not with_coef or np.array_equal(got["d_coef"].view(np.int16).reshape(n, 1024), z)
            assert {f: _launches(cd, f) for f in FUSED} == {f: 1 for f in FUSED}
    finally:
        cd.set_option("dct32_fwdinv_blocks_per_wave", 0)
    # The header allows this call no overlap of an input with an output, so what an overlapping call writes is not compared; the library
    # nevertheless looks for it and must then stay with the default shape: the reconstruction over the input, with and without coefficients
    buf, co = cd.alloc(n * 2048), cd.alloc(n * 2048)
    for with_coef in (True, False):
        buf.upload(x)
        cd.dct32_fwd_inv_dev(buf.ptr, co.ptr if with_coef else 0, buf.ptr, n)
        sync_or_exit(cd, 0)
        assert {f: _launches(cd, f) for f in FUSED} == {f: 1 for f in FUSED}
    # SATD: "satd_variant" 2 (and 1, 3) and the family's launch knobs
    d, want = (a[:777] for a in satd_data[0])
    _satd_case(cd, satd_data, 1, 777, 0, 1)
    for key, value in (("satd_variant", 2), ("satd_variant", 1), ("satd_variant", 3), ("satd_groups_per_wave", 5), ("satd_wg_threads", 128),
                       ("satd_lds_bytes_per_wave", 9216)):
        cd.set_option(key, value)
        try:
            arena = Arena(cd)
            s_in = arena.input("d_diff", d, 16, 0, 0x4E00)
            s_out = arena.output("d_out", 777 * 4, 4, 0)
            cd.satd8x8_dev(s_in.ptr, s_out.ptr, 777)
            sync_or_exit(cd, 0)
            assert np.array_equal(arena.check()["d_out"].view(np.uint32), want), (key, value)
            assert _launches(cd, "satd8x8") == 1, (key, value)
        finally:
            cd.set_option(key, 0)
    # an empty batch launches nothing and counts nothing
    cd.dct32_fwd_inv_dev(buf.ptr, co.ptr, buf.ptr, 0)
    cd.satd8x8_dev(buf.ptr, co.ptr, 0)
    cd.sad_dev(8, buf.ptr, buf.ptr, co.ptr, 0)
    assert {f: _launches(cd, f) for f in FUSED} == {f: 1 for f in FUSED} and _launches(cd, "satd8x8") == 1 and "sad8" not in cd.autotune_report()


def test_refused_past_the_table(forced, dct_data, satd_data):
    """k = table size - 1 is the last candidate a family accepts; from k = table size on the family's call returns X266HIP_EINVAL, names the option
    and launches nothing (no byte of any buffer changes).  The sizes are literals: a table that grows or shrinks breaks here, next to the
    sweeps that follow the tables by themselves."""
    cd, n = forced, 40
    assert {f: len(t) for f, t in FUSED.items()} == {"dct32_fwd_inv": 8, "dct32_recon_only": 5} and len(SATD) == 6 and len(SAD) == 5
    x = dct_data[0][0][:n]
    d = satd_data[0][0][:n]
    a8 = np.random.default_rng(5).integers(0, 256, (n, 64), dtype=np.uint8)

    def fused(with_coef):
        arena = Arena(cd)
        s_in = arena.input("d_in", x, 16, 0, 0x5D00)
        s_co = arena.output("d_coef", n * 2048, 16, 0) if with_coef else None
        s_re = arena.output("d_recon", n * 2048, 16, 0)
        return arena, cd.L.xDct32FwdInvBatchDev(cd.ctx, s_in.ptr, s_co.ptr if with_coef else None, s_re.ptr, n, None)

    def satd():
        arena = Arena(cd)
        s_in, s_out = arena.input("d_diff", d, 16, 0, 0x5E00), arena.output("d_out", n * 4, 4, 0)
        return arena, cd.L.xSatd8x8BatchDev(cd.ctx, s_in.ptr, s_out.ptr, n, None)

    def sad():
        arena = Arena(cd)
        s_a, s_b, s_out = arena.input("d_a", a8, 16, 0, 0x5F00), arena.input("d_b", a8[::-1], 16, 0, 0x5F01), arena.output("d_out", n * 4, 4, 0)
        return arena, cd.L.xSadBatchDev(cd.ctx, 8, s_a.ptr, s_b.ptr, s_out.ptr, n, None)

    calls = (("dct32_fwd_inv", 8, lambda: fused(True)), ("dct32_recon_only", 5, lambda: fused(False)), ("satd8x8", 6, satd), ("sad8", 5, sad))
    for k in (4, 5, 6, 7, 8):
        _force(cd, k)
        for family, count, call in calls:
            arena, rc = call()
            sync_or_exit(cd, 0)
            if k < count:
                assert rc == 0, (family, k, cd.L.xHipLastError(cd.ctx).decode())
                arena.check()
                assert cd.autotune_report()[family] == {"forced": k, "launches": 1}, (family, k)
                TALLY[family, k] += 1
            else:
                assert rc == EINVAL, (family, k, rc)
                assert "autotune" in cd.L.xHipLastError(cd.ctx).decode(), (family, k)
                arena.check_untouched()
                assert family not in cd.autotune_report(), (family, k)
    with pytest.raises(x266_amd.X266Error):
        cd.set_option("autotune", 2 + 9)                                 # the option itself ends at k = 8, which no table has
    assert cd.get_option("autotune") == 2 + 8


@pytest.mark.parametrize("k", [1, 6])
def test_deep_shapes_replayed_from_a_graph(forced, dct_data, k):
    """a tuned context records its kept shape when a call is captured, so the deep pipelines must also be right as graph nodes: candidate 1
    (DEPTH = 3) and 6 (DEPTH = 4) of the fused table, one linear graph of the one call on a created stream, replayed on fresh inputs"""
    cd = forced
    bpw, tpb, _, depth = FUSED["dct32_fwd_inv"][k]
    assert depth == (3 if k == 1 else 4)
    n = 2 * (tpb // 64) * bpw + 2 * depth + 1
    _force(cd, k)
    arena = Arena(cd)
    s_in = arena.input("d_in", np.zeros(n * 2048, np.uint8), 16, 0, 0x6D00)
    s_co, s_re = arena.output("d_coef", n * 2048, 16, 0), arena.output("d_recon", n * 2048, 16, 0)
    st = cd.stream_create()
    try:
        sync_or_exit(cd, 0)
        cd.graph_begin(st)
        cd.dct32_fwd_inv_dev(s_in.ptr, s_co.ptr, s_re.ptr, n, st)          # no timing: the forced shape is what the capture records
        graph = cd.graph_end(st)
        _counted(cd, "dct32_fwd_inv", k, 0)
        try:
            for mix, off in ((0, 11), (2, 1500)):
                x, z, r = (a[off:off + n] for a in dct_data[mix])
                s_in.image[s_in.start:s_in.start + s_in.size] = x.view(np.uint8).ravel()
                for s in (s_in, s_co, s_re):
                    s.buf.upload(s.image)                                # fresh input, outputs back to the fill
                cd.graph_launch(graph, st)
                sync_or_exit(cd, 0, st)
                got = arena.check()
                assert np.array_equal(got["d_coef"].view(np.int16).reshape(n, 1024), z), (k, mix)
                assert np.array_equal(got["d_recon"].view(np.int16).reshape(n, 1024), r), (k, mix)
            assert _launches(cd, "dct32_fwd_inv") == 1                   # replays are not calls
        finally:
            cd.graph_free(graph)
    finally:
        cd.stream_destroy(st)


def test_every_table_entry_was_launched(forced, dct_data, satd_data):
    """the counts the library reported for this file's forced launches, per family and candidate: none is zero.  One more small case per entry
    runs here first, so the test also stands when it is run by itself; the sweeps above add theirs when they ran in the same session."""
    cd = forced
    for k in range(max(len(t) for t in TABLES.values())):
        _force(cd, k)
        for family, table in FUSED.items():
            if k < len(table):
                _fused_case(cd, dct_data, family, k, table[k][0] + 1, k % 3, k)
        if k < len(SATD):
            _satd_case(cd, satd_data, k, 65, k % 3, k)
        if k < len(SAD):
            rng = np.random.default_rng(k)
            for edge in SAD_EDGES:
                a = rng.integers(0, 256, (3, edge * edge), dtype=np.uint8)
                b = rng.integers(0, 256, (3, edge * edge), dtype=np.uint8)
                got = _sad_case(cd, edge, a, b)
                _counted(cd, "sad%d" % edge, k, 0)
                assert np.array_equal(got, _sad_want(a, b))
    families = [(f, len(t)) for f, t in FUSED.items()] + [("satd8x8", len(SATD))] + [("sad%d" % e, len(SAD)) for e in SAD_EDGES]
    for family, count in families:
        print("forced launches %-17s %s" % (family, " ".join("%d:%d" % (k, TALLY[family, k]) for k in range(count))))
    assert all(TALLY[family, k] > 0 for family, count in families for k in range(count))
