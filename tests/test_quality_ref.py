"""CPU: the frame-quality reference (tests/_quality_ref.py) against the values include/x266hip.h states, against the same formula in
float64, and the host call xQualityFromTotals against numpy's float64.  No GPU."""
import ctypes
import functools

import numpy as np
import pytest

import _quality_ref as R


@functools.lru_cache(None)
def case(kind, w, h):
    """(src, dec, records, counters): computed once and shared"""
    src, dec = R.pair(kind, w, h, seed=0x51 + w + h)
    counters = {}
    rec = R.stats(src, dec, w, h, counters=counters)
    for a in (src, dec, rec):
        a.setflags(write=False)
    return src, dec, rec, counters


def test_the_worked_windows():
    flat = np.full((8, 8), 77)
    assert R.window(*R.sums_of(flat, flat))[0] == 1 << 30                   # identical windows: exactly one
    noise = np.random.RandomState(3).randint(0, 256, (8, 8))
    assert R.window(*R.sums_of(noise, noise))[0] == 1 << 30
    assert R.window(*R.sums_of(np.zeros((8, 8)), np.full((8, 8), 255)))[0] == 1677
    x, y = np.meshgrid(np.arange(8), np.arange(8))
    board = 255 * ((x + y) & 1)
    q, cn, exact = R.window(*R.sums_of(board, 255 - board))
    assert (cn, q) == (-132935237, -1069943477) and not exact


@pytest.mark.parametrize("w,h,luma,chroma", [(16, 16, 9, 1), (64, 64, 225, 49), (144, 80, 35 * 19, 17 * 9)])
def test_window_counts(w, h, luma, chroma):
    _, _, rec, _ = case("same", w, h)
    assert R.window_counts(w, h) == (luma, chroma)
    assert int(rec["win_y"].sum()) == luma and int(rec["win_c"].sum()) == chroma
    assert (rec["ssim"][:, 0] == rec["win_y"].astype(np.int64) << 30).all()       # a frame against itself: every q is one
    assert (rec["ssim"][:, 1] == rec["win_c"].astype(np.int64) << 30).all() and (rec["ssim"][:, 2] == rec["ssim"][:, 1]).all()
    assert not rec["sse"].any() and not rec["reserved"].any()
    if (w, h) == (144, 80):                                                  # 3 x 2 CTUs, the last column 16 wide and the last row 16 high
        assert rec["win_y"].tolist() == [256, 256, 48, 48, 48, 9] and rec["win_c"].tolist() == [64, 64, 8, 8, 8, 1]


def test_a_window_belongs_to_the_ctu_of_its_top_left_block():
    """one changed sample in luma block (16, 16), the first of CTU (1, 1): the four windows that hold it belong to four CTUs"""
    w, h = 144, 80
    src, _, same, _ = case("same", w, h)
    y, u, v = R.planes_from_tiles(src, w, h)
    y2 = y.copy()
    y2[64, 64] ^= 0x80
    dec = R.tiles_from_planes(y2, u, v)
    counters = {}
    rec = R.stats(src, dec, w, h, counters=counters)
    assert rec["sse"][:, 0].tolist() == [0, 0, 0, 0, 128 * 128, 0]
    q = counters["q"][0]
    changed = {0: (15, 15), 1: (16, 15), 3: (15, 16), 4: (16, 16)}          # CTU index: the window (bx, by) it owns
    for ctu in range(6):
        want = int(same["ssim"][ctu, 0])
        if ctu in changed:
            bx, by = changed[ctu]
            assert q[by, bx] < 1 << 30
            want += int(q[by, bx]) - (1 << 30)
        assert int(rec["ssim"][ctu, 0]) == want, ctu
    assert int((q != 1 << 30).sum()) == 4
    assert np.array_equal(rec["ssim"][:, 1:], same["ssim"][:, 1:])


def test_squared_error_of_the_extremes_and_the_totals():
    for w, h in ((16, 16), (144, 80)):
        src, dec, rec, _ = case("extremes", w, h)
        tot = R.totals(rec)
        assert tot[:3].tolist() == [65025 * w * h, 65025 * w * h // 4, 65025 * w * h // 4]
        assert (rec["ssim"][:, 0] == 1677 * rec["win_y"].astype(np.int64)).all()
        assert tot[6:].tolist() == list(R.window_counts(w, h))
    src, dec, rec, _ = case("noise", 144, 80)
    tot = R.totals(rec)
    assert tot.tolist() == [int(rec["sse"][:, p].astype(object).sum()) for p in range(3)] + [int(rec["ssim"][:, p].astype(object).sum()) for p in range(3)] + \
        [int(rec["win_y"].sum()), int(rec["win_c"].sum())]
    y0, y1 = R.planes_from_tiles(src, 144, 80)[0].astype(np.int64), R.planes_from_tiles(dec, 144, 80)[0].astype(np.int64)
    assert int(tot[0]) == int(((y0 - y1) ** 2).sum())
    for flags, dead in ((R.SSE, ("ssim", "win_y", "win_c")), (R.SSIM, ("sse",))):
        one = R.stats(src, dec, 144, 80, flags)
        for name in CTU_FIELDS:
            assert (not one[name].any()) if name in dead else np.array_equal(one[name], rec[name]), (flags, name)


CTU_FIELDS = ("ssim", "sse", "win_y", "win_c", "reserved")


@pytest.mark.parametrize("kind", ["noise", "distorted", "inverse"])
def test_q_is_the_float64_formula_within_four_units(kind):
    """q / 2^30 against the same formula in float64: three roundings of less than 2^-30 each bound the exact difference (lq, cq, and the
    last shift, each of a factor of at most one), one more unit covers the float64 evaluation"""
    w, h = 144, 80
    src, dec, rec, counters = case(kind, w, h)
    pa, pb = R.planes_from_tiles(src, w, h), R.planes_from_tiles(dec, w, h)
    worst = 0.0
    for p in range(3):
        s1, s2, ss, s12 = R.window_sums(pa[p], pb[p])
        q = counters["q"][p]
        for by in range(q.shape[0]):
            for bx in range(q.shape[1]):
                worst = max(worst, abs(int(q[by, bx]) / 2.0 ** 30 - R.window_float(s1[by, bx], s2[by, bx], ss[by, bx], s12[by, bx])))
    print("%s: worst |q / 2^30 - float64| = %.3f * 2^-30" % (kind, worst * 2.0 ** 30))
    assert worst <= 4 * 2.0 ** -30
    if kind != "distorted":                                                  # what the GPU cases rely on: truncation and floor differ somewhere
        assert counters["inexact_negative"] > 0
        assert counters["kinds"][0] == {(x, y) for x in range(3) for y in range(3)}
    if kind == "distorted":                                                  # a lightly distorted frame is close to one, and below it
        psnr, ssim = R.from_totals(R.totals(rec), w, h)
        assert (ssim > 0.9).all() and (ssim < 1.0).all() and (psnr > 35).all()


# ---- the host call -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import x266_amd
    x266_amd.build_library()
    return x266_amd.load_library()


def _from_totals(lib, total, w, h):
    t = np.ascontiguousarray(total, np.int64)
    psnr, ssim = np.full(4, -1.0), np.full(3, -1.0)
    rc = lib.xQualityFromTotals(ctypes.c_void_p(t.ctypes.data), w, h, ctypes.c_void_p(psnr.ctypes.data), ctypes.c_void_p(ssim.ctypes.data))
    return rc, psnr, ssim


@pytest.mark.parametrize("kind,w,h", [("noise", 144, 80), ("distorted", 144, 80), ("inverse", 48, 80), ("extremes", 16, 16)])
def test_from_totals_is_numpys_float64(lib, kind, w, h):
    """both sides do a handful of IEEE double operations and one log10: 1e-12 relative"""
    import x266_amd.quality as Q
    tot = R.totals(case(kind, w, h)[2])
    rc, psnr, ssim = _from_totals(lib, tot, w, h)
    want_psnr, want_ssim = R.from_totals(tot, w, h)
    assert rc == 0
    assert np.allclose(psnr, want_psnr, rtol=1e-12, atol=0) and np.allclose(ssim, want_ssim, rtol=1e-12, atol=0), (psnr, want_psnr, ssim, want_ssim)
    got = Q.from_totals(tot, w, h)
    assert np.array_equal(got[0], psnr) and np.array_equal(got[1], ssim)


def test_from_totals_degenerate_cases_and_refusals(lib):
    import x266_amd
    import x266_amd.quality as Q
    w, h = 144, 80
    win_y, win_c = R.window_counts(w, h)
    rc, psnr, ssim = _from_totals(lib, [0, 0, 0, win_y << 30, win_c << 30, win_c << 30, win_y, win_c], w, h)
    assert rc == 0 and psnr.tolist() == [100.0] * 4 and ssim.tolist() == [1.0] * 3        # a frame against itself
    rc, psnr, ssim = _from_totals(lib, [5, 0, 7, 0, 0, 0, 0, 0], w, h)                    # a run without SSIM: no window, 1.0
    assert rc == 0 and ssim.tolist() == [1.0] * 3 and psnr[1] == 100.0 and psnr[0] < 100.0 and psnr[3] < 100.0
    good = [5, 6, 7, 1 << 30, 2 << 30, -(3 << 30), win_y, win_c]
    assert _from_totals(lib, good, w, h)[0] == 0
    for i in range(3):
        bad = list(good)
        bad[i] = -1
        assert _from_totals(lib, bad, w, h)[0] == -1                                      # a negative SSE
    for i, v in ((6, win_y - 1), (6, win_y + 1), (6, -win_y), (7, win_c + 1), (7, 1), (6, win_c)):
        bad = list(good)
        bad[i] = v
        assert _from_totals(lib, bad, w, h)[0] == -1, (i, v)                              # window counts that are not the geometry's
    for bw, bh in ((0, 80), (144, 0), (-16, 80), (152, 80), (144, 72), (160, 80)):
        assert _from_totals(lib, good, bw, bh)[0] == -1, (bw, bh)
    t, out4, out3 = np.array(good, np.int64), np.zeros(4), np.zeros(3)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.xQualityFromTotals(None, w, h, ptr(out4), ptr(out3)) == -1
    assert lib.xQualityFromTotals(ptr(t), w, h, None, ptr(out3)) == -1 and lib.xQualityFromTotals(ptr(t), w, h, ptr(out4), None) == -1
    with pytest.raises(x266_amd.X266Error):
        Q.from_totals(good[:7], w, h)
    with pytest.raises(x266_amd.X266Error):
        Q.from_totals([-1] + good[1:], w, h)
    assert Q.totals_chunk() == lib.xQualityTotalsChunk() > 0
