"""The reference statement of sample adaptive offset (tests/_sao_ref.py) on the CPU: against a plain-loop evaluation of the header's
text, its invariants, and the coverage of the data recipe the GPU tests use.  None of these needs a GPU or the library."""
import collections

import numpy as np
import pytest

import _sao_ref as R


# ---- the header's text, sample by sample ----------------------------------------------------------------------------------------------
def _sign(v):
    return (v > 0) - (v < 0)


def _category(p, x, y, k):
    ph, pw = p.shape
    (ax, ay), (bx, by) = (((-1, 0), (1, 0)), ((0, -1), (0, 1)), ((-1, -1), (1, 1)), ((1, -1), (-1, 1)))[k]
    if not (0 <= x + ax < pw and 0 <= y + ay < ph and 0 <= x + bx < pw and 0 <= y + by < ph):
        return 0
    c = int(p[y, x])
    return {-2: 1, -1: 2, 0: 0, 1: 3, 2: 4}[_sign(c - int(p[y + ay, x + ax])) + _sign(c - int(p[y + by, x + bx]))]


def _loop_stats(org, dec, w, h):
    nx, ny = R.ctus(w, h)
    out = np.zeros((nx * ny, 3, 48, 2), np.int64)
    for m in range(3):
        edge = 64 if m == 0 else 32
        ph, pw = dec[m].shape
        for y in range(ph):
            for x in range(pw):
                rec = out[(y // edge) * nx + x // edge, m]
                d = int(org[m][y, x]) - int(dec[m][y, x])
                for k in range(4):
                    cat = _category(dec[m], x, y, k)
                    if cat:
                        rec[4 * k + cat - 1] += (1, d)
                rec[16 + (int(dec[m][y, x]) >> 3)] += (1, d)
    return out


def _loop_offset(n, e, lo, hi, lam, band):
    h0 = 0 if n == 0 else max(lo, min(hi, _sign(e) * ((2 * abs(e) + n) // (2 * n))))
    cands = [h0 - _sign(h0) * i for i in range(abs(h0) + 1)]              # h0, each step towards 0, and 0
    cost = lambda v: 16 * (n * v * v - 2 * v * e) + lam * (min(abs(v) + 1, 7) + (1 if band and v else 0))
    best = min(cands, key=lambda v: (cost(v), abs(v)))
    return best, cost(best)


def _loop_decide(st, lam):
    out = np.zeros((st.shape[0], 3, 8), np.uint8)
    for t in range(st.shape[0]):
        found = []
        for m in range(3):
            eo = [[_loop_offset(int(st[t, m, 4 * k + q, 0]), int(st[t, m, 4 * k + q, 1]), 0 if q < 2 else -7, 7 if q < 2 else 0, lam, False)
                   for q in range(4)] for k in range(4)]
            bands = [_loop_offset(int(st[t, m, 16 + b, 0]), int(st[t, m, 16 + b, 1]), -7, 7, lam, True) for b in range(32)]
            windows = [sum(bands[p + i][1] for i in range(4)) for p in range(29)]
            found.append((eo, bands, windows.index(min(windows)), min(windows)))
        for comps, bo_rate in (((0,), 7), ((1, 2), 12)):
            cands = [lam] + [4 * lam + sum(sum(j for _, j in found[m][0][k]) for m in comps) for k in range(4)]
            cands.append(bo_rate * lam + sum(found[m][3] for m in comps))
            pick = cands.index(min(cands))
            for m in comps:
                if 1 <= pick <= 4:
                    out[t, m, :2] = (2, pick - 1)
                    out[t, m, 2:6] = np.array([hh for hh, _ in found[m][0][pick - 1]], np.int8).view(np.uint8)
                elif pick == 5:
                    p = found[m][2]
                    out[t, m, :2] = (1, p)
                    out[t, m, 2:6] = np.array([found[m][1][p + i][0] for i in range(4)], np.int8).view(np.uint8)
    return out


def _loop_apply(dec, params, w, h):
    nx = R.ctus(w, h)[0]
    outs = []
    for m in range(3):
        edge = 64 if m == 0 else 32
        ph, pw = dec[m].shape
        o = np.array(dec[m])
        for y in range(ph):
            for x in range(pw):
                rec = params[(y // edge) * nx + x // edge, m]
                offs = rec[2:6].view(np.int8)
                c = int(dec[m][y, x])
                if rec[0] == 2:
                    cat = _category(dec[m], x, y, int(rec[1]) & 3)
                    if cat:
                        o[y, x] = max(0, min(255, c + int(offs[cat - 1])))
                elif rec[0] == 1:
                    j = ((c >> 3) - int(rec[1])) & 31
                    if j < 4:
                        o[y, x] = max(0, min(255, c + int(offs[j])))
        outs.append(o)
    return outs


# ---- 1. numpy against the loops -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sharp2", "band", "far"])
def test_numpy_statement_is_the_plain_loop(kind):
    w, h = 80, 48
    org, dec = R.case(kind, w, h)
    st = R.stats(org, dec)
    assert np.array_equal(st, _loop_stats(org, dec, w, h))
    assert st[:, 0, :16, 0].sum() > 0 and (st[..., 16:, 0].sum(axis=-1) == [[64 * 48, 32 * 24, 32 * 24], [16 * 48, 8 * 24, 8 * 24]]).all()
    for lam in (0, 37, 400, 65535):
        params = R.decide(st, lam)
        assert np.array_equal(params, _loop_decide(st, lam)), lam
        for got, want in zip(R.apply(dec, params, w, h), _loop_apply(dec, params, w, h)):
            assert np.array_equal(got, want), lam
    rng = np.random.RandomState(5)
    wild = rng.randint(0, 256, (2, 3, 8)).astype(np.uint8)                  # any type, any arg, any int8 offset
    wild[0, :, 0], wild[1, :, 0] = (2, 1, 2), (1, 2, 7)
    for got, want in zip(R.apply(dec, wild, w, h), _loop_apply(dec, wild, w, h)):
        assert np.array_equal(got, want)


# ---- 2. invariants --------------------------------------------------------------------------------------------------------------------
def test_all_off_copies_the_frame():
    w, h = 144, 80
    _, dec = R.case("sharp0", w, h)
    for got, want in zip(R.apply(dec, np.zeros((6, 3, 8), np.uint8), w, h), dec):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("lam", [0, 1, 37, 65535])
def test_identical_frames_decide_off(lam):
    w, h = 144, 80
    org, _ = R.case("sharp1", w, h)
    st = R.stats(org, org)
    assert not st[..., 1].any()
    assert not R.decide(st, lam).any()


def test_lambda_0_never_raises_a_components_squared_error():
    for w, h in R.SIZES:
        for kind in R.KINDS:
            org, dec = R.case(kind, w, h)
            out = R.apply(dec, R.decide(R.stats(org, dec), 0), w, h)
            for m in range(3):
                edge = 64 if m == 0 else 32
                assert (R.squared_error(org[m], out[m], edge) <= R.squared_error(org[m], dec[m], edge)).all(), (w, h, kind, m)


def test_largest_lambda_decides_off_on_the_recipe():
    for w, h in R.SIZES:
        for kind in R.KINDS:
            org, dec = R.case(kind, w, h)
            assert not R.decide(R.stats(org, dec), 65535).any(), (w, h, kind)


def test_mirror_swaps_classes_2_and_3():
    _, dec = R.case("sharp3", 80, 48)
    for p in dec:
        cat, mirrored = R.categories(p), R.categories(p[:, ::-1])
        for k, other in ((0, 0), (1, 1), (2, 3), (3, 2)):
            assert np.array_equal(mirrored[k][:, ::-1], cat[other])


# ---- 3. what the recipe exercises, on the reference alone ------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", R.SIZES)
def test_recipe_coverage(w, h):
    info = collections.Counter()
    filled = np.zeros((3, 48), np.int64)
    for kind in R.KINDS:
        org, dec = R.case(kind, w, h)
        st = R.stats(org, dec)
        filled += (st[..., 0] > 0).sum(axis=0)
        for lam in R.LAMBDAS:
            R.decide(st, lam, info)
    for plane in ("luma", "chroma"):
        for choice in ("off", "bo", "eo0", "eo1", "eo2", "eo3"):
            assert info["%s_%s" % (plane, choice)] > 0, (plane, choice)
    assert (filled[:, :16] > 0).all() and ((filled[:, 16:] > 0).sum(axis=1) >= 8).all()
    assert info["reaches_7"] > 0 and info["clamped_to_7"] > 0 and info["cut_by_rate"] > 0
    assert info["tie_to_earlier"] > 0 and info["band_position_tie"] > 0
