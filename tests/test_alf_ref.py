"""CPU: the vectorised reference statement of the adaptive loop filter (tests/_alf_ref.py) against plain loops written from the text
of include/x266hip.h, and the conditions the test data must meet -- asserted here on the statement, never on the device's output."""
import numpy as np
import pytest

import _alf_ref as R

VAR = (0, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4)
TT = (0, 1, 0, 2, 2, 3, 1, 3)
KCLIP = (256, 32, 8, 2)


def r(p, x, y):
    ph, pw = p.shape
    return int(p[min(max(y, 0), ph - 1), min(max(x, 0), pw - 1)])


def g(tr, dx, dy):
    return {0: (dx, dy), 1: (dy, dx), 2: (dx, -dy), 3: (dy, -dx)}[tr]


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def loop_classify(p):
    h, w = p.shape
    out = np.zeros((h // 4, w // 4), np.uint8)
    for by in range(h // 4):
        for bx in range(w // 4):
            V = H = D0 = D1 = 0
            for y in range(4 * by - 2, 4 * by + 6):
                for x in range(4 * bx - 2, 4 * bx + 6):
                    if (x + y) % 2:
                        continue
                    c = r(p, x, y)
                    V += abs(2 * c - r(p, x, y - 1) - r(p, x, y + 1))
                    H += abs(2 * c - r(p, x - 1, y) - r(p, x + 1, y))
                    D0 += abs(2 * c - r(p, x - 1, y - 1) - r(p, x + 1, y + 1))
                    D1 += abs(2 * c - r(p, x + 1, y - 1) - r(p, x - 1, y + 1))
            hv1, hv0, dir_hv = (V, H, 1) if V > H else (H, V, 3)
            d1, d0, dir_d = (D0, D1, 0) if D0 > D1 else (D1, D0, 2)
            m1, m0, dir1, dir2 = (d1, d0, dir_d, dir_hv) if d1 * hv0 > hv1 * d0 else (hv1, hv0, dir_hv, dir_d)
            dir_s = 2 if 2 * m1 > 9 * m0 else 1 if m1 > 2 * m0 else 0
            act = VAR[min(15, (H + V) >> 5)]
            cls = act + (5 * (((dir1 & 1) << 1) + dir_s) if dir_s else 0)
            assert 0 <= cls <= 24
            out[by, bx] = cls | TT[2 * dir1 + (dir2 >> 1)] << 5
    return out


def loop_apply_plane(p, taps, edge, class_map, coef, clip, ctrl_column):
    """coef, clip: [n, 25, taps] (luma) or [n, taps] (chroma, class_map None)"""
    ph, pw = p.shape
    nx = (pw + edge - 1) // edge
    out = p.copy()
    for y in range(ph):
        for x in range(pw):
            k = int(ctrl_column[(y // edge) * nx + x // edge])
            if k < 1 or k > coef.shape[0]:
                continue
            if class_map is None:
                cf, cl, tr = coef[k - 1], clip[k - 1], 0
            else:
                b = int(class_map[y // 4, x // 4])
                cf, cl, tr = coef[k - 1][min(b & 31, 24)], clip[k - 1][min(b & 31, 24)], b >> 5 & 3
            c, s = r(p, x, y), 0
            for i, (dx, dy) in enumerate(taps):
                gx, gy = g(tr, dx, dy)
                kk = KCLIP[int(cl[i]) & 3]
                s += int(cf[i]) * (clamp(r(p, x + gx, y + gy) - c, -kk, kk) + clamp(r(p, x - gx, y - gy) - c, -kk, kk))
            out[y, x] = clamp(c + ((s + 64) >> 7), 0, 255)
    return out


def loop_stats_plane(org, dec, taps, edge, class_map):
    """[n_ctu, classes, words]"""
    ph, pw = dec.shape
    ny, nx = (ph + edge - 1) // edge, (pw + edge - 1) // edge
    n = len(taps)
    words = 2 + n + n * (n + 1) // 2
    out = np.zeros((ny * nx, 25 if class_map is not None else 1, words), np.int64)
    for y in range(ph):
        for x in range(pw):
            cls = tr = 0
            if class_map is not None:
                b = int(class_map[y // 4, x // 4])
                cls, tr = min(b & 31, 24), b >> 5 & 3
            c = r(dec, x, y)
            d = int(org[y, x]) - c
            e = []
            for dx, dy in taps:
                gx, gy = g(tr, dx, dy)
                e.append(r(dec, x + gx, y + gy) + r(dec, x - gx, y - gy) - 2 * c)
            rec = out[(y // edge) * nx + x // edge, cls]
            rec[0] += 1
            rec[1] += d * d
            at = 2 + n
            for i in range(n):
                rec[2 + i] += e[i] * d
                for j in range(i, n):
                    rec[at] += e[i] * e[j]
                    at += 1
    return out


# ---- the statement against the loops ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", R.SIZES)
def test_classification_is_the_headers(w, h):
    for kind in R.CLASSIFY_KINDS + ("spikes",):
        dec = R.case(kind, w, h)[1][0]
        assert np.array_equal(R.classify(dec), loop_classify(dec)), kind


def test_apply_is_the_headers():
    w, h = 80, 48
    _, dec = R.case("noise", w, h)
    cmap = R.noise(w // 4, h // 4, 5)
    luma, chroma = R.random_filters(3, 2, 17)
    ctrl = np.array([[1, 2, 0], [3, 3, 1]], np.uint8)                       # U of CTU 1: 3 is above the count, a copy
    got = R.apply(dec, cmap, luma, chroma, ctrl)
    lc, lk = R.split_luma(luma)
    cc, ck = R.split_chroma(chroma)
    assert np.array_equal(got[0], loop_apply_plane(dec[0], R.P_LUMA, 64, cmap, lc, lk, ctrl[:, 0]))
    assert np.array_equal(got[1], loop_apply_plane(dec[1], R.P_CHROMA, 32, None, cc, ck, ctrl[:, 1]))
    assert np.array_equal(got[2], loop_apply_plane(dec[2], R.P_CHROMA, 32, None, cc, ck, ctrl[:, 2]))
    assert not np.array_equal(got[0], dec[0]) and np.array_equal(got[1][:, 32:], dec[1][:, 32:]) and np.array_equal(got[2][:, :32], dec[2][:, :32])
    assert not np.array_equal(got[1][:, :32], dec[1][:, :32]) and not np.array_equal(got[2][:, 32:], dec[2][:, 32:])
    assert (got[0] == 0).any() and (got[0] == 255).any()                    # clip8 fires both ways


def test_statistics_are_the_headers():
    w, h = 80, 48
    for kind, cmap in (("blur", None), ("far", R.noise(w // 4, h // 4, 6))):
        org, dec = R.case(kind, w, h)
        st = R.stats(org, dec, cmap)
        used = R.classify(dec[0]) if cmap is None else cmap
        luma = loop_stats_plane(org[0], dec[0], R.P_LUMA, 64, used).reshape(-1, 25 * 92)
        u = loop_stats_plane(org[1], dec[1], R.P_CHROMA, 32, None).reshape(-1, 29)
        v = loop_stats_plane(org[2], dec[2], R.P_CHROMA, 32, None).reshape(-1, 29)
        assert np.array_equal(st, np.concatenate([luma, u, v], axis=1)), kind
        assert np.abs(st).max() < 2 ** 31
    assert st[:, 0:2300:92].sum() == w * h and np.array_equal(R.sum_stats(st, [0, 1]), st[1])


def test_decision_is_the_headers():
    org, dec = R.case("blur", 80, 48)
    st = R.stats(org, dec)
    luma, chroma = R.random_filters(3, 2, 23)
    luma, chroma = (luma.view(np.int8) // 8).view(np.uint8), (chroma.view(np.int8) // 8).view(np.uint8)
    lc, _ = R.split_luma(luma)
    rec = st[0]
    # the quadratic form with the full symmetric matrix
    for k in (0, 3, 24):
        part = rec[92 * k:92 * k + 92]
        a = np.zeros((12, 12), np.int64)
        for wd, (i, j) in enumerate(R.triangle(12)):
            a[i, j] = a[j, i] = part[14 + wd]
        c = lc[1, k]
        assert R.record_cost(part, c) == int(c @ a @ c - 256 * (c * part[2:14]).sum())
    assert [R.ceil_log2(n) for n in range(1, 9)] == [0, 1, 2, 2, 3, 3, 3, 3]
    zero = R.pack(np.zeros((1, 25, 12)), None, np.zeros((1, 6)), None)
    assert not R.decide(st, *zero, 0).any()                                 # a tie with off: off comes first
    empty = np.zeros_like(st)
    assert not R.decide(empty, luma, chroma, 0).any()                       # count 0


# ---- the conditions on the data -----------------------------------------------------------------------------------------------------
def test_stripes_reach_their_classes_and_the_fixtures_reach_all():
    w, h = 144, 80
    cls, _ = R.decode(R.classify(R.case("stripes", w, h)[1][0]))
    assert set(cls.ravel().tolist()) == {2, 3, 4, 7, 8, 9, 12, 13, 14}
    seen, turns = set(), set()
    for kind in R.CLASSIFY_KINDS:
        cls, tr = R.decode(R.classify(R.case(kind, w, h)[1][0]))
        seen |= set(cls.ravel().tolist())
        turns |= set(tr.ravel().tolist())
    assert seen == set(range(25)) and turns == {0, 1, 2, 3}


def solved_filters(org, dec):
    """the packed sets solved from the statement's own totals: one luma set; U's and V's solutions as the two chroma alternatives"""
    st = R.stats(org, dec)
    lc, uc, vc = R.solve(R.sum_stats(st))
    return st, R.pack(lc[None], None, np.stack([uc, vc]), None)


@pytest.mark.parametrize("w,h", R.SIZES)
def test_solved_filters_reduce_the_error_of_blur(w, h):
    org, dec = R.case("blur", w, h)
    st, (luma, chroma) = solved_filters(org, dec)
    ctrl = np.tile(np.array([1, 1, 2], np.uint8), (st.shape[0], 1))
    out = R.apply(dec, None, luma, chroma, ctrl)
    before, after = R.squared_error(org[0], dec[0]), R.squared_error(org[0], out[0])
    estimate = sum(R.ctu_costs(rec, luma, chroma)[0][0] for rec in st) / 2.0 ** 14
    print("blur %dx%d: luma SSE %d -> %d, estimated change %.0f" % (w, h, before, after, estimate))
    assert after < before
    assert abs(estimate - (after - before)) < 0.1 * (before - after)        # the estimate from the statistics agrees with the real change


def test_far_approaches_the_bounds_and_same_has_no_error():
    org, dec = R.case("far", 144, 80)
    st = R.stats(org, dec)
    assert np.abs(st).max() > 2 ** 29 and np.abs(st).max() < 2 ** 31
    org, dec = R.case("same", 80, 48)
    st = R.stats(org, dec).reshape(2, -1)
    for rec, n in [(st[:, 92 * k:92 * k + 92], 12) for k in range(25)] + [(st[:, 2300:2329], 6), (st[:, 2329:], 6)]:
        assert not rec[:, 1:2 + n].any()
