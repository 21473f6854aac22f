"""The deblocking statement of tests/_deblock_ref.py against two independent evaluations written as plain loops, its properties,
the coverage of the test recipes, and the header / library surface.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _deblock_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOP_SIZES = R.SIZES + [(144, 80)]


# ---- the restatement: scalars, one sample at a time ---------------------------------------------------------------------------------------
def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


class Loop:
    """side information looked up one entry at a time"""

    def __init__(self, side, w, h):
        self.s, self.w, self.h, self.cx = side, w, h, (w + 63) // 64

    def _get(self, arr, r, default):
        return default if arr is None else int(np.asarray(arr).ravel()[r])

    def n(self, r):
        return 4 << (self._get(self.s.cls, r, 3) & 3)

    def qp(self, r):
        return min(self._get(self.s.qps, r, self.s.qp), 51)

    def luma_region(self, bx, by):
        return ((by // 8) * self.cx + bx // 8) * 6 + ((by // 4) % 2) * 2 + (bx // 4) % 2

    def luma_edge(self, pb, qb, coord):
        """(bs, beta, tc) of the edge between blocks pb = (bx, by) and qb"""
        rp, rq = self.luma_region(*pb), self.luma_region(*qb)
        transform = rp != rq or coord % self.n(rq) == 0
        intra = self._get(self.s.intra, rp, 0) != 0 or self._get(self.s.intra, rq, 0) != 0
        coded = self._get(self.s.nnz, rp, 1) != 0 or self._get(self.s.nnz, rq, 1) != 0
        bs = 0
        if transform and intra:
            bs = 2
        elif transform and coded:
            bs = 1
        elif not intra and self.s.mv is not None:
            m = np.asarray(self.s.mv).reshape(-1, 2)
            a, b = m[pb[1] * (self.w // 8) + pb[0]], m[qb[1] * (self.w // 8) + qb[0]]
            if abs(int(a[0]) - int(b[0])) >= 4 or abs(int(a[1]) - int(b[1])) >= 4:
                bs = 1
        if bs == 0:
            return 0, 0, 0
        qp = (self.qp(rp) + self.qp(rq) + 1) >> 1
        return bs, int(R.BETA[_clamp(qp + 2 * self.s.beta_offset_div2, 0, 51)]), int(R.TC[_clamp(qp + 2 * (bs - 1) + 2 * self.s.tc_offset_div2, 0, 53)])

    def chroma_edge(self, pt, qt, coord, plane):
        """tc of the edge between tiles pt = (tx, ty) and qt on plane 0 / 1, or None when it is not filtered"""
        ctu = lambda t: (t[1] // 4) * self.cx + t[0] // 4
        quad = lambda t: ctu(t) * 6 + ((t[1] // 2) % 2) * 2 + (t[0] // 2) % 2
        if ctu(pt) == ctu(qt) and coord % self.n(ctu(qt) * 6 + 4 + plane) != 0:
            return None
        if self._get(self.s.intra, quad(pt), 0) == 0 and self._get(self.s.intra, quad(qt), 0) == 0:
            return None
        qp = (self.qp(ctu(pt) * 6 + 4 + plane) + self.qp(ctu(qt) * 6 + 4 + plane) + 1) >> 1
        return int(R.TC[_clamp(qp + 2 + 2 * self.s.tc_offset_div2, 0, 53)])


def _luma_segment(get, put, beta, tc):
    """one segment of four lines; get(i, j) / put(i, j, v): sample j (0..7 = p3 p2 p1 p0 q0 q1 q2 q3) of line i"""
    l = [[get(i, j) for j in range(8)] for i in range(4)]
    dp = [abs(l[i][1] - 2 * l[i][2] + l[i][3]) for i in (0, 3)]
    dq = [abs(l[i][6] - 2 * l[i][5] + l[i][4]) for i in (0, 3)]
    if sum(dp) + sum(dq) >= beta:
        return
    strong = all(2 * (dp[n] + dq[n]) < (beta >> 2) and abs(l[i][0] - l[i][3]) + abs(l[i][4] - l[i][7]) < (beta >> 3) and
                 abs(l[i][3] - l[i][4]) < ((5 * tc + 1) >> 1) for n, i in enumerate((0, 3)))
    dep, deq = sum(dp) < ((beta + (beta >> 1)) >> 3), sum(dq) < ((beta + (beta >> 1)) >> 3)
    for i in range(4):
        p3, p2, p1, p0, q0, q1, q2, q3 = l[i]
        if strong:
            put(i, 3, _clamp((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, p0 - 2 * tc, p0 + 2 * tc))
            put(i, 2, _clamp((p2 + p1 + p0 + q0 + 2) >> 2, p1 - 2 * tc, p1 + 2 * tc))
            put(i, 1, _clamp((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3, p2 - 2 * tc, p2 + 2 * tc))
            put(i, 4, _clamp((q2 + 2 * q1 + 2 * q0 + 2 * p0 + p1 + 4) >> 3, q0 - 2 * tc, q0 + 2 * tc))
            put(i, 5, _clamp((q2 + q1 + q0 + p0 + 2) >> 2, q1 - 2 * tc, q1 + 2 * tc))
            put(i, 6, _clamp((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3, q2 - 2 * tc, q2 + 2 * tc))
            continue
        d = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4
        if abs(d) >= 10 * tc:
            continue
        d = _clamp(d, -tc, tc)
        put(i, 3, _clamp(p0 + d, 0, 255))
        put(i, 4, _clamp(q0 - d, 0, 255))
        if dep:
            put(i, 2, _clamp(p1 + _clamp((((p2 + p0 + 1) >> 1) - p1 + d) >> 1, -(tc >> 1), tc >> 1), 0, 255))
        if deq:
            put(i, 5, _clamp(q1 + _clamp((((q2 + q0 + 1) >> 1) - q1 - d) >> 1, -(tc >> 1), tc >> 1), 0, 255))


def _chroma_line(get, put, tc):
    p1, p0, q0, q1 = (get(j) for j in range(4))
    d = _clamp((((q0 - p0) << 2) + p1 - q1 + 4) >> 3, -tc, tc)
    put(1, _clamp(p0 + d, 0, 255))
    put(2, _clamp(q0 - d, 0, 255))


def _luma_segment_at(buf_get, buf_put, lp, vertical, edge, start):
    """the segment of lines start .. start + 3 of the edge at coordinate `edge` (x for a vertical edge, y for a horizontal one)"""
    line0 = start // 8
    pb, qb = ((edge // 8 - 1, line0), (edge // 8, line0)) if vertical else ((line0, edge // 8 - 1), (line0, edge // 8))
    bs, beta, tc = lp.luma_edge(pb, qb, edge)
    if bs == 0:
        return
    at = (lambda i, j: (start + i, edge - 4 + j)) if vertical else (lambda i, j: (edge - 4 + j, start + i))
    _luma_segment(lambda i, j: buf_get(*at(i, j)), lambda i, j, v: buf_put(*at(i, j), v), beta, tc)


def _chroma_line_at(buf_get, buf_put, lp, plane, vertical, edge, pos):
    t = pos // 8
    pt, qt = ((edge // 8 - 1, t), (edge // 8, t)) if vertical else ((t, edge // 8 - 1), (t, edge // 8))
    tc = lp.chroma_edge(pt, qt, edge, plane)
    if tc is None:
        return
    at = (lambda j: (pos, edge - 2 + j)) if vertical else (lambda j: (edge - 2 + j, pos))
    _chroma_line(lambda j: buf_get(*at(j)), lambda j, v: buf_put(*at(j), v), tc)


def loop_in_place(y, u, v, side):
    """picture order on ONE buffer per plane: every vertical edge, then every horizontal edge"""
    h, w = y.shape
    lp = Loop(side, w, h)
    out = []
    for plane, src in ((None, y), (0, u), (1, v)):
        b = [[int(x) for x in row] for row in src]
        ph, pw = src.shape

        def get(r, c):
            return b[r][c]

        def put(r, c, val):
            b[r][c] = val

        for vertical in (True, False):
            lines, across = (ph, pw) if vertical else (pw, ph)
            for edge in range(8, across, 8):
                if plane is None:
                    for start in range(0, lines, 4):
                        _luma_segment_at(get, put, lp, vertical, edge, start)
                else:
                    for pos in range(lines):
                        _chroma_line_at(get, put, lp, plane, vertical, edge, pos)
        out.append(np.array(b, np.uint8))
    return out


def loop_by_areas(y, u, v, side):
    """every shifted 8x8 area [8k-4, 8k+4) x [8m-4, 8m+4), clipped at the frame, on its own: from the UNFILTERED input, touching
    nothing outside the area (an access outside raises), into a separate output"""
    h, w = y.shape
    lp = Loop(side, w, h)
    out = []
    for plane, src in ((None, y), (0, u), (1, v)):
        ph, pw = src.shape
        res = np.zeros((ph, pw), np.uint8)
        for m in range(ph // 8 + 1):
            for k in range(pw // 8 + 1):
                r0, r1, c0, c1 = max(8 * m - 4, 0), min(8 * m + 4, ph), max(8 * k - 4, 0), min(8 * k + 4, pw)
                area = {(r, c): int(src[r, c]) for r in range(r0, r1) for c in range(c0, c1)}

                def get(r, c):
                    return area[(r, c)]                                    # KeyError: the filter left its area

                def put(r, c, val):
                    assert (r, c) in area
                    area[(r, c)] = val

                for vertical, edge, lo, hi in ((True, 8 * k, r0, r1), (False, 8 * m, c0, c1)):
                    if not 0 < edge < (pw if vertical else ph):
                        continue
                    if plane is None:
                        for start in range(lo, hi, 4):
                            _luma_segment_at(get, put, lp, vertical, edge, start)
                    else:
                        for pos in range(lo, hi):
                            _chroma_line_at(get, put, lp, plane, vertical, edge, pos)
                for (r, c), val in area.items():
                    res[r, c] = val
        out.append(res)
    return out


def _statement(y, u, v, side):
    py, counts = R.deblock_luma(y, side)
    pu, pv, _ = R.deblock_chroma(u, v, side, counts)
    return [py, pu, pv], counts


@pytest.fixture(scope="module")
def cases():
    """every kind of every size, with the statement's result: computed once"""
    out = {}
    for w, h in R.SIZES + R.COMPOSITE:
        for kind in R.KINDS:
            y, u, v, side = R.case(kind, w, h)
            out[(w, h, kind)] = (y, u, v, side) + tuple(_statement(y, u, v, side))
    return out


# ---- 1, 2: the two other evaluations ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", LOOP_SIZES)
def test_statement_equals_the_in_place_loop(cases, w, h):
    for kind in R.KINDS:
        y, u, v, side, want, _ = cases[(w, h, kind)]
        for a, b in zip(loop_in_place(y, u, v, side), want):
            assert np.array_equal(a, b), kind


@pytest.mark.parametrize("w,h", LOOP_SIZES)
def test_statement_equals_the_areas_filtered_independently(cases, w, h):
    for kind in R.KINDS:
        y, u, v, side, want, _ = cases[(w, h, kind)]
        for a, b in zip(loop_by_areas(y, u, v, side), want):
            assert np.array_equal(a, b), kind


def test_null_forms_of_the_loop_and_the_statement_agree():
    y, u, v, side = R.case("blocks", 64, 64)
    for name in ("cls", "intra", "nnz", "qps", "mv"):
        s = side.replace(**{name: None, "qp": 33})
        for a, b in zip(loop_in_place(y, u, v, s), _statement(y, u, v, s)[0]):
            assert np.array_equal(a, b), name


# ---- 3: properties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", R.SIZES)
def test_a_constant_plane_is_unchanged(cases, w, h):
    y, u, v, _, got, _ = cases[(w, h, "constant")]
    assert len(np.unique(y)) == 1
    for a, b in zip(got, (y, u, v)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("w,h", R.SIZES)
def test_all_zero_bs_is_the_identity(cases, w, h):
    y, u, v, side = cases[(w, h, "blocks")][:4]
    got, counts = _statement(y, u, v, side.replace(intra=None, nnz=np.zeros_like(side.nnz), mv=None))
    assert counts["luma_v"]["bs1"] == counts["luma_v"]["bs2"] == counts["u_h"]["filtered"] == 0
    for a, b in zip(got, (y, u, v)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("w,h", R.SIZES)
def test_beta_zero_is_the_identity_on_luma(cases, w, h):
    y, u, v, side = cases[(w, h, "blocks")][:4]
    got, counts = _statement(y, u, v, side.replace(qps=None, qp=15, beta_offset_div2=0))
    assert counts["luma_v"]["bs1"] + counts["luma_v"]["bs2"] > 0
    assert np.array_equal(got[0], y)


@pytest.mark.parametrize("w,h", R.SIZES + R.COMPOSITE)
def test_changes_stay_next_to_the_grid(cases, w, h):
    """no sample further than 3 (luma) or 1 (chroma) from a grid edge changes; a border row or column changes only through the
    interior edges that cross it: the sample must then lie within that reach of an edge in the OTHER direction"""
    for kind in R.KINDS:
        y, u, v, _, got, _ = cases[(w, h, kind)]
        for src, out, reach in ((y, got[0], 3), (u, got[1], 1), (v, got[2], 1)):
            ph, pw = src.shape
            near = lambda n: np.array([any(8 * e - reach <= i < 8 * e + reach for e in range(1, n // 8)) for i in range(n)])
            near_v, near_h = near(pw)[None, :], near(ph)[:, None]           # within reach of a vertical / horizontal interior edge
            changed = src != out
            assert not (changed & ~(near_v | near_h)).any(), kind
            assert not (changed[[0, -1], :] & ~near_v).any() and not (changed[:, [0, -1]] & ~near_h).any(), kind


# ---- 4: coverage of the recipes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", R.SIZES + R.COMPOSITE)
def test_recipes_cover_the_statement(cases, w, h):
    total = R.new_counts()
    for kind in R.KINDS:
        R.add_counts(total, cases[(w, h, kind)][5])
    R.assert_coverage(w, h, total)


# ---- 5: the surface ----------------------------------------------------------------------------------------------------------------------------
CALLS = ("xDeblockLumaGpu", "xDeblockChromaGpu", "xDeblockGpu")


def test_header_declares_and_library_exports_the_calls():
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    assert "typedef struct x266_deblock_t" in hdr
    for name in CALLS:
        assert re.search(r"int %s\(x266hip_ctx \*ctx, const x266_ref_block_t \*d_in, int width, int height, const x266_deblock_t \*p,\s*"
                         r"x266_ref_block_t \*d_out, void \*stream\);" % name, hdr), name
    lib = os.path.join(ROOT, "x266_amd", "libx266hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    handle = ctypes.CDLL(lib)
    for name in CALLS:
        assert hasattr(handle, name), name
