"""CPU: the reference statement of tests/_intra_frame_ref.py against itself -- the gather rule against a second statement written
from the definition (a sample is available iff its 32x32 block is inside the frame and is coded earlier), the conditions the
inputs of tests/test_gpu_intra_frame.py must meet for that test to mean something, causality, and the modes fed back."""
import numpy as np
import pytest

import _intra_frame_ref as R


# ---- the gather rule, a second time ---------------------------------------------------------------------------------------------------
def _coding_number(bx, by, luma):
    """position of 32x32 block (bx, by) in coding order: CTUs in raster order (any row stride larger than a row), quadrants 0..3 inside"""
    if not luma:
        return by * 4096 + bx                                               # a chroma plane has one block per CTU
    return ((by >> 1) * 4096 + (bx >> 1)) * 4 + 2 * (by & 1) + (bx & 1)


def _gather_by_definition(plane, bx, by, luma):
    hh, ww = plane.shape
    x0, y0 = 32 * bx, 32 * by
    me = _coding_number(bx, by, luma)
    scan = [(x0 - 1, y0 + 63 - i) for i in range(64)] + [(x0 - 1, y0 - 1)] + [(x0 + i, y0 - 1) for i in range(64)]
    val = []
    for x, y in scan:
        inside = 0 <= x < ww and 0 <= y < hh
        val.append(int(plane[y, x]) if inside and _coding_number(x // 32, y // 32, luma) < me else None)
    known = [i for i in range(129) if val[i] is not None]
    out = []
    for i in range(129):
        if not known:
            out.append(128)
        elif i < known[0]:
            out.append(val[known[0]])
        else:
            out.append(val[max(k for k in known if k <= i)])
    return np.array(out[63::-1] + out[64:], np.uint8)


@pytest.mark.parametrize("w,h", R.SIZES)
def test_gather_equals_the_definition(w, h):
    planes = R.case("noise", w, h, seed=40 + w + h)
    for comp in range(3):
        got = R.refs_from_planes(planes, w, h, comp)
        assert got.shape == ((w // 64) * (h // 64) * (4 if comp == 0 else 1), 144) and not got[:, 129:].any()
        i = 0
        for cy in range(h // 64):
            for cx in range(w // 64):
                for q in range(4 if comp == 0 else 1):
                    bx, by = (2 * cx + (q & 1), 2 * cy + (q >> 1)) if comp == 0 else (cx, cy)
                    assert np.array_equal(got[i, :129], _gather_by_definition(planes[comp], bx, by, comp == 0)), (comp, cx, cy, q)
                    i += 1


def test_sizes_contain_every_neighbour_case():
    seen = set()
    for w, h in R.SIZES:
        for by in range(h // 32):
            for bx in range(w // 32):
                seen.add((2 * (by & 1) + (bx & 1),) + tuple(bool(a) for a in R.luma_availability(bx, by, w // 32, h // 32)))
    assert (0, False, False, False, False, False) in seen                   # no neighbour at all
    assert (0, True, True, True, True, True) in seen                        # quadrant 0 with BL from the left CTU
    assert (1, False, True, True, True, True) in seen and (1, False, True, True, True, False) in seen   # TR from CTU (cx+1, cy-1) / outside
    assert (0, True, True, False, False, False) in seen and (2, False, False, False, True, True) in seen   # the top row with a left CTU, the left edge


# ---- what the inputs must provoke -----------------------------------------------------------------------------------------------------
def test_oriented_input_spreads_the_luma_modes(oracle):
    modes = R.coded(oracle, "oriented", 192, 128).modes[:, :4].ravel().tolist()
    print("luma modes", sorted(set(modes)))
    assert len(set(modes)) >= 6
    assert any(m in (0, 1) for m in modes) and any(2 <= m <= 17 for m in modes) and any(18 <= m <= 34 for m in modes)


def test_every_chroma_candidate_position_wins(oracle):
    pos = set()
    for w, h in ((128, 128), (192, 128)):
        pos |= set(R.coded(oracle, "oriented", w, h).chroma_pos.tolist())
    print("chroma candidate positions", sorted(pos))
    assert pos == {0, 1, 2, 3, 4}


def test_flat_input_takes_the_first_mode_and_codes_nothing(oracle):
    for w, h in R.SIZES:
        c = R.coded(oracle, "flat", w, h)
        assert not c.modes.any() and not c.nnz.any() and not c.chroma_pos.any()
        assert all((p == 128).all() for p in c.planes)


def test_some_case_has_an_empty_region_next_to_a_coded_one(oracle):
    found = False
    for kind in R.KINDS:
        for qp in (22, 37, 51):
            nnz = R.coded(oracle, kind, 192, 128, qp).nnz.ravel()           # regions in the order of d_nnz
            found = found or bool(((nnz[:-1] == 0) != (nnz[1:] == 0)).any())
    assert found


# ---- the loop is closed ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_causality(oracle, kind):
    """every block's reconstruction = clip8(prediction(mode, the set gathered from the FINAL reconstruction) + its residual): what a
    block referred to was final when it was coded"""
    import _quant_ref as Q
    w, h = 192, 128
    c = R.coded(oracle, kind, w, h)
    nx = w // 64
    sets = [R.refs_from_planes(c.planes, w, h, comp) for comp in range(3)]
    for ctu in range(nx * (h // 64)):
        cx, cy = ctu % nx, ctu // nx
        for q in range(6):
            refs = sets[0][4 * ctu + q] if q < 4 else sets[q - 3][ctu]
            assert np.array_equal(refs[:129], c.refs[ctu, q]), (ctu, q)
            pred = oracle.intra32_predict(refs[None, :129], c.modes[ctu, q:q + 1]).reshape(32, 32)
            res = oracle.dct32_inv(Q.dequant(c.levels[ctu, q], 5, 22).astype(np.int16)[None]).reshape(32, 32)
            if q < 4:
                x0, y0 = 64 * cx + 32 * (q & 1), 64 * cy + 32 * (q >> 1)
            else:
                x0, y0 = 32 * cx, 32 * cy
            got = c.planes[max(q - 3, 0)][y0:y0 + 32, x0:x0 + 32]
            assert np.array_equal(got, np.clip(pred.astype(np.int32) + res, 0, 255)), (ctu, q)


@pytest.mark.parametrize("kind", ("oriented", "extreme"))
def test_decided_modes_fed_back_reproduce_every_output(oracle, kind):
    w, h = 192, 128
    c = R.coded(oracle, kind, w, h)
    modes = c.modes.copy()
    modes[:, 5] = 99                                                        # entry 5 is ignored
    d = R.code_frame(oracle, R.case(kind, w, h), w, h, None, 22, 171, modes_in=modes)
    assert np.array_equal(c.levels, d.levels) and np.array_equal(c.nnz, d.nnz) and np.array_equal(c.modes, d.modes)
    assert all(np.array_equal(a, b) for a, b in zip(c.planes, d.planes))
