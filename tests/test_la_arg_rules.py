"""CPU: the surface of the five lookahead calls and of xSceneCutFromTotals: header, struct layout, exports, bindings, and the scene cut's
refusals and decisions through the ABI.  The calls keep their device pointers in a host-read struct; tests/cpp/struct_rules_check.cpp
holds their argument rules (x266_amd/csrc/x266_args.hpp: la_downscale, la_intra_costs, la_frame_cost, la_propagate, la_tree_qp,
scene_cut_from_totals) and tests/test_struct_arg_rules.py runs it.  No GPU, no HIP."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("xLaDownscaleGpu", "xLaIntraCostsGpu", "xLaFrameCostGpu", "xLaPropagateGpu", "xLaTreeQpGpu")
ALIGN = {"d_src": 16, "d_low": 16, "d_intra": 4, "d_inter0": 8, "d_inter1": 8, "d_block": 16, "d_total": 8, "d_prop": 8, "d_prop_ref0": 8, "d_prop_ref1": 8,
         "d_aq_offset": 2, "d_offset": 2}
FIELDS = ["d_src", "d_low", "d_intra", "d_mode", "d_inter0", "d_inter1", "d_block", "d_total", "d_prop", "d_prop_ref0", "d_prop_ref1", "d_aq_offset", "d_offset",
          "d_qp", "width", "height", "intra_penalty", "strength_q8", "qp", "chroma_qp_offset"]


@_cpp_driver.needs_gxx
def test_the_header_declares_the_calls_outside_the_one_table():
    """context first, stream last, the device pointers in the struct: the parser of the one table must not count them, and the
    struct's field comments state the alignments the driver holds"""
    from test_gpu_placement import device_entry_points, header_alignments
    declared = device_entry_points()
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    assert "lookahead: half-size frames, frame costs, scene cuts and the propagation tree" in hdr
    for name in CALLS:
        assert name not in declared and name not in header_alignments(every=True), name
        assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_la_t \*p, void \*stream\);" % name, hdr), name
    assert re.search(r"int xLaTotalsChunk\(void\);", hdr)
    assert re.search(r"int xSceneCutFromTotals\(const int64_t total\[8\], int threshold_q8, int frames_since_key, int min_keyint, int max_keyint\);", hdr)
    body = re.search(r"typedef struct x266_la_t \{(.*?)\} x266_la_t;", hdr, re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == FIELDS
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"\*\s*(d_\w+);[^\n]*?(\d+)-byte aligned", body)}
    assert stated == ALIGN, stated
    for field in ("d_mode", "d_qp"):
        assert re.search(r"\*\s*%s;[^\n]*any alignment" % field, body), field
    for field in ("d_mode", "d_inter0", "d_inter1", "d_prop", "d_prop_ref0", "d_prop_ref1", "d_aq_offset", "d_offset", "d_qp"):
        assert re.search(r"\*\s*%s;[^\n]*or NULL" % field, body), field            # ... and which fields may be NULL
    for field in ("d_src", "d_low", "d_intra", "d_block", "d_total"):
        assert not re.search(r"\*\s*%s;[^\n]*NULL" % field, body), field
    _cpp_driver.assert_driver_follows_header("x266_la_t", CALLS)
    rec = re.search(r"typedef struct x266_la_block_t \{(.*?)\} x266_la_block_t;", hdr, re.S).group(1)
    assert re.findall(r"\b([a-z0-9_]+)[,;]", re.sub(r"/\*.*?\*/", "", rec)) == ["cost", "intra", "mvx", "mvy", "kind", "mode", "reserved"]


def test_the_library_exports_the_calls_and_they_refuse_null():
    import x266_amd
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in CALLS + ("xLaTotalsChunk", "xSceneCutFromTotals"):
        assert name in exported and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name                   # bound with argument types
    p = x266_amd.Codec.la_params(width=96, height=160, intra_penalty=300, strength_q8=512, qp=31, chroma_qp_offset=-3, d_low=4096)
    assert ctypes.sizeof(x266_amd.LaParams) == 136
    assert (p.width, p.height, p.intra_penalty, p.strength_q8, p.qp, p.chroma_qp_offset) == (96, 160, 300, 512, 31, -3)
    assert not p.d_src and p.d_low == 4096 and not p.d_qp
    assert [f[0] for f in x266_amd.LaParams._fields_] == FIELDS
    with pytest.raises(TypeError):
        x266_amd.Codec.la_params(d_nothing=1)
    assert x266_amd.LA_BLOCK_DTYPE.itemsize == 16 and x266_amd.LA_BLOCK_DTYPE.names == ("cost", "intra", "mvx", "mvy", "kind", "mode", "reserved")
    assert [x266_amd.LA_BLOCK_DTYPE.fields[n][1] for n in x266_amd.LA_BLOCK_DTYPE.names] == [0, 4, 8, 10, 12, 13, 14]
    for name in CALLS:
        fn = getattr(lib, name)
        assert fn.argtypes[1] is ctypes.POINTER(x266_amd.LaParams)
        assert fn(None, ctypes.byref(p), None) == -1, name                     # a NULL context is refused, not dereferenced
        assert fn(None, None, None) == -1, name                                # ... and so is a NULL p
    chunk = lib.xLaTotalsChunk()
    assert chunk >= 64 and chunk % 64 == 0 and chunk == x266_amd.la_totals_chunk()
    for method in ("la_params", "la_downscale", "la_intra_costs", "la_frame_cost", "la_propagate", "la_tree_qp", "la_downscale_dev", "la_intra_costs_dev",
                   "la_frame_cost_dev", "la_propagate_dev", "la_tree_qp_dev"):
        assert callable(getattr(x266_amd.Codec, method)), method


def test_scene_cut_refusals_and_decisions():
    """xSceneCutFromTotals through the ABI: every refusal of the header, and its decisions against the restatement"""
    import _la_ref as R
    import x266_amd
    lib = x266_amd.load_library()
    good = np.array([90000, 100000, 10, 40, 10, 95000, 97000, 60], np.int64)

    def call(total, *scalars):
        t = None if total is None else np.ascontiguousarray(total, np.int64)
        return lib.xSceneCutFromTotals(None if t is None else ctypes.c_void_p(t.ctypes.data), *scalars)

    assert call(None, 102, 100, 25, 250) == -1
    for scalars in ((-1, 100, 25, 250), (257, 100, 25, 250), (102, -1, 25, 250), (102, 100, 0, 250), (102, 100, -5, 250), (102, 100, 25, 24)):
        assert call(good, *scalars) == -1, scalars
    for i in range(8):
        bad = good.copy()
        bad[i] = -1
        assert call(bad, 102, 100, 25, 250) == -1, i
    for n in (0, (1 << 24) + 1):
        bad = good.copy()
        bad[7] = n
        assert call(bad, 102, 100, 25, 250) == -1, n
    for i in (0, 1):
        bad = good.copy()
        bad[i] = (1 << 40) + 1
        assert call(bad, 102, 100, 25, 250) == -1, i
    with pytest.raises(x266_amd.X266Error):
        x266_amd.scene_cut_from_totals(good, 300, 100, 25, 250)
    with pytest.raises(x266_amd.X266Error):
        x266_amd.scene_cut_from_totals(good[:7], 102, 100, 25, 250)
    # accepted at the edges of every range, and the decision is the restatement's
    r = np.random.RandomState(20)
    cases = [(good, 102, 100, 25, 250), (good, 0, 0, 1, 1), (good, 256, 2 ** 31 - 1, 1, 2 ** 31 - 1), (good, 256, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1),
             (good, 256, 2 ** 31 - 1, 1, 1)]
    for _ in range(400):
        t = good.copy()
        t[1] = r.randint(0, 1 << 30)
        t[0] = int(t[1] * r.uniform(0.5, 1.1))
        lo = int(r.randint(1, 60))
        cases.append((t, int(r.randint(0, 257)), int(r.randint(0, 400)), lo, lo + int(r.randint(0, 300))))
    big = good.copy()
    big[0] = big[1] = 1 << 40
    cases.append((big, 256, 3, 25, 250))
    seen = set()
    for total, *scalars in cases:
        want = R.scene_cut(total, *scalars)
        assert call(total, *scalars) == want, (total, scalars)
        assert x266_amd.scene_cut_from_totals(total, *scalars) == bool(want)
        seen.add(want)
    assert seen == {0, 1}
