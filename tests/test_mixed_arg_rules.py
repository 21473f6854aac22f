"""CPU: the surface of mixed inter / intra frame coding, xDct32CodeMixedFrameGpu: header, struct layout, bindings, and that the per-wave
pieces exist once.  The call keeps its device pointers in a host-read struct; tests/cpp/struct_rules_check.cpp holds its argument rules
(x266_amd/csrc/x266_args.hpp: mixed_code_frame) and tests/test_struct_arg_rules.py runs it.  No GPU, no HIP."""
import ctypes
import os
import re
import subprocess

import pytest

import _cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "xDct32CodeMixedFrameGpu"
ALIGN = {"d_cur": 16, "d_pred": 16, "d_qp": 1, "d_kind_in": 1, "d_mode_in": 1, "d_level": 16, "d_nnz": 4, "d_kind": 1, "d_mode": 1, "d_cost": 4, "d_recon": 16}
OPTIONAL = ("d_qp", "d_kind_in", "d_mode_in", "d_nnz", "d_cost")
FIELDS = list(ALIGN) + ["width", "height", "qp", "rounding", "intra_penalty"]


@_cpp_driver.needs_gxx
def test_the_header_declares_the_call_outside_the_one_table():
    """context first, stream last, the device pointers in the struct: the parser of the one table must not count it, and the struct's
    field comments state the alignments the driver holds and "or NULL" where that applies"""
    from test_gpu_placement import device_entry_points, header_alignments
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    assert "mixed inter / intra coding of a frame: intra 32x32 regions in P- and B-frames" in hdr
    assert CALL not in device_entry_points() and CALL not in header_alignments(every=True)
    assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_mixed_t \*p, void \*stream\);" % CALL, hdr)
    body = re.search(r"typedef struct x266_mixed_t \{(.*?)\} x266_mixed_t;", hdr, re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == FIELDS
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"\*\s*(d_\w+);[^\n]*?(\d+)-byte aligned", body)}
    assert stated == ALIGN, stated
    for field in ALIGN:
        assert bool(re.search(r"\*\s*%s;[^\n]*or NULL" % field, body)) == (field in OPTIONAL), field
    _cpp_driver.assert_driver_follows_header("x266_mixed_t", (CALL,), outputs_marked=True)
    assert {f for f, (_, optional, _) in _cpp_driver.struct_call_lines()[CALL].items() if optional} == set(OPTIONAL)
    for consequence in ("(a) with every kind 0", "(b) with every kind 1", "(c) a region's result depends only on regions before it",
                        "(d) entries 0..3 of every CTU of d_kind"):                # the consequences the tests rely on
        assert consequence in hdr, consequence


def test_the_shared_pieces_exist_once():
    """the per-wave pieces are defined once and used by both the intra call's kernel and the mixed call's kernels, and the inter prediction
    is scored by the function that scores the intra modes"""
    csrc = os.path.join(ROOT, "x266_amd", "csrc")
    sources = {n: open(os.path.join(csrc, n)).read() for n in os.listdir(csrc) if n.endswith((".hip", ".hpp", ".cpp"))}
    everything = "\n".join(sources.values())
    for name in ("gather_set", "luma_availability", "chroma_availability", "predict_fragment", "wave_slot", "interleave_chroma", "sample_offset",
                 "code_region", "region_quant", "intra_score_modes", "score_tiles", "cost_stage_source", "cost_window", "predict_line16"):
        assert len(re.findall(r"__device__ __forceinline__ [^\n(]*\b%s\(" % name, everything)) == 1, name
    frame = sources["intra_frame_kernels.hip"]
    kernels = re.split(r"\n(?=__global__ )", frame)
    body = {re.search(r"void (\w+)\(", k).group(1): k for k in kernels[1:]}
    assert {"intra_frame_step_kernel", "mixed_frame_step_kernel", "mixed_inter_regions_kernel"} <= set(body)
    for name in ("gather_set", "luma_availability", "chroma_availability", "predict_fragment", "wave_slot", "interleave_chroma", "code_region",
                 "intra_score_modes"):
        assert name + "(" in body["intra_frame_step_kernel"] and name + "(" in body["mixed_frame_step_kernel"], name
    assert "code_region(" in body["mixed_inter_regions_kernel"] and "score_tiles(" in body["mixed_frame_step_kernel"]
    assert "score_tiles(" in sources["x266_intra.hpp"].split("void intra_score_modes(")[1]     # the modes' scores come from the same function


def test_the_library_exports_the_call_and_it_refuses_null():
    import x266_amd
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert CALL in exported and hasattr(lib, CALL)
    fn = getattr(lib, CALL)
    assert fn.argtypes is not None and fn.argtypes[1] is ctypes.POINTER(x266_amd.MixedParams)
    p = x266_amd.Codec.mixed_params(width=192, height=128, qp=22, rounding=171, intra_penalty=4096, d_pred=4096)
    assert ctypes.sizeof(x266_amd.MixedParams) == 11 * 8 + 5 * 4 + 4
    assert (p.width, p.height, p.qp, p.rounding, p.intra_penalty) == (192, 128, 22, 171, 4096)
    assert not p.d_cur and p.d_pred == 4096 and not p.d_cost
    assert [f[0] for f in x266_amd.MixedParams._fields_] == FIELDS
    with pytest.raises(TypeError):
        x266_amd.Codec.mixed_params(d_nothing=1)
    assert fn(None, ctypes.byref(p), None) == -1                              # a NULL context is refused, not dereferenced
    assert fn(None, None, None) == -1                                         # ... and so is a NULL p
    for method in ("mixed_params", "dct32_code_mixed_frame_dev", "code_mixed_frame"):
        assert callable(getattr(x266_amd.Codec, method)), method
