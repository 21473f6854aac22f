"""CPU: the surface and the argument rules of xTransformDecideCtuTilesGpu: header, struct layout, export, bindings, and the rule
function of x266_amd/csrc/x266_args.hpp (transform_decide) against the contract as tests/cpp/tdecide_rules_check.cpp writes it down --
single perturbations of a base tuple with and without each optional buffer: alignment halves, saturating extents, every illegal
overlap, the mask rules.  The driver is a stand-alone program, built twice: plain, and with the address and undefined-behaviour
sanitizers.  g++ only: no GPU, no HIP."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import _cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "xTransformDecideCtuTilesGpu"
DRIVER = "tdecide_rules_check"
CHECK_FLOOR = 6500                                                        # the finished driver prints 6589: a walk that shrank must not pass quietly


@functools.lru_cache(None)
def driver_output():
    with tempfile.TemporaryDirectory(prefix="tdecide_rules_") as where:
        exe, r = _cpp_driver.build(where, DRIVER)
        assert r.returncode == 0, r.stderr[-4000:]
        assert not r.stderr.strip(), r.stderr[-4000:]                        # the shared arithmetic compiles without a warning as plain C++
        return _cpp_driver.run(exe)


def driver_fields():
    """{field: (alignment, optional, output)} from the driver's line, fields in printed order"""
    items = re.search(r"^%s: (.*)$" % CALL, driver_output(), re.M).group(1)
    got = {}
    for item in items.split(", "):
        m = re.fullmatch(r"(d_\w+) (\d+) (opt )?(in|out)", item)
        assert m, item
        got[m.group(1)] = (int(m.group(2)), bool(m.group(3)), m.group(4) == "out")
    return got


@_cpp_driver.needs_gxx
def test_the_rules_hold():
    text = driver_output()
    assert int(re.search(r"^checks x266_tdecide_t (\d+)$", text, re.M).group(1)) >= CHECK_FLOOR


@_cpp_driver.needs_gxx
def test_the_rules_hold_under_the_sanitizers(tmp_path):
    _cpp_driver.build_and_run_sanitized(tmp_path, DRIVER)


@_cpp_driver.needs_gxx
def test_the_header_declares_the_call_and_the_driver_follows_its_comments():
    """context first, stream last, the device pointers in the struct; every pointer field's comment states its alignment and "or NULL"
    exactly where the driver holds the field optional, in struct order"""
    from test_gpu_placement import device_entry_points, header_alignments
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    assert CALL not in device_entry_points() and CALL not in header_alignments(every=True)     # the one table's parser must not count it
    assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_tdecide_t \*p, void \*stream\);" % CALL, hdr)
    stated = _cpp_driver.header_struct_fields("x266_tdecide_t")
    held = driver_fields()
    assert list(stated) == list(held)
    assert {f: v[0] for f, v in stated.items()} == {"d_cur": 16, "d_pred": 16, "d_qp": 1, "d_cand": 2, "d_class": 1, "d_level": 16, "d_nnz": 4, "d_stat": 8,
                                                    "d_cost": 8}
    for field, (align, optional, output) in held.items():
        assert align == stated[field][0] and optional == stated[field][1], field
    assert {f for f, v in held.items() if v[2]} == {"d_class", "d_level", "d_nnz", "d_stat", "d_cost"}
    assert re.search(r"#define X266_TDECIDE_CLASSES 0x777F\b", hdr)
    body = re.search(r"typedef struct x266_tdecide_t \{(.*?)\} x266_tdecide_t;", hdr, re.S).group(1)
    assert re.search(r"uint16_t cand_luma, cand_chroma;", body) and re.search(r"uint16_t class_bits\[16\];", body)


def test_the_library_exports_the_call_and_it_refuses_null():
    import x266_amd
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert CALL in exported and hasattr(lib, CALL)
    fn = getattr(lib, CALL)
    assert fn.argtypes is not None and fn.argtypes[1] is ctypes.POINTER(x266_amd.TDecideParams)
    p = x266_amd.Codec.tdecide_params(width=144, height=80, qp=30, lam=368, cand_luma=0x28, class_bits=[5, 6, 7])
    assert ctypes.sizeof(x266_amd.TDecideParams) == 128 and x266_amd.TDecideParams.class_bits.offset == 92
    assert (p.width, p.height, p.qp, p.lambda_, p.cand_luma, p.cand_chroma) == (144, 80, 30, 368, 0x28, 0x777F)
    assert list(p.class_bits) == [5, 6, 7] + [0] * 13 and not p.d_level and not p.d_cost
    assert x266_amd.TDECIDE_CLASSES == 0x777F
    assert fn(None, ctypes.byref(p), None) == -1                              # a NULL context is refused, not dereferenced
    assert fn(None, None, None) == -1                                         # ... and so is a NULL p
    for method in ("tdecide_params", "transform_decide", "transform_decide_dev"):
        assert callable(getattr(x266_amd.Codec, method)), method


def test_the_kernel_is_composed_from_the_shared_pieces():
    """the transform and RDOQ pieces stand once, in shared headers that the Makefile tracks; rdoq_kernels.hip holds the decision kernel and
    defines none of them again"""
    csrc = os.path.join(ROOT, "x266_amd", "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("rdoq_kernels.hip", "transform_kernels.hip", "x266_transform_blocks.hpp",
                                                                     "x266_rdoq_blocks.hpp", "Makefile")}
    for piece in ("put_segment", "luma_residual16", "chroma_residual8", "copy_table", "fwd_tile_of_class", "fwd_tile_in_slot"):
        assert len(re.findall(r"__forceinline__ \w+ %s\(" % piece, text["x266_transform_blocks.hpp"])) == 1, piece
        for unit in ("rdoq_kernels.hip", "transform_kernels.hip"):
            assert not re.search(r"__forceinline__ \w+ %s\(" % piece, text[unit]), (unit, piece)
    for piece in ("rdoq_steps", "cg_place", "cg_bits", "rdoq_cg_from_lds", "rdoq_cg_to_lds"):
        assert len(re.findall(r"__forceinline__ \w+ %s\(" % piece, text["x266_rdoq_blocks.hpp"])) == 1, piece
        assert not re.search(r"__forceinline__ \w+ %s\(" % piece, text["rdoq_kernels.hip"]), piece
    hdr_line = re.search(r"^HDR\s*:=(.*)$", text["Makefile"], re.M).group(1)
    assert "$(HERE)x266_transform_blocks.hpp " in hdr_line and "$(HERE)x266_rdoq_blocks.hpp " in hdr_line
    assert "tdecide_kernel" in text["rdoq_kernels.hip"] and text["rdoq_kernels.hip"].count("rdoq_steps(") == 2
