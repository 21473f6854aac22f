"""CPU: the surface and the argument rules of xQualityStatsGpu and xQualityFromTotals: header, struct layout, exports, bindings, and the
rule functions of x266_amd/csrc/x266_args.hpp (quality_stats, quality_from_totals) against the contract as
tests/cpp/quality_rules_check.cpp writes it down -- single perturbations of a base tuple with and without d_total: alignment halves,
saturating extents, every illegal overlap, the flags, the totals' refusals.  The driver is a stand-alone program, built twice: plain, and
with the address and undefined-behaviour sanitizers.  g++ only: no GPU, no HIP."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import pytest

import _cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "xQualityStatsGpu"
DRIVER = "quality_rules_check"
CHECK_FLOOR = 850                                                         # the finished driver prints 883: a walk that shrank must not pass quietly


@functools.lru_cache(None)
def driver_output():
    with tempfile.TemporaryDirectory(prefix="quality_rules_") as where:
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
    assert int(re.search(r"^checks x266_quality_t (\d+)$", text, re.M).group(1)) >= CHECK_FLOOR


@_cpp_driver.needs_gxx
def test_the_rules_hold_under_the_sanitizers(tmp_path):
    _cpp_driver.build_and_run_sanitized(tmp_path, DRIVER)


@_cpp_driver.needs_gxx
def test_the_header_declares_the_calls_and_the_driver_follows_its_comments():
    """context first, stream last, the device pointers in the struct; every pointer field's comment states its alignment, "or NULL"
    exactly where the driver holds the field optional and "output" exactly where it holds it written, in struct order"""
    from test_gpu_placement import device_entry_points, header_alignments
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    assert CALL not in device_entry_points() and CALL not in header_alignments(every=True)     # the one table's parser must not count it
    assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_quality_t \*p, void \*stream\);" % CALL, hdr)
    assert re.search(r"int xQualityTotalsChunk\(void\);", hdr)
    assert re.search(r"int xQualityFromTotals\(const int64_t total\[8\], int width, int height, double psnr\[4\], double ssim\[3\]\);", hdr)
    stated = _cpp_driver.header_struct_fields("x266_quality_t")
    held = driver_fields()
    assert list(stated) == list(held) == ["d_src", "d_dec", "d_ctu", "d_total"]
    assert {f: v[0] for f, v in stated.items()} == {"d_src": 16, "d_dec": 16, "d_ctu": 16, "d_total": 8}
    for field, (align, optional, output) in held.items():
        assert align == stated[field][0] and optional == stated[field][1] and output == ("output" in stated[field][2]), field
    assert re.search(r"#define X266_QUALITY_SSE\s+1\b", hdr) and re.search(r"#define X266_QUALITY_SSIM\s+2\b", hdr)
    body = re.search(r"typedef struct x266_quality_ctu_t \{(.*?)\} x266_quality_ctu_t;", hdr, re.S).group(1)
    assert re.findall(r"\b(int64_t|uint32_t)\s+([^;]+);", body) == [("int64_t", "ssim[3]"), ("uint32_t", "sse[3]"), ("uint32_t", "win_y, win_c"), ("uint32_t", "reserved")]


def test_the_library_exports_the_calls_and_they_refuse_null():
    import x266_amd
    import x266_amd.quality as Q
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in (CALL, "xQualityTotalsChunk", "xQualityFromTotals"):
        assert name in exported and hasattr(lib, name), name
    fn = getattr(lib, CALL)
    assert fn.argtypes is not None and fn.argtypes[1] is ctypes.POINTER(x266_amd.QualityParams)
    assert ctypes.sizeof(x266_amd.QualityParams) == 48 and x266_amd.QualityParams.width.offset == 32 and x266_amd.QualityParams.flags.offset == 40
    assert x266_amd.QUALITY_CTU_DTYPE.itemsize == 48 and x266_amd.QUALITY_CTU_DTYPE.fields["sse"][1] == 24 and x266_amd.QUALITY_CTU_DTYPE.fields["win_y"][1] == 36
    assert (x266_amd.QUALITY_SSE, x266_amd.QUALITY_SSIM) == (1, 2)
    p = Q.quality_params(d_src=0x1000, d_ctu=0x3000, width=144, height=80)
    assert (p.d_src, p.d_dec, p.d_ctu, p.d_total, p.width, p.height, p.flags) == (0x1000, None, 0x3000, None, 144, 80, 3)
    assert Q.quality_params(flags=1).flags == 1
    assert fn(None, ctypes.byref(p), None) == -1                              # a NULL context is refused, not dereferenced
    assert fn(None, None, None) == -1                                         # ... and so is a NULL p
    assert lib.xQualityTotalsChunk() == Q.totals_chunk() > 0


def test_the_binding():
    """quality_params refuses an unknown field in the keyword builders' words; the numpy calls are module functions, and the Codec gains
    the one ..._dev method"""
    import x266_amd
    import x266_amd.quality as Q
    with pytest.raises(TypeError) as e:
        Q.quality_params(bogus=1, d_src=16)
    assert str(e.value) == "quality_params: no such field: ['bogus']"
    with pytest.raises(TypeError) as e:
        x266_amd.Codec.la_params(bogus=1)
    assert str(e.value) == "la_params: no such field: ['bogus']"             # the same text
    assert [n for n in dir(x266_amd.Codec) if "quality" in n.lower()] == ["quality_stats_dev"]
    for name in ("quality_params", "quality_stats", "totals_chunk", "from_totals"):
        assert callable(getattr(Q, name)), name
    src = open(os.path.join(ROOT, "x266_amd", "quality.py")).read()
    assert "codec._frame(" in src and "codec._fetch(" in src and "Codec._keyword_params(" in src    # the shared pieces, not copies
