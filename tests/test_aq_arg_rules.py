"""CPU: the argument rules of xAqStatsGpu and xAqDecideGpu (x266_amd/csrc/x266_args.hpp: aq_stats, aq_decide) against the contract as
tests/cpp/aq_rules_check.cpp writes it down: a base tuple, single perturbations, made-up addresses, the largest frame an int describes.
The driver is a stand-alone program, built twice -- plain, and with the address and undefined-behaviour sanitizers.  The two calls keep
their device pointers in a host-read struct, so the table of tests/cpp/arg_rules_check.cpp does not count them; the surface tests here
do what tests/test_arg_rules.py does for the calls of that table.  g++ only: no GPU, no HIP."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CALLS = ("xAqStatsGpu", "xAqDecideGpu")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra"] + extra + ["-I", os.path.join(ROOT, "x266_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "aq_rules_check.cpp")], capture_output=True, text=True)
    return exe, r


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-4000:])
    assert "the argument rules hold" in out.stdout
    return out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_rules_hold(tmp_path):
    exe, r = _build(tmp_path, "aq_rules_check", [])
    assert r.returncode == 0, r.stderr[-4000:]
    text = _run(exe)
    checks = int(re.search(r"(\d+) checks, 0 failures", text).group(1))
    assert checks >= 250, checks                                              # a walk that shrank must not pass quietly


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_rules_hold_under_the_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime")
    exe, r = _build(tmp_path, "aq_rules_check_san", SANITIZE + ["-fno-omit-frame-pointer", "-g"])
    assert r.returncode == 0, r.stderr[-4000:]
    _run(exe)


def test_the_header_declares_the_calls_outside_the_one_table():
    """context first, stream last, the device pointers in the struct: the parser of the one table must not count them, and the
    struct's field comments state the alignments the driver holds"""
    from test_gpu_placement import device_entry_points, header_alignments
    declared = device_entry_points()
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    for name in CALLS:
        assert name not in declared and name not in header_alignments(every=True), name
        assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_aq_t \*p, void \*stream\);" % name, hdr), name
    assert re.search(r"int xAqTotalsChunk\(void\);", hdr)
    assert re.search(r"int xWeightsFromTotals\(const int64_t cur\[8\], const int64_t ref\[8\], int list, x266_wp_t \*wp\);", hdr)
    body = re.search(r"typedef struct x266_aq_t \{(.*?)\} x266_aq_t;", hdr, re.S).group(1)
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"\*\s*(d_\w+);[^\n]*?(\d+)-byte aligned", body)}
    assert stated == {"d_src": 16, "d_tile": 16, "d_total": 8, "d_offset": 2}, stated
    assert re.search(r"\*\s*d_qp;[^\n]*any alignment", body)
    driver = open(os.path.join(ROOT, "tests", "cpp", "aq_rules_check.cpp")).read()
    for field, align in list(stated.items()) + [("d_qp", 1)]:
        assert re.search(r'\{"%s", %d,' % (field, align), driver), field
    rec = re.search(r"typedef struct x266_aq_tile_t \{(.*?)\} x266_aq_tile_t;", hdr, re.S).group(1)
    assert re.findall(r"\b([a-z0-9_]+)[,;]", rec) == ["sum_y", "ssq_y", "sum_u", "ssq_u", "sum_v", "ssq_v", "energy", "log2_q8"]


def test_the_library_exports_the_calls_and_they_refuse_null():
    import x266_amd
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in CALLS + ("xAqTotalsChunk", "xWeightsFromTotals"):
        assert name in exported and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name                   # bound with argument types
    p = x266_amd.Codec.aq_params(width=48, height=80, mode=2, strength_q8=300, qp=31, chroma_qp_offset=-3)
    assert ctypes.sizeof(x266_amd.AqParams) == 64 and (p.width, p.height, p.mode, p.strength_q8, p.qp, p.chroma_qp_offset) == (48, 80, 2, 300, 31, -3)
    assert not p.d_src and not p.d_qp
    assert [f[0] for f in x266_amd.AqParams._fields_[:5]] == ["d_src", "d_tile", "d_total", "d_offset", "d_qp"]
    assert x266_amd.AQ_TILE_DTYPE.itemsize == 32 and x266_amd.AQ_TILE_DTYPE.names[6:] == ("energy", "log2_q8")
    for name in CALLS:
        fn = getattr(lib, name)
        assert fn.argtypes[1] is ctypes.POINTER(x266_amd.AqParams)
        assert fn(None, ctypes.byref(p), None) == -1, name                     # a NULL context is refused, not dereferenced
        assert fn(None, None, None) == -1, name                                # ... and so is a NULL p
    chunk = lib.xAqTotalsChunk()
    assert chunk >= 64 and chunk % 64 == 0 and chunk == x266_amd.aq_totals_chunk()
    assert lib.xWeightsFromTotals(None, None, 0, None) == -1
    for method in ("aq_params", "aq_stats", "aq_decide", "aq_stats_dev", "aq_decide_dev", "weights_from_totals"):
        assert callable(getattr(x266_amd.Codec, method)), method
