"""CPU: the argument rules of the five adaptive-loop-filter calls (x266_amd/csrc/x266_args.hpp) against the contract as
tests/cpp/alf_rules_check.cpp writes it down -- a stand-alone program, built plain and with the address and undefined-behaviour
sanitizers, and run as itself -- and the alignments it states against the header's declarations; a NULL context is refused.
The family's rules are held here and not in tests/cpp/arg_rules_check.cpp: the header declares the five calls in a column, with
blanks between the name and its parenthesis, which that older table's "every declared call has a row" pattern does not count, and
this file checks instead that every xAlf* declaration has its row in this driver."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
STATED = {"xAlfClassifyGpu": {"d_dec": 16, "d_class": 1},
          "xAlfStatsGpu": {"d_org": 16, "d_dec": 16, "d_class": 1, "d_stats": 4},
          "xAlfSumStatsGpu": {"d_stats": 4, "d_mask": 1, "d_total": 8},
          "xAlfDecideGpu": {"d_stats": 4, "d_luma": 4, "d_chroma": 4, "d_ctrl": 1},
          "xAlfApplyGpu": {"d_in": 16, "d_class": 1, "d_luma": 4, "d_chroma": 4, "d_ctrl": 1, "d_out": 16}}


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra"] + extra + ["-I", os.path.join(ROOT, "x266_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "alf_rules_check.cpp")], capture_output=True, text=True)
    return exe, r


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-4000:])
    assert "the adaptive loop filter argument rules hold" in out.stdout
    return out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_rules_hold_and_state_the_contracts_alignments(tmp_path):
    exe, r = _build(tmp_path, "alf_rules_check", [])
    assert r.returncode == 0, r.stderr[-4000:]
    lines = dict(re.findall(r"^(x\w+): (.*)$", _run(exe), re.M))
    got = {name: {k: int(v) for k, v in (i.split() for i in items.split(", "))} for name, items in lines.items()}
    assert got == STATED                                                    # frames 16, statistics 4, totals 8, filter arrays 4, byte arrays 1
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    assert "Frames are 16-byte aligned, d_stats 4, d_total 8, d_luma and d_chroma 4, the byte arrays (d_class, d_mask, d_ctrl) 1" in hdr
    assert set(re.findall(r"^int (xAlf\w+) *\(", hdr, re.M)) == set(STATED)  # every call of the family has its rules checked here
    for name, ptrs in STATED.items():
        decl = re.search(r"^int %s *\(([^;]*)\);" % name, hdr, re.M).group(1)
        for ptr in ptrs:
            assert re.search(r"\*\s*%s\b" % ptr, decl), (name, ptr)
        assert decl.count("*") == len(ptrs) + 2, (name, decl)                # ... besides ctx and stream


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_rules_hold_under_the_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime")
    exe, r = _build(tmp_path, "alf_rules_check_san", SANITIZE + ["-fno-omit-frame-pointer", "-g"])
    assert r.returncode == 0, r.stderr[-4000:]
    _run(exe)


def test_a_null_context_is_refused_not_dereferenced():
    import x266_amd
    x266_amd.build_library()
    lib = x266_amd.load_library()
    for name in STATED:
        fn = getattr(lib, name)
        assert fn(*[0 if t in (ctypes.c_int, ctypes.c_size_t) else None for t in fn.argtypes]) < 0, name
