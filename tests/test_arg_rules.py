"""CPU: the argument rules of the device entry points (x266_amd/csrc/x266_args.hpp: NULL, alignment, "the span fits in the address
space", "no output overlaps another buffer", sizes and scalar ranges) against the contract as tests/cpp/arg_rules_check.cpp writes
it down: a base tuple per entry point and single perturbations of it, with made-up addresses.  The driver is a stand-alone program,
built twice -- plain, and with the address and undefined-behaviour sanitizers -- and its per-entry-point alignment lines must be
the ones include/x266hip.h states and tests/test_gpu_placement.py places buffers at.  g++ only: no GPU, no HIP."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra"] + extra + ["-I", os.path.join(ROOT, "x266_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "arg_rules_check.cpp")], capture_output=True, text=True)
    return exe, r


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-4000:])
    assert "the argument rules hold" in out.stdout
    return out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_rules_hold_and_state_the_headers_alignments(tmp_path):
    exe, r = _build(tmp_path, "arg_rules_check", [])
    assert r.returncode == 0, r.stderr[-4000:]
    lines = dict(re.findall(r"^(x\w+): (.*)$", _run(exe), re.M))
    got = {name: {k: int(v) for k, v in (i.split() for i in items.split(", "))} for name, items in lines.items()}
    from test_gpu_placement import header_alignments
    stated = header_alignments()
    assert len(stated) >= 37
    assert {n: a for n, a in got.items() if n.endswith("Dev")} == stated
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    declared = set(re.findall(r"\b(x\w+(?:Dev|Gpu))\(", hdr))
    assert set(got) == declared, sorted(set(got) ^ declared)                  # a new entry point needs its rules checked here


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_rules_hold_under_the_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime")
    exe, r = _build(tmp_path, "arg_rules_check_san", SANITIZE + ["-fno-omit-frame-pointer", "-g"])
    assert r.returncode == 0, r.stderr[-4000:]
    _run(exe)
