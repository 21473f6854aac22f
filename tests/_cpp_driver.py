"""The stand-alone C++ drivers under tests/cpp/: build one with g++ (plain, or with the address and undefined-behaviour sanitizers --
each driver is a program with its own main, nothing is preloaded), run it, and read what tests/cpp/struct_rules_check.cpp prints about
the calls that take their device pointers in a host-read struct.  g++ only: no GPU, no HIP."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def build(tmp_path, driver, extra_flags=(), source=None):
    """(executable, the compiler's CompletedProcess) of tests/cpp/<driver>.cpp, or of `source` (a driver a test wrote itself)"""
    exe = os.path.join(str(tmp_path), driver + ("_san" if extra_flags else ""))
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra"] + list(extra_flags) + ["-I", os.path.join(ROOT, "x266_amd", "csrc"),
                        "-o", exe, str(source) if source else os.path.join(ROOT, "tests", "cpp", driver + ".cpp")], capture_output=True, text=True)
    return exe, r


def run(exe, verdict="the argument rules hold"):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-4000:])
    assert verdict in out.stdout
    return out.stdout


def build_and_run_sanitized(tmp_path, driver):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime")
    exe, r = build(tmp_path, driver, SANITIZE + ["-fno-omit-frame-pointer", "-g"])
    assert r.returncode == 0, r.stderr[-4000:]
    return run(exe)


@functools.lru_cache(maxsize=None)
def struct_rules_output():
    """what the plain build of the struct calls' driver prints; built and run once for all the tests that read it"""
    where = tempfile.mkdtemp(prefix="struct_rules_")
    atexit.register(shutil.rmtree, where, ignore_errors=True)
    exe, r = build(where, "struct_rules_check")
    assert r.returncode == 0, r.stderr[-4000:]
    assert not r.stderr.strip(), r.stderr[-4000:]                              # the shared arithmetic compiles without a warning as plain C++
    return run(exe)


def struct_call_lines():
    """{call: {field: (alignment, optional, output)}} from the driver's lines "name: d_x 16 in, d_y 4 opt out", fields in printed order"""
    got = {}
    for name, items in re.findall(r"^(x\w+): (.*)$", struct_rules_output(), re.M):
        got[name] = {}
        for item in items.split(", "):
            m = re.fullmatch(r"(d_\w+) (\d+) (opt )?(in|out)", item)
            assert m, (name, item)
            got[name][m.group(1)] = (int(m.group(2)), bool(m.group(3)), m.group(4) == "out")
    return got


def header_struct_fields(struct):
    """{field: (alignment, "or NULL" stated, comment)} of the struct's device pointers as include/x266hip.h comments them, in struct order"""
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
    fields = {}
    for name, comment in re.findall(r"\*\s*(d_\w+);\s*/\*(.*?)\*/", body, re.S):
        m = re.search(r"(\d+)-byte aligned", comment)
        assert m or "any alignment" in comment, name
        fields[name] = (int(m.group(1)) if m else 1, "or NULL" in comment, comment)
    return fields


def assert_driver_follows_header(struct, calls, outputs_marked=False, may_be_null=()):
    """The driver's line of every call of the family names fields of the struct, in struct order, at the alignment the field's comment
    states, optional exactly where it states "or NULL" (or for the (call, field) pairs of may_be_null, which the comment words otherwise);
    together the lines cover every pointer of the struct.  outputs_marked: the comments say "output" where the call writes."""
    stated, lines = header_struct_fields(struct), struct_call_lines()
    covered = set()
    for call in calls:
        assert call in lines, call
        assert list(lines[call]) == [f for f in stated if f in lines[call]], (call, list(lines[call]))
        for field, (align, optional, output) in lines[call].items():
            assert align == stated[field][0], (call, field)
            assert optional == (stated[field][1] or (call, field) in may_be_null), (call, field)
            if outputs_marked:
                assert output == ("output" in stated[field][2]), (call, field)
        covered |= set(lines[call])
    assert covered == set(stated), covered ^ set(stated)
