"""CPU: the device's frame-quality arithmetic (x266_amd/csrc/x266_quality.hpp) run as plain C++ by tests/cpp/quality_window_check.cpp, a
stand-alone program built twice -- plain, and with the address and undefined-behaviour sanitizers -- and every value it prints held
against tests/_quality_ref.py.  g++ only: no GPU, no HIP."""
import functools
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _cpp_driver
import _quality_ref as R

DRIVER = "quality_window_check"
VERDICT = "the window arithmetic holds"
LINE = re.compile(r"^window (\w+) a=([0-9a-f]{128}) b=([0-9a-f]{128}) s1=(\d+) s2=(\d+) ss=(\d+) s12=(\d+) sse=(\d+) cn=(-?\d+) q=(-?\d+)$", re.M)
WINDOW_FLOOR = 90                                                           # the finished driver prints 96: a list that shrank must not pass quietly


def check(text):
    """every printed window against the reference; {name: (cn, q)}"""
    seen = {}
    for name, a, b, s1, s2, ss, s12, sse, cn, q in LINE.findall(text):
        a, b = np.frombuffer(bytes.fromhex(a), np.uint8), np.frombuffer(bytes.fromhex(b), np.uint8)
        sums = R.sums_of(a, b)
        assert sums == (int(s1), int(s2), int(ss), int(s12)), name
        assert int(sse) == int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()), name
        want_q, want_cn, _ = R.window(*sums)
        assert (int(cn), int(q)) == (want_cn, want_q), (name, cn, q, want_cn, want_q)
        seen[name] = (int(cn), int(q))
    assert len(seen) == int(re.search(r"^windows (\d+)$", text, re.M).group(1)) >= WINDOW_FLOOR
    return seen


@functools.lru_cache(None)
def plain_output():
    with tempfile.TemporaryDirectory(prefix="quality_window_") as where:
        exe, r = _cpp_driver.build(where, DRIVER)
        assert r.returncode == 0, r.stderr[-4000:]
        assert not r.stderr.strip(), r.stderr[-4000:]                        # the shared arithmetic compiles without a warning as plain C++
        return _cpp_driver.run(exe, VERDICT)


@_cpp_driver.needs_gxx
def test_every_printed_window_is_the_references():
    seen = check(plain_output())
    assert seen["identical_flat"][1] == 1 << 30 and seen["zeros_against_255"][1] == 1677 == seen["255_against_zeros"][1]
    assert seen["checkerboard_against_inverse"] == (-132935237, -1069943477)
    for n in range(24):
        assert seen["noise_%d_identical" % n][1] == 1 << 30
        assert seen["noise_%d_inverse" % n][0] < 0 and seen["noise_%d_inverse" % n][1] < 0      # the signed quotient, truncated toward zero
    assert any(cn < 0 for name, (cn, q) in seen.items() if re.fullmatch(r"noise_\d+", name))
    assert all(0 < seen["distorted_%d" % n][1] < 1 << 30 for n in range(8))
    assert {"flat_0_plus_1", "flat_1_minus_1", "flat_254_plus_1", "flat_255_minus_1"} <= set(seen)


@_cpp_driver.needs_gxx
def test_the_same_under_the_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + _cpp_driver.SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime")
    exe, r = _cpp_driver.build(tmp_path, DRIVER, _cpp_driver.SANITIZE + ["-fno-omit-frame-pointer", "-g"])
    assert r.returncode == 0, r.stderr[-4000:]
    text = _cpp_driver.run(exe, VERDICT)
    check(text)
    assert text == plain_output()
