"""Layout of the bucket form of the group sums (hbbft_amd/csrc/group_bucket.hpp, compiled with g++): for
the digit-boundary scalars 1, 2, 3, 2^64 - 1, 2^64, |x| - 1, |x|, |x| + 1, |x|^2 - 1, |x|^2, 2^126, 3 * 2^126,
2^128 - 1 and 10^4 seeded random ones the G1 digits recombine to r, the G2 digits to r through
d0 + d1 |x| + d2 |x|^2, and every digit is < 4; the thread map is a bijection onto (window, slice), the LDS
bytes stay within the budget and the tail's segments cover every window exactly once
(tests/csrc/group_bucket_check.cpp).  The same stand-alone program runs a second time built with the
address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "group_bucket_check.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(exe, extra):
    return subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *extra, "-I",
                           os.path.join(ROOT, "hbbft_amd", "csrc"), "-o", exe, SRC], capture_output=True, text=True)


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"group_bucket: 0 bad of (\d+)", out.stdout)
    assert m and int(m.group(1)) > 10 ** 6, out.stdout
    return out.stdout


def test_group_bucket_layout(tmp_path):
    exe = str(tmp_path / "group_bucket_check")
    b = _build(exe, [])
    assert b.returncode == 0, b.stderr
    out = _run(exe)
    assert "GB_WINDOWS 64 32\n" in out  # two-bit windows over 128 bits (G1) and over d0, d1 < 2^64 (G2)
    m = re.search(r"GB_LDS (\d+) (\d+) budget (\d+)", out)
    assert m and max(int(m.group(1)), int(m.group(2))) <= int(m.group(3)) <= 64 * 1024


def test_group_bucket_layout_sanitized(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    p = subprocess.run(["g++", *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime for g++")
    exe = str(tmp_path / "group_bucket_check_san")
    b = _build(exe, san)
    assert b.returncode == 0, b.stderr
    _run(exe)
