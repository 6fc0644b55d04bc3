"""The branch-free inverse of the lane-pair pairing kernel (hbbft_amd/csrc/words.hpp INV_UNIFORM,
compiled with g++) returns the per-divstep form's words: 20,000 seeded random values, 0, 1, 2, m - 1,
m - 2, (m + 1) / 2, every 2^k and 2^k - 1 below m, over the BLS12-381 base and scalar fields, and
y * y^-1 == 1 on the first 200 values.  The same stand-alone program runs a second time built with the
address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "words_inv_uniform_check.cpp")
# 20,000 random + 6 named + the 2^k (381 / 255) + the 2^k - 1 (381 / 255: k = 0 is the value 0 again)
WANT = "p: 0 bad of 20768, r: 0 bad of 20516"

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(exe, extra):
    return subprocess.run(["g++", "-O2", "-std=c++17", *extra, "-I", os.path.join(ROOT, "hbbft_amd", "csrc"),
                           "-o", exe, SRC], capture_output=True, text=True)


def test_uniform_inverse_matches_per_divstep(tmp_path):
    exe = str(tmp_path / "words_inv_uniform_check")
    b = _build(exe, [])
    assert b.returncode == 0, b.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert WANT in out.stdout


def test_uniform_inverse_sanitized(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    p = subprocess.run(["g++", *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime for g++")
    exe = str(tmp_path / "words_inv_uniform_check_san")
    b = _build(exe, san)
    assert b.returncode == 0, b.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert WANT in out.stdout
