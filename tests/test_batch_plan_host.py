"""Host planning of the batched independent checks (hbbft_amd/csrc/batch_plan.hpp, compiled with g++):
the groups of BATCH_GROUP consecutive items, the single last item, the tiles of the G2 sums and of the
Miller-product launch at the three lane widths, and the fallback lists, at n = 0, 1, 2, 3, the tile and
group bounds (63 .. 65, 127 .. 129, 255 .. 258, 511 .. 513), 1,024 and 10,100
(tests/csrc/batch_plan_check.cpp).  The same stand-alone program runs a second time built with the address
and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "batch_plan_check.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(exe, extra):
    return subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", *extra, "-I", os.path.join(ROOT, "hbbft_amd", "csrc"),
                           "-o", exe, SRC], capture_output=True, text=True)


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"batch_plan: 0 bad of (\d+)", out.stdout)
    assert m and int(m.group(1)) > 10000, out.stdout
    return out.stdout


def test_batch_plan(tmp_path):
    exe = str(tmp_path / "batch_plan_check")
    b = _build(exe, [])
    assert b.returncode == 0, b.stderr
    out = _run(exe)
    from hbbft_amd import _lib
    assert "BATCH_GROUP %d\n" % _lib.BATCH_GROUP in out  # the constant the Python side exports is the header's
    with open(os.path.join(ROOT, "include", "hbbft_hip.h")) as f:
        assert "#define HBH_BATCH_GROUP %d\n" % _lib.BATCH_GROUP in f.read()


def test_batch_plan_sanitized(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    p = subprocess.run(["g++", *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime for g++")
    exe = str(tmp_path / "batch_plan_check_san")
    b = _build(exe, san)
    assert b.returncode == 0, b.stderr
    _run(exe)
