"""Host planning of the grouped share checks (hbbft_amd/csrc/group_plan.hpp, compiled with g++): for
shuffled index arrays the groups in CSR form, the permutation (a bijection that brings each group's
items together in call order), the tiles at group sizes 1, 2, GROUP_TILE - 1, GROUP_TILE,
GROUP_TILE + 1 and 2 GROUP_TILE + 5, absent table entries, the singles list and the fallback gather list
of a group-verdict vector (tests/csrc/group_plan_check.cpp).  The same stand-alone program runs a second
time built with the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "group_plan_check.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(exe, extra):
    return subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", *extra, "-I", os.path.join(ROOT, "hbbft_amd", "csrc"),
                           "-o", exe, SRC], capture_output=True, text=True)


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"group_plan: 0 bad of (\d+)", out.stdout)
    assert m and int(m.group(1)) > 10000, out.stdout
    return out.stdout


def test_group_plan(tmp_path):
    exe = str(tmp_path / "group_plan_check")
    b = _build(exe, [])
    assert b.returncode == 0, b.stderr
    out = _run(exe)
    # the constant the Python side exports is the header's
    from hbbft_amd import _lib
    assert "GROUP_TILE %d\n" % _lib.GROUP_TILE in out
    assert _lib.GROUP_TILE >= 2 and _lib.GROUP_TILE & (_lib.GROUP_TILE - 1) == 0  # the LDS tree halves it


def test_group_plan_sanitized(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    p = subprocess.run(["g++", *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime for g++")
    exe = str(tmp_path / "group_plan_check_san")
    b = _build(exe, san)
    assert b.returncode == 0, b.stderr
    _run(exe)
