"""HBH_IMPL_WAVEP without a GPU: the header's macros against the Python mirror, the kind's place in
the engine's dispatch, and the build list."""
import os
import re

from hbbft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def header_macros():
    text = re.sub(r"/\*.*?\*/", "", read("include", "hbbft_hip.h"), flags=re.S)
    return {k: int(v, 0) for k, v in re.findall(r"^#define\s+(HBH_[A-Z0-9_]+)\s+(-?\w+)\s*$", text, flags=re.M)}


def test_header_macros_equal_python_constants():
    m = header_macros()
    assert m["HBH_IMPL_WAVEP"] == 10 == _lib.IMPL_WAVEP
    assert (_lib.AUTO_WAVEP_MIN, _lib.AUTO_WAVEP_MAX) == (m["HBH_AUTO_WAVEP_MIN"], m["HBH_AUTO_WAVEP_MAX"])
    impls = {k: v for k, v in m.items() if k.startswith("HBH_IMPL_")}
    assert len(set(impls.values())) == len(impls)  # no two kinds share a value
    assert 9 not in impls.values()                  # 9 stays rejected


def test_auto_range_is_empty_or_inside_the_wave_kernels_sizes():
    lo, hi = _lib.AUTO_WAVEP_MIN, _lib.AUTO_WAVEP_MAX
    assert lo >= 1
    if lo <= hi:  # a shipped range lies where one wave per check is in use at all
        assert hi <= header_macros()["HBH_AUTO_OCT_MAX"]


def test_engine_dispatches_the_kind():
    eng = read("hbbft_amd", "csrc", "engine_pairing.hip")
    assert "hbl::wavep_verify(" in eng
    assert eng.count("HBH_AUTO_WAVEP_MIN") >= 2 and eng.count("HBH_AUTO_WAVEP_MAX") >= 2  # resolve_impl, verify_auto
    assert "impl != HBH_IMPL_WAVEP" in read("hbbft_amd", "csrc", "engine.hip")  # accepted by the setter
    assert "$(BUILD)/k_wavep.o" in read("hbbft_amd", "Makefile")
