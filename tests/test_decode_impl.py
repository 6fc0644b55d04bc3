"""The decoder-form switch (hbh_engine_set_decode_impl) without a GPU: header macros against the
Python constants, the bound symbol, and the op model's premise -- in the throughput form the
subgroup role is the longer chain, in the latency form the root role is."""
import os
import re

from hbbft_amd import _lib
from hbbft_amd import workcount as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hbbft_hip.h")


def header_macros():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {k: int(v, 0) for k, v in re.findall(r"^#define\s+(HBH_[A-Z0-9_]+)\s+(-?\w+)\s*$", text, flags=re.M)}


def test_header_macros_equal_python_constants():
    m = header_macros()
    assert (m["HBH_DEC_AUTO"], m["HBH_DEC_LANE"], m["HBH_DEC_SPLIT"]) == (0, 1, 2)
    assert (_lib.DEC_AUTO, _lib.DEC_LANE, _lib.DEC_SPLIT) == (m["HBH_DEC_AUTO"], m["HBH_DEC_LANE"], m["HBH_DEC_SPLIT"])
    assert _lib.AUTO_DEC_G1_SPLIT_MAX == m["HBH_AUTO_DEC_G1_SPLIT_MAX"]
    assert _lib.AUTO_DEC_G2_SPLIT_MAX == m["HBH_AUTO_DEC_G2_SPLIT_MAX"]
    assert _lib.AUTO_DEC_G1_SPLIT_MAX >= 0 and _lib.AUTO_DEC_G2_SPLIT_MAX >= 0


def test_symbol_is_bound():
    sig = [s for s in _lib.SIGNATURES if s[0] == "hbh_engine_set_decode_impl"]
    assert len(sig) == 1
    assert len(sig[0][2]) == 2   # (engine, impl)
    from hbbft_amd.engine import Engine
    assert callable(Engine.set_decode_impl)


def test_workcount_split_subgroup_role_is_shorter_than_root():
    for g in ("g1", "g2"):
        roles = W.WIRE_DECODE_ROLES[(g, "split")]
        assert roles["subgroup"] < roles["root"], (g, roles)
        assert W.wire_decode_critical_path(g, "split") == roles["root"]
        assert W.WIRE_DECODE_PRODUCTS[(g, "split")] > W.WIRE_DECODE_PRODUCTS[(g, "lane")]   # latency costs work


def test_workcount_lane_subgroup_role_is_longer_than_root():
    for g in ("g1", "g2"):
        roles = W.WIRE_DECODE_ROLES[(g, "lane")]
        assert roles["subgroup"] > roles["root"], (g, roles)
        assert 0 < W.wire_split_model_ratio(g) < 1
