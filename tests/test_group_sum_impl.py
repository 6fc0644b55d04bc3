"""The group-sum form switch (hbh_engine_set_group_sum_impl) without a GPU: header macros against the
Python constants, the bound symbol, and the op model's two premises -- at a tile of 64 items the bucket
form issues less than half the chain form's products, and at a tile of 2 items it issues more (its
reduction and tail are paid per tile, whatever the tile holds): the crossover a threshold is for."""
import os
import re

import pytest

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
    assert (m["HBH_GSUM_AUTO"], m["HBH_GSUM_CHAIN"], m["HBH_GSUM_BUCKET"]) == (0, 1, 2)
    assert (_lib.GSUM_AUTO, _lib.GSUM_CHAIN, _lib.GSUM_BUCKET) == (0, 1, 2)
    assert _lib.AUTO_GSUM_G1_BUCKET_MIN == m["HBH_AUTO_GSUM_G1_BUCKET_MIN"]
    assert _lib.AUTO_GSUM_G2_BUCKET_MIN == m["HBH_AUTO_GSUM_G2_BUCKET_MIN"]
    assert _lib.AUTO_GSUM_G1_BUCKET_MIN >= 0 and _lib.AUTO_GSUM_G2_BUCKET_MIN >= 0


def test_symbol_is_bound():
    sig = [s for s in _lib.SIGNATURES if s[0] == "hbh_engine_set_group_sum_impl"]
    assert len(sig) == 1
    assert len(sig[0][2]) == 2   # (engine, impl)
    from hbbft_amd.engine import Engine
    assert callable(Engine.set_group_sum_impl)


@pytest.mark.parametrize("kind", ["g1", "g2"])
def test_workcount_bucket_form_crossover(kind):
    assert W.group_sum_ops(kind, "bucket", 64) * 2 < W.group_sum_ops(kind, "chain", 64)
    assert W.group_sum_ops(kind, "bucket", 2) > W.group_sum_ops(kind, "chain", 2)
    for impl in ("chain", "bucket"):
        assert 0 < W.group_sum_critical_path(kind, impl, 64) <= W.group_sum_critical_path(kind, impl, 128)
    with pytest.raises(ValueError):
        W.group_sum_ops(kind, "other", 64)
