"""Ciphertext::verify from the ciphertext itself (Engine.verify_ciphertexts_uv = hbh_verify_ciphertexts_uv:
the Q form of the device hash written into the Q2 table of the pairing check) against
verify_ciphertexts_bp over host-stage Q_bp, verify_ciphertexts over host-stage hash_g1_g2, and the oracle's
Ciphertext::verify.  HOST and DEVICE forms forced, DEVICE with the round cap at 2, and AUTO on both sides
of HBH_AUTO_HASH_DEVICE_MIN."""
import random

import pytest

from hbbft_amd import _lib, hoststage
from hbbft_amd.sync_key_gen import G1_GEN, R_ORDER
from oracle import tc

pytestmark = pytest.mark.gpu

LENGTHS = (0, 32, 64, 65, 1096)


def g1_pt(b):
    return None if b == bytes(96) else (int.from_bytes(b[:48], "little"), int.from_bytes(b[48:], "little"))


def g2_pt(b):
    if b == bytes(192):
        return None
    v = [int.from_bytes(b[48 * k:48 * k + 48], "little") for k in range(4)]
    return ((v[0], v[1]), (v[2], v[3]))


@pytest.fixture(scope="module")
def cases():
    """11 valid ciphertexts and 5 tampered copies as (U, V, W) lists, with the verdicts of the oracle's
    Ciphertext::verify, computed once"""
    rng = random.Random(152)
    n = 11
    pks = hoststage.g1_mul([G1_GEN] * 3, [rng.randrange(1, R_ORDER) for _ in range(3)])
    msgs = [bytes(rng.randrange(256) for _ in range(LENGTHS[i % len(LENGTHS)])) for i in range(n)]
    cts = hoststage.encrypt([pks[i % 3] for i in range(n)], msgs, [rng.randrange(1, R_ORDER) for _ in range(n)])
    (u1, v1, w1), (u2, v2, w2), (u4, v4, w4) = cts[1], cts[2], cts[4]
    bad = [(u1, v1[:5] + bytes([v1[5] ^ 1]) + v1[6:], w1),  # a V byte flipped
           (u2, v2, w1),                                      # W of another ciphertext
           (u1, v2, w2),                                      # U of another ciphertext
           (bytes(96), v4, w4),                               # U = O
           (u4, v4, bytes(192))]                              # W = O
    cts = cts + bad
    want = bytes([1] * n + [0] * len(bad))
    oracle = bytes(int(tc.ciphertext_verify((g1_pt(u), v, g2_pt(w)))) for u, v, w in cts)
    assert oracle == want
    return cts, want


def tiled(cts, want, n):
    k = -(-n // len(cts))
    return (cts * k)[:n], (want * k)[:n]


def split(cts):
    return [c[0] for c in cts], [c[1] for c in cts], [c[2] for c in cts]


@pytest.fixture
def eng(engine):
    engine.set_profiling(True)
    yield engine
    engine.set_profiling(False)
    engine.dbg_set_hash_rounds(0)
    engine.set_hash_impl(_lib.HASH_AUTO)


def hash_launches(engine):
    return engine.stage_time(_lib.STAGE_HASH)[1]


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("form", ["host", "device", "device-2-rounds"])
def test_verdicts(eng, cases, form, n):
    cts, want = tiled(*cases, n)
    us, vs, ws = split(cts)
    eng.set_hash_impl(_lib.HASH_HOST)
    ref_bp = eng.verify_ciphertexts_bp(us, ws, hoststage.hash_g1_g2_bp(us, vs))
    ref_full = eng.verify_ciphertexts(us, ws, hoststage.hash_g1_g2(us, vs))
    assert ref_bp == ref_full == want
    if form != "host":
        eng.set_hash_impl(_lib.HASH_DEVICE)
    if form == "device-2-rounds":
        eng.dbg_set_hash_rounds(2)
    eng.set_profiling(True)  # restarts the stage counts
    got = eng.verify_ciphertexts_uv(us, vs, ws)
    assert hash_launches(eng) == (0 if form == "host" else 1)
    assert got == want


def test_auto_threshold(eng, cases):
    """AUTO: one item below HBH_AUTO_HASH_DEVICE_MIN stays on the host stage, the threshold itself runs on
    the device; 64 distinct ciphertexts (the 16 cases and 48 more valid ones), tiled"""
    m = _lib.AUTO_HASH_DEVICE_MIN
    assert m > 1
    rng = random.Random(153)
    pk = hoststage.g1_mul([G1_GEN], [rng.randrange(1, R_ORDER)])
    more = hoststage.encrypt(pk, [b"auto %d" % i for i in range(48)], [rng.randrange(1, R_ORDER) for _ in range(48)])
    cts, want = tiled(cases[0] + more, cases[1] + bytes([1] * 48), m)
    assert len(set(cts)) == 64
    us, vs, ws = split(cts)
    eng.set_hash_impl(_lib.HASH_AUTO)
    assert eng.verify_ciphertexts_uv(us[:m - 1], vs[:m - 1], ws[:m - 1]) == want[:m - 1]
    assert hash_launches(eng) == 0
    assert eng.verify_ciphertexts_uv(us, vs, ws) == want
    assert hash_launches(eng) == 1


def test_arguments(eng, cases):
    cts, _ = cases
    us, vs, ws = split(cts)
    assert eng.verify_ciphertexts_uv([], [], []) == b""
    with pytest.raises(ValueError):
        eng.verify_ciphertexts_uv(us, vs[:-1], ws)
    with pytest.raises(ValueError):
        eng.verify_ciphertexts_uv(us, vs, ws[:-1])
