"""The Q form of the device hash (hbbft_amd/csrc/k_hash.hip k_hash_clear_bp through
Engine.hash_g1_g2_bp = hbh_engine_hash_g1_g2_bp) against the host stage's hbh_hash_g1_g2_bp, byte for byte.
Every test forces the DEVICE form and checks that a hash stage ran.

U is fixed and V = b"hbh-trial-%d", so the hashed messages V || compress(U) differ only in V and need
between 1 and 10 candidate x (counted here on the message actually hashed)."""
import random

import pytest

from hbbft_amd import _lib, hoststage
from hbbft_amd.sync_key_gen import G1_GEN
from oracle import bls12_381 as C
from oracle import tc

pytestmark = pytest.mark.gpu

NTRIAL = 200
# KCOF = h2 s^-1 mod r, s = (z^2 - z - 1) + (z - 1) p + 2 p^2 mod r (tools/gen_constants.py)
_Z, _LAM = -C.X_ABS, C.P % C.R
KCOF = C.H2 * pow(((_Z * _Z - _Z - 1) + (_Z - 1) * _LAM + 2 * _LAM * _LAM) % C.R, -1, C.R) % C.R


def candidates(msg):
    """how many x G2::rand draws for msg before x^3 + b is a square (a in Fq2 is a square iff its norm is
    a square in Fq): tests/test_gpu_hash_g2.py's count"""
    rng = tc.ChaChaRng(tc.sha3_256(msg))
    k = 0
    while True:
        k += 1
        x = (rng.gen_fq(), rng.gen_fq())
        rng.gen_bool()
        a = C.f2_add(C.f2_mul(C.f2_sqr(x), x), C.B2)
        nrm = (a[0] * a[0] + a[1] * a[1]) % C.P
        if nrm == 0 or pow(nrm, (C.P - 1) // 2, C.P) == 1:
            return k


@pytest.fixture(scope="module")
def trials():
    """(U, Vs, host-stage Q_bp, host-stage hash_g1_g2, candidate counts) of the 200 trial ciphertext
    heads, computed once"""
    u = hoststage.g1_mul([G1_GEN], [0x1234567])[0]
    vs = [b"hbh-trial-%d" % i for i in range(NTRIAL)]
    cu = hoststage.g1_compress([u])[0]
    cand = [candidates(v + cu) for v in vs]  # |V| <= 64: hash_g1_g2 hashes V || compress(U)
    return u, vs, hoststage.hash_g1_g2_bp([u] * NTRIAL, vs), hoststage.hash_g1_g2([u] * NTRIAL, vs), cand


@pytest.fixture
def dev(engine):
    engine.set_hash_impl(_lib.HASH_DEVICE)
    engine.set_profiling(True)
    yield engine
    engine.set_profiling(False)
    engine.dbg_set_hash_rounds(0)
    engine.set_hash_impl(_lib.HASH_AUTO)


def ran_on_device(engine):
    return engine.stage_time(_lib.STAGE_HASH)[1]


@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_batch_sizes(dev, trials, n):
    """65: two workgroups, one of them partial; 200: the spread of candidate counts"""
    u, vs, want, _, cand = trials
    assert max(cand) >= 6  # the inputs cannot silently become easy
    assert dev.hash_g1_g2_bp([u] * n, vs[:n]) == want[:n]
    assert ran_on_device(dev) == 1


def test_message_lengths(dev):
    """|V| <= 64 is hashed as it is, longer V through sha3 first"""
    rng = random.Random(151)
    us = hoststage.g1_mul([G1_GEN] * 4, [rng.randrange(1, C.R) for _ in range(4)])
    vs = [bytes(rng.randrange(256) for _ in range(n)) for n in (0, 64, 65, 200)]
    got = dev.hash_g1_g2_bp(us, vs)
    assert ran_on_device(dev) == 1
    assert got == hoststage.hash_g1_g2_bp(us, vs)


def test_round_cap_leftovers_take_the_host_path(dev, trials):
    u, vs, want, _, cand = trials
    dev.dbg_set_hash_rounds(2)
    assert sum(1 for c in cand if c > 2) > 20
    assert dev.hash_g1_g2_bp([u] * NTRIAL, vs) == want
    assert ran_on_device(dev) == 1


def test_kcof_multiple_is_hash_g1_g2(dev, trials):
    u, vs, _, full, _ = trials
    q = dev.hash_g1_g2_bp([u] * 8, vs[:8])
    assert ran_on_device(dev) == 1
    assert hoststage.g2_mul(q, [KCOF] * 8) == full[:8]


def test_full_form_beside_the_q_form(dev, trials):
    """both instantiations share the engine's work buffers: neither disturbs the other"""
    u, vs, want, full, _ = trials
    assert dev.hash_g1_g2_bp([u] * NTRIAL, vs) == want
    assert dev.hash_g1_g2([u] * NTRIAL, vs) == full
    assert dev.hash_g1_g2_bp([u] * 65, vs[:65]) == want[:65]
    assert dev.hash_g1_g2([u] * 65, vs[:65]) == full[:65]
    assert ran_on_device(dev) == 4


def test_host_form_and_arguments(engine, trials):
    u, vs, want, _, _ = trials
    engine.set_hash_impl(_lib.HASH_HOST)
    engine.set_profiling(True)
    try:
        assert engine.hash_g1_g2_bp([u] * 65, vs[:65]) == want[:65]
        assert ran_on_device(engine) == 0
        assert engine.hash_g1_g2_bp([], []) == []
        with pytest.raises(ValueError):
            engine.hash_g1_g2_bp([u], [])
    finally:
        engine.set_profiling(False)
        engine.set_hash_impl(_lib.HASH_AUTO)
