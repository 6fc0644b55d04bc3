"""The lane-quad form of the device hash (hbbft_amd/csrc/k_hash_quad.hip, Engine.set_hash_form(HFORM_QUAD))
against the host stage (csrc/host_hash.cpp), byte for byte, against the lane form under the same round
cap, and against the oracle's textbook G2::rand on a few messages.  Every test forces DEVICE and QUAD.

The messages are the b"hbh-trial-%d" of tests/test_gpu_hash_g2.py, whose candidate counts 1..12 are pinned
there.  The quad sampler tries four candidates per launch, so a message with c candidates is won by lane
(c - 1) % 4 of launch (c - 1) // 4 + 1: the counts put winners on every lane of launches 1 and 2, and
message 389 (12 candidates) on lane 3 of launch 3."""
import hashlib
import random

import numpy as np
import pytest
import torch

from hbbft_amd import _lib, hoststage
from hbbft_amd.sync_key_gen import G1_GEN, R_ORDER
from oracle import bls12_381 as C
from oracle import tc
from tests.test_gpu_hash_g2 import NTRIAL, abi_g2, candidates, trial

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trials():
    """(messages, host-stage hashes, candidate counts) of the 2,000 trial messages, computed once"""
    msgs = [trial(i) for i in range(NTRIAL)]
    return msgs, hoststage.hash_g2(msgs), [candidates(m) for m in msgs]


@pytest.fixture
def quad(engine):
    engine.set_hash_impl(_lib.HASH_DEVICE)
    engine.set_hash_form(_lib.HFORM_QUAD)
    engine.set_profiling(True)
    yield engine
    engine.set_profiling(False)
    engine.dbg_set_hash_rounds(0)
    engine.set_hash_form(_lib.HFORM_AUTO)
    engine.set_hash_impl(_lib.HASH_AUTO)


def hash_stages(engine):
    return engine.stage_time(_lib.STAGE_HASH)[1]


def test_all_trials_and_every_quad_lane(quad, trials):
    msgs, want, cand = trials
    cells = {}
    for i, c in enumerate(cand):
        cells.setdefault(((c - 1) // 4 + 1, (c - 1) % 4), []).append(i)
    for launch in (1, 2):  # the inputs cannot silently become easy
        for lane in range(4):
            assert cells.get((launch, lane)), (launch, lane)
    assert cand[389] == 12 and 389 in cells[(3, 3)]
    got = quad.hash_g2(msgs)
    assert hash_stages(quad) == 1
    bad = [i for i in range(NTRIAL) if got[i] != want[i]]
    assert not bad, (bad[:10], [cand[i] for i in bad[:10]])


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257])
def test_batch_shapes(quad, trials, n):
    """a workgroup is 16 quads: one live quad, both sides of a full workgroup, of four, and a partial last one"""
    msgs, want, _ = trials
    assert quad.hash_g2(msgs[300:300 + n]) == want[300:300 + n]  # 310 (8 candidates) is in every batch from 15
    assert hash_stages(quad) == 1


def test_long_paths(quad, trials):
    msgs, want, cand = trials
    assert quad.hash_g2([msgs[389]] * 64) == [want[389]] * 64
    easy = [i for i in range(NTRIAL) if cand[i] == 1][:63]
    idx = easy[:20] + [389] + easy[20:]
    assert quad.hash_g2([msgs[i] for i in idx]) == [want[i] for i in idx]
    assert hash_stages(quad) == 2


def hash_dev_bytes(engine, msgs):
    n = len(msgs)
    seeds = b"".join(hashlib.sha3_256(m).digest() for m in msgs)
    d_seeds = torch.from_numpy(np.frombuffer(seeds, dtype=np.uint8).copy()).to("cuda:0")
    d_out = torch.full((n * 192,), 0xEE, dtype=torch.uint8, device="cuda:0")
    engine.hash_g2_dev(None, n, d_seeds.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy().tobytes()


@pytest.mark.parametrize("cap", [2, 5])
def test_round_cap_is_a_cap_on_candidates(quad, trials, cap):
    """cap 2: one masked launch; cap 5: a full launch and one with a single live lane per quad"""
    msgs, want, cand = trials
    n = 200
    quad.dbg_set_hash_rounds(cap)
    assert sum(1 for c in cand[:n] if c > cap) > 5 and sum(1 for c in cand[:n] if c == cap) > 0
    assert quad.hash_g2(msgs[:n]) == want[:n]  # the host-pointer call hashes the leftovers itself
    raw = hash_dev_bytes(quad, msgs[:n])
    assert hash_stages(quad) == 2
    for i in range(n):
        assert raw[i * 192:(i + 1) * 192] == (want[i] if cand[i] <= cap else bytes(192)), (i, cand[i])
    quad.set_hash_form(_lib.HFORM_LANE)
    assert hash_dev_bytes(quad, msgs[:n]) == raw
    assert quad.hash_g2(msgs[:n]) == want[:n]


def test_message_lengths(quad):
    """SHA3's rate is 136 bytes: lengths around one and two blocks, empty and long; the oracle's G2::rand
    is the independent check"""
    rng = random.Random(14)
    msgs = [bytes(rng.randrange(256) for _ in range(n)) for n in (0, 1, 135, 136, 137, 271, 272, 1000)]
    got = quad.hash_g2(msgs)
    assert hash_stages(quad) == 1
    assert got == hoststage.hash_g2(msgs)
    assert got == [abi_g2(tc.hash_g2(m)) for m in msgs]


def test_hash_g1_g2(quad):
    rng = random.Random(15)
    us = hoststage.g1_mul([G1_GEN] * 4, [rng.randrange(1, C.R) for _ in range(4)])
    vs = [bytes(rng.randrange(256) for _ in range(n)) for n in (0, 64, 65, 200)]
    got = quad.hash_g1_g2(us, vs)
    assert hash_stages(quad) == 1
    assert got == hoststage.hash_g1_g2(us, vs)


@pytest.fixture(scope="module")
def heads():
    """(U, Vs, host-stage Q_bp) of 200 ciphertext heads, tests/test_gpu_hash_bp.py's"""
    u = hoststage.g1_mul([G1_GEN], [0x1234567])[0]
    vs = [trial(i) for i in range(200)]
    return u, vs, hoststage.hash_g1_g2_bp([u] * 200, vs)


@pytest.mark.parametrize("cap", [0, 2])
@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_q_form(quad, heads, n, cap):
    u, vs, want = heads
    quad.dbg_set_hash_rounds(cap)  # 0: the default
    assert quad.hash_g1_g2_bp([u] * n, vs[:n]) == want[:n]
    assert hash_stages(quad) == 1


def test_verify_signed_verdicts(quad):
    rng = random.Random(241)
    n, nkeys = 40, 5
    sks = [rng.randrange(1, R_ORDER) for _ in range(nkeys)]
    keys = hoststage.g1_mul([G1_GEN] * nkeys, sks)
    msgs = [b"quad signed message %d" % i for i in range(n)]
    hs = hoststage.hash_g2(msgs)
    signer = [i % nkeys for i in range(n)]
    sigs = hoststage.g2_mul(hs, [sks[j] for j in signer])
    pks = [keys[j] for j in signer]
    sigs[3] = hoststage.g2_mul([hs[4]], [sks[signer[3]]])[0]  # forged: a signature over another message
    pks[17] = keys[(signer[17] + 1) % nkeys]                   # another signer's key
    want = bytes(0 if i in (3, 17) else 1 for i in range(n))
    got = quad.verify_signed(pks, sigs, msgs)
    assert hash_stages(quad) == 1
    assert got == want
    quad.set_hash_form(_lib.HFORM_LANE)
    assert quad.verify_signed(pks, sigs, msgs) == got
    assert hash_stages(quad) == 2
    quad.set_hash_impl(_lib.HASH_HOST)
    quad.set_hash_form(_lib.HFORM_QUAD)  # no effect on a call that takes the host stage
    assert quad.verify_signed(pks, sigs, msgs) == got
    assert hash_stages(quad) == 2


def test_verify_ciphertexts_uv_verdicts(quad):
    rng = random.Random(242)
    n = 35
    pks = hoststage.g1_mul([G1_GEN] * 3, [rng.randrange(1, R_ORDER) for _ in range(3)])
    msgs = [bytes(rng.randrange(256) for _ in range((0, 32, 64, 65, 300)[i % 5])) for i in range(n)]
    cts = hoststage.encrypt([pks[i % 3] for i in range(n)], msgs, [rng.randrange(1, R_ORDER) for _ in range(n)])
    (u1, v1, w1), (u2, v2, w2), (u4, v4, w4) = cts[1], cts[2], cts[4]
    bad = [(u1, v1[:5] + bytes([v1[5] ^ 1]) + v1[6:], w1),  # a V byte flipped
           (u2, v2, w1),                                      # W of another ciphertext
           (u1, v2, w2),                                      # U of another ciphertext
           (bytes(96), v4, w4),                               # U = O
           (u4, v4, bytes(192))]                              # W = O
    cts = cts + bad
    want = bytes([1] * n + [0] * len(bad))
    us, vs, ws = [c[0] for c in cts], [c[1] for c in cts], [c[2] for c in cts]
    got = quad.verify_ciphertexts_uv(us, vs, ws)
    assert hash_stages(quad) == 1
    assert got == want
    quad.set_hash_form(_lib.HFORM_LANE)
    assert quad.verify_ciphertexts_uv(us, vs, ws) == got
    assert hash_stages(quad) == 2
    quad.set_hash_impl(_lib.HASH_HOST)
    assert quad.verify_ciphertexts_uv(us, vs, ws) == got
    assert hash_stages(quad) == 2


def test_setter(quad, trials):
    msgs, want, _ = trials
    for bad in (3, -1, 17):
        with pytest.raises(_lib.HbhError):
            quad.set_hash_form(bad)
    # a refused value changes nothing: the engine goes on hashing (the two forms write the same bytes by
    # contract, so which one ran is not visible from outside)
    assert (_lib.HFORM_AUTO, _lib.HFORM_LANE, _lib.HFORM_QUAD) == (0, 1, 2)
    assert quad.hash_g2(msgs[:20]) == want[:20]
    assert hash_stages(quad) == 1
    quad.set_hash_form(_lib.HFORM_LANE)
    quad.set_hash_form(_lib.HFORM_AUTO)
    assert quad.hash_g2(msgs[:20]) == want[:20]
    assert hash_stages(quad) == 2
