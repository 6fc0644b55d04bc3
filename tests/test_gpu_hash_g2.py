"""The device form of hash_g2 / hash_g1_g2 (hbbft_amd/csrc/k_hash.hip through Engine.hash_g2,
hash_g1_g2, hash_g2_dev) against the host stage (csrc/host_hash.cpp), byte for byte, and against the
oracle's textbook G2::rand on a few messages.  Every test forces the DEVICE form except the AUTO one.

The messages b"hbh-trial-%d" (i < 2,000) need between 1 and 12 candidate x before one gives a square
(counted here with the oracle's stream and the Euler criterion on the norm), so the sampler's rounds,
its worklist compaction and the saved stream positions are all exercised; i = 389 needs 12."""
import hashlib
import json
import os
import random

import numpy as np
import pytest
import torch

from hbbft_amd import _lib, hoststage
from hbbft_amd.sync_key_gen import G1_GEN
from oracle import bls12_381 as C
from oracle import tc
from tests.hash_trials import candidates, trial  # noqa: F401 (test_gpu_hash_quad imports them from here)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NTRIAL = 2000


def abi_g2(pt):
    (x0, x1), (y0, y1) = pt
    return b"".join(v.to_bytes(48, "little") for v in (x0, x1, y0, y1))


@pytest.fixture(scope="module")
def trials():
    """(messages, host-stage hashes, candidate counts) of the 2,000 trial messages, computed once"""
    msgs = [trial(i) for i in range(NTRIAL)]
    return msgs, hoststage.hash_g2(msgs), [candidates(m) for m in msgs]


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


def test_golden_documents(dev):
    with open(os.path.join(GOLDEN, "threshold_sign_n10_t3.json")) as f:
        d = json.load(f)
    docs = [bytes.fromhex(doc["doc"]) for doc in d["docs"]]
    got = dev.hash_g2(docs)
    assert ran_on_device(dev) == 1
    for g, rec in zip(got, d["docs"]):
        assert hoststage.g2_compress([g])[0] == bytes.fromhex(rec["hash_compressed"])
    assert got == hoststage.hash_g2(docs)


def test_message_lengths(dev):
    """SHA3's rate is 136 bytes: lengths around one and two blocks, empty and long; the oracle's G2::rand
    (Fq2 exponentiation root, double-and-add by the 636-bit h2) is the independent check."""
    rng = random.Random(14)
    msgs = [bytes(rng.randrange(256) for _ in range(n)) for n in (0, 1, 135, 136, 137, 271, 272, 1000)]
    got = dev.hash_g2(msgs)
    assert ran_on_device(dev) == 1
    assert got == hoststage.hash_g2(msgs)
    assert got == [abi_g2(tc.hash_g2(m)) for m in msgs]


def test_many_candidates(dev, trials):
    msgs, want, cand = trials
    hist = {}
    for c in cand:
        hist[c] = hist.get(c, 0) + 1
    assert hist == {1: 1028, 2: 493, 3: 229, 4: 137, 5: 56, 6: 23, 7: 17, 8: 10, 9: 5, 10: 1, 12: 1}
    assert max(cand) >= 10 and cand[389] == 12  # the inputs cannot silently become easy
    assert [i for i, c in enumerate(cand) if c >= 8] == [78, 162, 310, 389, 419, 534, 541, 593, 649, 928, 988, 1100,
                                                         1502, 1539, 1614, 1772, 1930]
    got = dev.hash_g2(msgs)
    assert ran_on_device(dev) == 1
    bad = [i for i in range(NTRIAL) if got[i] != want[i]]
    assert not bad, (bad[:10], [cand[i] for i in bad[:10]])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(dev, trials, n):
    msgs, want, _ = trials
    assert dev.hash_g2(msgs[300:300 + n]) == want[300:300 + n]  # 310 (8 candidates) is in every batch but n = 1
    assert ran_on_device(dev) == 1


def test_every_lane_on_the_long_path(dev, trials):
    msgs, want, cand = trials
    assert dev.hash_g2([msgs[389]] * 64) == [want[389]] * 64
    easy = [i for i in range(NTRIAL) if cand[i] == 1][:63]
    idx = easy[:20] + [389] + easy[20:]
    assert dev.hash_g2([msgs[i] for i in idx]) == [want[i] for i in idx]
    assert ran_on_device(dev) == 2


def test_round_cap_leftovers_take_the_host_path(dev, trials):
    msgs, want, cand = trials
    n = 200
    dev.dbg_set_hash_rounds(2)
    assert sum(1 for c in cand[:n] if c > 2) > 20
    assert dev.hash_g2(msgs[:n]) == want[:n]
    # the device-pointer call cannot fall back: it reports those messages with the all-zero point
    seeds = b"".join(hashlib.sha3_256(m).digest() for m in msgs[:n])
    d_seeds = torch.from_numpy(np.frombuffer(seeds, dtype=np.uint8).copy()).to("cuda:0")
    d_out = torch.full((n * 192,), 0xEE, dtype=torch.uint8, device="cuda:0")
    dev.hash_g2_dev(None, n, d_seeds.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy().tobytes()
    for i in range(n):
        assert raw[i * 192:(i + 1) * 192] == (want[i] if cand[i] <= 2 else bytes(192)), (i, cand[i])
    with pytest.raises(_lib.HbhError):
        dev.dbg_set_hash_rounds(-1)


def test_hash_g1_g2(dev):
    """|V| <= 64 is hashed as it is, longer V through sha3 first."""
    rng = random.Random(15)
    us = hoststage.g1_mul([G1_GEN] * 4, [rng.randrange(1, C.R) for _ in range(4)])
    vs = [bytes(rng.randrange(256) for _ in range(n)) for n in (0, 64, 65, 200)]
    got = dev.hash_g1_g2(us, vs)
    assert ran_on_device(dev) == 1
    assert got == hoststage.hash_g1_g2(us, vs)


def test_hash_g2_dev_feeds_the_pairing_check_on_a_caller_stream(dev, trials):
    """hash_g2_dev on a non-default stream, its HBM output the Q1 table (identity map) of
    verify_pairing_eq_dev on the same stream: PublicKey::verify without the hashes leaving HBM."""
    msgs, want, _ = trials
    n = 8
    rng = random.Random(16)
    sks = [rng.randrange(1, C.R) for _ in range(n)]
    pks = hoststage.g1_mul([G1_GEN] * n, sks)
    sigs = hoststage.g2_mul(want[:n], sks)
    sigs[2] = hoststage.g2_mul([want[3]], [sks[2]])[0]  # a signature over another message
    pks[5] = pks[6]                                      # another signer's key
    ref = dev.verify_signatures(pks, sigs, want[:n])
    assert list(ref) == [1, 1, 0, 1, 1, 0, 1, 1]

    def up(b):
        return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to("cuda:0")

    d_seeds = up(b"".join(hashlib.sha3_256(m).digest() for m in msgs[:n]))
    d_pks, d_sigs = up(b"".join(pks)), up(b"".join(sigs))
    d_h = torch.zeros(n * 192, dtype=torch.uint8, device="cuda:0")
    d_v = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    dev.hash_g2_dev(st.cuda_stream, n, d_seeds.data_ptr(), d_h.data_ptr())
    dev.verify_pairing_eq_dev(st.cuda_stream, n, d_pks.data_ptr(), d_h.data_ptr(), n, None,
                              None, d_sigs.data_ptr(), n, None, d_v.data_ptr())
    st.synchronize()
    assert d_h.cpu().numpy().tobytes() == b"".join(want[:n])
    assert bytes(d_v.cpu().tolist()) == ref


def test_auto(engine, trials):
    """AUTO sends a small call to the host stage and a large one wherever the measured threshold says:
    the bytes are the host stage's either way."""
    msgs, want, _ = trials
    engine.set_hash_impl(_lib.HASH_AUTO)
    engine.set_profiling(True)
    try:
        assert engine.hash_g2(msgs[:4]) == want[:4]
        assert engine.stage_time(_lib.STAGE_HASH)[1] == 0  # below every threshold: no kernel ran
        assert engine.hash_g2(msgs) == want
        on_device = _lib.AUTO_HASH_DEVICE_MIN != 0 and NTRIAL >= _lib.AUTO_HASH_DEVICE_MIN
        assert engine.stage_time(_lib.STAGE_HASH)[1] == (1 if on_device else 0)
    finally:
        engine.set_profiling(False)
    with pytest.raises(_lib.HbhError):
        engine.set_hash_impl(3)
