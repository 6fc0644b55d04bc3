"""PublicKey::verify from the messages themselves (Engine.verify_signed = hbh_verify_signatures: hash_g2
on the device, the hashes the Q1 table of the pairing check without leaving HBM) against
Engine.verify_signatures over host-stage hashes and the C oracle, and the DynamicHoneyBadger batch
paths that use it (DhbKeyGen, VoteCounter with device_hash=True) against their defaults.  The hash form
is forced to DEVICE throughout."""
import random

import pytest

from hbbft_amd import _lib, hoststage
from hbbft_amd.dynamic_honey_badger import (DhbKeyGen, SignedKeyGenMsg, SignedVote, Vote, VoteCounter,
                                            encryption_schedule, node_change, vote_bytes)
from hbbft_amd.sync_key_gen import G1_GEN, G2_GEN, R_ORDER, SyncKeyGen
from oracle import cbls
from tests.hash_trials import candidates, trial

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev(engine):
    engine.set_hash_impl(_lib.HASH_DEVICE)
    engine.set_profiling(True)
    yield engine
    engine.set_profiling(False)
    engine.dbg_set_hash_rounds(0)
    engine.set_hash_impl(_lib.HASH_AUTO)


def hash_launches(engine):
    return engine.stage_time(_lib.STAGE_HASH)[1]


def test_verify_signed_matches_host_hashed_verdicts(dev):
    rng = random.Random(158)
    n, nkeys = 200, 7
    sks = [rng.randrange(1, R_ORDER) for _ in range(nkeys)]
    keys = hoststage.g1_mul([G1_GEN] * nkeys, sks)
    msgs = [b"" if i == 9 else b"signed message %d" % i for i in range(n)]
    hs = hoststage.hash_g2(msgs)
    signer = [i % nkeys for i in range(n)]
    sigs = hoststage.g2_mul(hs, [sks[j] for j in signer])
    pks = [keys[j] for j in signer]
    want_valid = []
    for i in range(n):
        kind = i % 11
        if kind == 3:    # a signature over another message
            sigs[i] = hoststage.g2_mul([hs[(i + 1) % n]], [sks[signer[i]]])[0]
        elif kind == 5:  # another signer's key
            pks[i] = keys[(signer[i] + 1) % nkeys]
        elif kind == 7:  # a signature at infinity
            sigs[i] = bytes(192)
        want_valid.append(kind not in (3, 5, 7))
    assert want_valid[9]  # the empty message is a valid item
    got = dev.verify_signed(pks, sigs, msgs)
    assert hash_launches(dev) == 1
    assert got == dev.verify_signatures(pks, sigs, hs)
    assert list(got) == [int(w) for w in want_valid]
    for i in range(0, n, 10):  # 20 samples against the C oracle's PublicKey::verify
        assert got[i] == int(cbls.verify_g2(pks[i], sigs[i], hs[i])), i
    # the host form of the same call
    dev.set_hash_impl(_lib.HASH_HOST)
    dev.set_profiling(True)
    assert dev.verify_signed(pks, sigs, msgs) == got
    assert hash_launches(dev) == 0
    assert dev.verify_signed([], [], []) == b""


def test_round_cap_leftovers_are_patched_into_the_hash_table(dev):
    """With the sampler capped at two rounds the device leaves every message of more than two candidates
    to the host stage, whose hashes are patched into the Q1 table in HBM before the pairing check reads
    it.  An unpatched entry is the all-zero point: a valid signature's verdict would turn to 0."""
    rng = random.Random(159)
    n, nkeys = 65, 5  # one full wave plus one item
    msgs = [trial(i) for i in range(300, 300 + n)]
    cand = [candidates(m) for m in msgs]
    left = [i for i, c in enumerate(cand) if c > 2]
    assert len(left) >= 5 and n - len(left) >= 5
    assert 10 in left and 0 not in left  # the two corrupted positions: one patched, one resolved
    sks = [rng.randrange(1, R_ORDER) for _ in range(nkeys)]
    keys = hoststage.g1_mul([G1_GEN] * nkeys, sks)
    hs = hoststage.hash_g2(msgs)
    signer = [i % nkeys for i in range(n)]
    sigs = hoststage.g2_mul(hs, [sks[j] for j in signer])
    pks = [keys[j] for j in signer]
    for i in (0, 10):  # a signature over another message
        sigs[i] = hoststage.g2_mul([hs[i + 1]], [sks[signer[i]]])[0]
    dev.dbg_set_hash_rounds(2)
    got = dev.verify_signed(pks, sigs, msgs)
    assert hash_launches(dev) == 1
    dev.set_hash_impl(_lib.HASH_HOST)
    dev.set_profiling(True)
    assert got == dev.verify_signed(pks, sigs, msgs)
    assert hash_launches(dev) == 0
    assert list(got) == [0 if i in (0, 10) else 1 for i in range(n)]


def key_gen_run(engine, device_hash):
    """tests/test_gpu_dhb_key_gen.py's scenario: four nodes sign their Parts and Acks, proposer 1 commits
    a forged signature and proposer 2 a wrong-era copy.  Returns everything the batch paths decide."""
    rng = random.Random(77)
    n, t, era = 4, 1, 7
    sks = [rng.randrange(1, R_ORDER) for _ in range(n)]
    pub = dict(enumerate(hoststage.g1_mul([G1_GEN] * n, sks)))
    current = {i: pub[i] for i in range(n - 1)}  # node 3 is a joining candidate: no current key
    dhbs, parts = [], []
    for i in range(n):
        kg, part = SyncKeyGen.new(i, sks[i], pub, t, engine, rng=rng)
        dhbs.append(DhbKeyGen(engine, era, i, sks[i], current, key_gen=kg, candidate_keys=pub, device_hash=device_hash))
        parts.append(part)
    for i in range(n):
        dhbs[i].send_transaction(parts[i])
    contributions = [(i, list(dhbs[i].key_gen_msg_buffer)) for i in range(n)]
    forged = SignedKeyGenMsg(era, 0, parts[0], hoststage.g2_mul([G2_GEN], [12345])[0])
    stale = SignedKeyGenMsg(era - 1, 2, parts[2], contributions[2][1][0].sig)
    contributions[1] = (1, contributions[1][1] + [forged])
    contributions[2] = (2, [stale] + contributions[2][1])
    log = []
    for d in dhbs:
        step = d.handle_committed(contributions, rng)
        log.append(([(f.node_id, f.kind) for f in step.fault_log], len(step.messages), d.calls, d.checks))
    contributions = [(i, list(dhbs[i].key_gen_msg_buffer)) for i in range(n)]
    for d in dhbs:
        step = d.handle_committed(contributions, rng)
        log.append(([(f.node_id, f.kind) for f in step.fault_log], d.key_gen.is_ready(), d.calls, d.checks))
    log.append([d.key_gen.generate()[0] for d in dhbs])
    return log


def test_dhb_key_gen_device_hash(dev):
    want = key_gen_run(dev, False)
    assert hash_launches(dev) == 0
    got = key_gen_run(dev, True)
    assert hash_launches(dev) == sum(entry[2] for entry in got[4:8]) == 8  # every engine call of the batches hashed on the device
    assert got == want
    assert want[0][0] == [(1, "InvalidKeyGenMessageSignature"), (2, "InvalidKeyGenMessageEra")]


def committed_batch_run(engine, device_hash):
    """tests/test_dhb_votes.py's random committed batch: 16 voters, forged signatures, wrong eras, stale and
    repeated numbers, an unknown voter, five proposers."""
    n, era = 16, 9
    rng = random.Random(11)
    sks = [rng.randrange(1, R_ORDER) for _ in range(n)]
    pks = dict(enumerate(hoststage.g1_mul([G1_GEN] * n, sks)))
    ct = VoteCounter(engine, era, 0, sks[0], pks, (n - 1) // 3, device_hash=device_hash)
    rng = random.Random(12)
    changes = [node_change({j: pks[j]}) for j in range(3)] + [encryption_schedule("EveryNthEpoch", 4)]
    votes = []
    for voter in range(n):
        for num in range(rng.randrange(1, 4)):
            votes.append((voter, Vote(rng.choice(changes), era if rng.random() > 0.1 else era - 1, num)))
    hs = hoststage.hash_g2(vote_bytes([v for _, v in votes]))
    sigs = hoststage.g2_mul(hs, [sks[voter] for voter, _ in votes])
    svs = [SignedVote(v, voter, s) for (voter, v), s in zip(votes, sigs)]
    for k in range(0, len(svs), 5):  # forged
        svs[k] = SignedVote(svs[k].vote, svs[k].voter, svs[(k + 1) % len(svs)].sig)
    svs.append(SignedVote(Vote(changes[0], era, 7), 99, sigs[0]))  # unknown voter
    rng.shuffle(svs)
    svs += svs[:6]  # replays of committed numbers
    faults = ct.add_committed_batch([(p, svs[p::5]) for p in range(5)])
    return faults, dict(ct.committed), ct.compute_winner(), ct.calls, ct.checks


def test_vote_counter_device_hash(dev):
    want = committed_batch_run(dev, False)
    assert hash_launches(dev) == 0
    got = committed_batch_run(dev, True)
    assert hash_launches(dev) == 1
    assert got == want
    assert len(want[0]) > 0 and want[3] == 1
