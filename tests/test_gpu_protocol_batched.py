"""The protocol paths with batched=True (SyncKeyGen's Ciphertext::verify through
Engine.verify_ciphertexts_uv_batched; DhbKeyGen's and VoteCounter's PublicKey::verify through
Engine.verify_signed_batched) against the same flows with batched=False, both with device_hash=True, from
the same seeds: identical messages, outcomes, fault lists and keys.  Each flow has one faulty sender.  The
flows are those of tests/test_gpu_sync_key_gen_device_hash.py and tests/test_gpu_verify_signed.py at
N = 4, t = 1."""
import random

import pytest

from hbbft_amd import hoststage
from hbbft_amd.dynamic_honey_badger import (DhbKeyGen, SignedKeyGenMsg, SignedVote, Vote, VoteCounter,
                                            encryption_schedule, key_gen_msg_bytes, node_change, vote_bytes)
from hbbft_amd.sync_key_gen import G1_GEN, G2_GEN, R_ORDER, Ack, Ciphertext, Part, SyncKeyGen

pytestmark = pytest.mark.gpu
BATCHED = ("verify_ciphertexts_uv_batched", "verify_signed_batched")
PLAIN = ("verify_ciphertexts_uv", "verify_signed")


class Spy:
    """The engine, counting the calls made through it."""

    def __init__(self, engine):
        self._engine, self.calls = engine, {}

    def __getattr__(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1
        return getattr(self._engine, name)


def key_gen_run(engine, batched):
    n, t = 4, 1
    rng = random.Random(2504)
    sks = [rng.randrange(1, R_ORDER) for _ in range(n)]
    pub = dict(enumerate(hoststage.g1_mul([G1_GEN] * n, sks)))
    nodes, props = [], []
    for i in range(n):
        kg, part = SyncKeyGen.new(i, sks[i], pub, t, engine, rng=rng, device_hash=True, batched=batched)
        nodes.append(kg)
        props.append(part)
    log = {"parts": [p.to_bytes() for p in props], "acks": [], "part_out": [], "ack_out": []}
    # sender 3 is faulty: its row for node 1 carries another row's W (DecryptRow at node 1 only)
    rows = list(props[3].rows)
    rows[1] = Ciphertext(rows[1].u, rows[1].v, rows[0].w)
    bad_part = Part(props[3].degree, props[3].commit, rows)
    acks = [[] for _ in range(t + 1)]
    for node_id, node in enumerate(nodes):  # three Parts in one call: one ciphertext batch of three
        outs = node.handle_parts([(0, props[0]), (1, props[1]), (3, bad_part)], rng)
        for sender, out in zip((0, 1, 3), outs):
            log["part_out"].append((sender, node_id, out.fault))
            log["acks"].append(out.ack.to_bytes() if out.ack else None)
            if sender <= t and node_id <= 2 * t:
                acks[sender].append((node_id, out.ack))
    # node 2's Ack for proposal 1 with the value for node 0 tampered: DecryptValue at node 0
    who, ack = acks[1][2]
    vals = list(ack.values)
    vals[0] = Ciphertext(vals[0].u, bytes([vals[0].v[0] ^ 1]) + vals[0].v[1:], vals[0].w)
    bad_ack = (who, Ack(ack.proposer_idx, vals))
    for node_id, node in enumerate(nodes):
        batch = acks[0] + acks[1][:2] + [bad_ack if node_id == 0 else acks[1][2]]
        log["ack_out"].append([o.fault for o in node.handle_acks(batch)])
        log["ack_out"].append(node.is_ready())
    log["keys"] = [node.generate() for node in nodes]
    return log


def test_sync_key_gen_batched(engine):
    plain, batched = Spy(engine), Spy(engine)
    want = key_gen_run(plain, False)
    got = key_gen_run(batched, True)
    assert got == want
    assert [o for o in want["part_out"] if o[2] is not None] == [(3, 1, "DecryptRow")]
    assert want["ack_out"][0] == [None] * 5 + ["DecryptValue"] and want["ack_out"][2] == [None] * 6
    assert all(want["ack_out"][1::2])
    assert batched.calls.get(BATCHED[0], 0) == plain.calls.get(PLAIN[0], 0) > 0
    assert PLAIN[0] not in batched.calls and BATCHED[0] not in plain.calls


def dhb_run(engine, batched):
    rng = random.Random(2505)
    n, t, era = 4, 1, 7
    sks = [rng.randrange(1, R_ORDER) for _ in range(n)]
    pub = dict(enumerate(hoststage.g1_mul([G1_GEN] * n, sks)))
    current = {i: pub[i] for i in range(n - 1)}  # node 3 is a joining candidate: no current key
    dhbs, parts = [], []
    for i in range(n):
        kg, part = SyncKeyGen.new(i, sks[i], pub, t, engine, rng=rng, device_hash=True, batched=batched)
        dhbs.append(DhbKeyGen(engine, era, i, sks[i], current, key_gen=kg, candidate_keys=pub, device_hash=True,
                              batched=batched))
        parts.append(part)
    for i in range(n):
        dhbs[i].send_transaction(parts[i])
    contributions = [(i, list(dhbs[i].key_gen_msg_buffer)) for i in range(n)]
    forged = SignedKeyGenMsg(era, 0, parts[0], hoststage.g2_mul([G2_GEN], [12345])[0])  # proposer 1 is faulty
    contributions[1] = (1, contributions[1][1] + [forged])
    log = []
    for d in dhbs:
        step = d.handle_committed(contributions, rng)
        sent = [(to, kind, e, key_gen_msg_bytes(m), sig) for to, (kind, e, m, sig) in step.messages]
        log.append(([(f.node_id, f.kind) for f in step.fault_log], sent, d.calls, d.checks))
    contributions = [(i, list(dhbs[i].key_gen_msg_buffer)) for i in range(n)]
    for d in dhbs:
        step = d.handle_committed(contributions, rng)
        log.append(([(f.node_id, f.kind) for f in step.fault_log], d.key_gen.is_ready(), d.calls, d.checks))
    log.append([d.key_gen.generate() for d in dhbs])
    return log


def test_dhb_key_gen_batched(engine):
    plain, batched = Spy(engine), Spy(engine)
    want = dhb_run(plain, False)
    got = dhb_run(batched, True)
    assert got == want
    assert want[0][0] == [(1, "InvalidKeyGenMessageSignature")]
    assert all(ready for _, ready, _, _ in want[4:8])
    for b, p in zip(BATCHED, PLAIN):
        assert batched.calls.get(b, 0) == plain.calls.get(p, 0) > 0
        assert p not in batched.calls and b not in plain.calls


def votes_run(engine, batched):
    n, era = 7, 9
    rng = random.Random(2506)
    sks = [rng.randrange(1, R_ORDER) for _ in range(n)]
    pks = dict(enumerate(hoststage.g1_mul([G1_GEN] * n, sks)))
    ct = VoteCounter(engine, era, 0, sks[0], pks, (n - 1) // 3, device_hash=True, batched=batched)
    changes = [node_change({j: pks[j]}) for j in range(2)] + [encryption_schedule("EveryNthEpoch", 4)]
    votes = [(voter, Vote(changes[voter % 3], era, 0)) for voter in range(n)]
    hs = hoststage.hash_g2(vote_bytes([v for _, v in votes]))
    sigs = hoststage.g2_mul(hs, [sks[voter] for voter, _ in votes])
    svs = [SignedVote(v, voter, s) for (voter, v), s in zip(votes, sigs)]
    svs[4] = SignedVote(svs[4].vote, svs[4].voter, svs[5].sig)  # voter 4's vote is forged: proposer 1 is faulty
    ok = ct.validate(svs)
    faults = ct.add_committed_batch([(p, svs[p::3]) for p in range(3)])
    return ok, faults, dict(ct.committed), ct.compute_winner(), ct.calls, ct.checks


def test_vote_counter_batched(engine):
    plain, batched = Spy(engine), Spy(engine)
    want = votes_run(plain, False)
    got = votes_run(batched, True)
    assert got == want
    assert want[0] == [True] * 4 + [False] + [True] * 2 and len(want[1]) == 1
    assert batched.calls.get(BATCHED[1], 0) == plain.calls.get(PLAIN[1], 0) > 0
    assert PLAIN[1] not in batched.calls and BATCHED[1] not in plain.calls


def test_batched_needs_device_hash(engine):
    with pytest.raises(ValueError):
        SyncKeyGen(0, 1, {0: G1_GEN}, 0, engine, batched=True)
    with pytest.raises(ValueError):
        DhbKeyGen(engine, 0, 0, 1, {0: G1_GEN}, batched=True)
    with pytest.raises(ValueError):
        VoteCounter(engine, 0, 0, 1, {0: G1_GEN}, 0, batched=True)
