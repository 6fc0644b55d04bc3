"""SyncKeyGen with device_hash=True (Ciphertext::verify through Engine.verify_ciphertexts_uv, encryption
through Engine.encrypt, the hash form forced to DEVICE) against the default host-stage path from the same
seeds: the same Part and Ack bytes, outcomes, faults and generated keys.  The flow is
tests/test_gpu_sync_key_gen.py::test_sync_key_gen at N = 4, t = 1 with one tampered Part row and one
tampered Ack value; the DynamicHoneyBadger scenario is tests/test_gpu_dhb_key_gen.py's."""
import random

import pytest

from hbbft_amd import _lib, hoststage
from hbbft_amd.dynamic_honey_badger import DhbKeyGen, SignedKeyGenMsg, key_gen_msg_bytes
from hbbft_amd.sync_key_gen import G1_GEN, G2_GEN, R_ORDER, Ack, Ciphertext, Part, SyncKeyGen

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev(engine):
    engine.set_hash_impl(_lib.HASH_DEVICE)
    engine.set_profiling(True)
    yield engine
    engine.set_profiling(False)
    engine.set_hash_impl(_lib.HASH_AUTO)


def hash_launches(engine):
    return engine.stage_time(_lib.STAGE_HASH)[1]


def key_gen_run(engine, device_hash):
    """Everything the N = 4, t = 1 flow sends and decides, as comparable values"""
    n, t = 4, 1
    rng = random.Random(1004)
    sks = [rng.randrange(1, R_ORDER) for _ in range(n)]
    pub = dict(enumerate(hoststage.g1_mul([G1_GEN] * n, sks)))
    nodes, props = [], []
    for i in range(n):
        kg, part = SyncKeyGen.new(i, sks[i], pub, t, engine, rng=rng, device_hash=device_hash)
        nodes.append(kg)
        props.append(part)
    log = {"parts": [p.to_bytes() for p in props], "acks": [], "part_out": [], "ack_out": []}
    # a Part whose row for node 1 carries another row's W: DecryptRow at node 1 only
    rows = list(props[3].rows)
    rows[1] = Ciphertext(rows[1].u, rows[1].v, rows[0].w)
    bad_part = Part(props[3].degree, props[3].commit, rows)
    acks = [[] for _ in range(t + 1)]
    for sender in range(t + 1):
        for node_id, node in enumerate(nodes):
            out = node.handle_parts([(sender, props[sender])], rng)[0]
            log["part_out"].append((sender, node_id, out.fault))
            log["acks"].append(out.ack.to_bytes())
            if node_id <= 2 * t:
                acks[sender].append((node_id, out.ack))
    for node_id, node in enumerate(nodes):
        out = node.handle_parts([(3, bad_part)], rng)[0]
        log["part_out"].append((3, node_id, out.fault, out.ack.to_bytes() if out.ack else None))
    # node 2's Ack for proposal 1 with the value for node 0 tampered (a V byte flipped): DecryptValue at node 0
    who, ack = acks[1][2]
    vals = list(ack.values)
    c = vals[0]
    vals[0] = Ciphertext(c.u, bytes([c.v[0] ^ 1]) + c.v[1:], c.w)
    bad_ack = (who, Ack(ack.proposer_idx, vals))
    for node_id, node in enumerate(nodes):
        batch = acks[0] + acks[1][:2] + [bad_ack if node_id == 0 else acks[1][2]]
        log["ack_out"].append([o.fault for o in node.handle_acks(batch)])
        log["ack_out"].append(node.is_ready())
    log["keys"] = [node.generate() for node in nodes]
    return log


def test_same_messages_outcomes_and_keys(dev):
    want = key_gen_run(dev, False)
    assert hash_launches(dev) == 0  # the default keeps every hash on the host stage
    got = key_gen_run(dev, True)
    assert hash_launches(dev) > 0
    assert got["parts"] == want["parts"] and got["acks"] == want["acks"]
    assert got == want
    faults = [o for o in want["part_out"] if o[2] is not None]
    assert faults == [(3, 1, "DecryptRow", None)]
    assert want["ack_out"][0] == [None] * 5 + ["DecryptValue"] and want["ack_out"][2] == [None] * 6
    assert all(want["ack_out"][1::2])
    assert all(pks == want["keys"][0][0] for pks, _ in want["keys"])


def dhb_run(engine, device_hash):
    """tests/test_gpu_dhb_key_gen.py's scenario (four nodes sign their Parts and Acks, a forged signature, a
    wrong-era copy), the flag given to DhbKeyGen and to the SyncKeyGen it drives"""
    rng = random.Random(77)
    n, t, era = 4, 1, 7
    sks = [rng.randrange(1, R_ORDER) for _ in range(n)]
    pub = dict(enumerate(hoststage.g1_mul([G1_GEN] * n, sks)))
    current = {i: pub[i] for i in range(n - 1)}
    dhbs, parts = [], []
    for i in range(n):
        kg, part = SyncKeyGen.new(i, sks[i], pub, t, engine, rng=rng, device_hash=device_hash)
        dhbs.append(DhbKeyGen(engine, era, i, sks[i], current, key_gen=kg, candidate_keys=pub, device_hash=device_hash))
        parts.append(part)
    for i in range(n):
        dhbs[i].send_transaction(parts[i])
    contributions = [(i, list(dhbs[i].key_gen_msg_buffer)) for i in range(n)]
    forged = SignedKeyGenMsg(era, 0, parts[0], hoststage.g2_mul([G2_GEN], [12345])[0])
    stale = SignedKeyGenMsg(era - 1, 2, parts[2], contributions[2][1][0].sig)
    contributions[1] = (1, contributions[1][1] + [forged])
    contributions[2] = (2, [stale] + contributions[2][1])
    log = [[p.to_bytes() for p in parts]]
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


def test_dhb_key_gen_device_hash(dev):
    want = dhb_run(dev, False)
    assert hash_launches(dev) == 0
    got = dhb_run(dev, True)
    assert hash_launches(dev) > 8  # the signature batches (8 calls) and SyncKeyGen's ciphertext batches
    assert got == want
    assert want[1][0] == [(1, "InvalidKeyGenMessageSignature"), (2, "InvalidKeyGenMessageEra")]
    assert all(ready for _, ready, _, _ in want[5:9])
