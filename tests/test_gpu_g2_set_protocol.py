"""BatchVerifier(engine, g2_capacity=...) on the flows of tests/test_gpu_protocol.py: a ThresholdSign
network and a ThresholdDecrypt network at N = 4, f = 1, several instances per node on ONE verdict
cache, one forged share each.  Each network runs with g2_capacity = 0 (no resident set) and with a
set smaller than the number of open keys, so some keys are resident and the others take the
stateless call in the same drain.  Both runs give the same outputs, the same faults in the same
order, the same verdict cache after every drain and the same counters."""
import random

import pytest

from oracle import bls12_381 as C
from oracle import cbls, tc
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a
from hbbft_amd.protocol import BatchVerifier, Ciphertext, NetworkInfo, ThresholdDecrypt, ThresholdSign

pytestmark = pytest.mark.gpu
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
N, F = 4, 1


class Spy:
    """The engine, with the names of the calls made through it."""

    def __init__(self, engine):
        self._engine, self.names = engine, []

    def __getattr__(self, name):
        attr = getattr(self._engine, name)
        if not callable(attr):
            return attr

        def call(*args, **kw):
            self.names.append(name)
            return attr(*args, **kw)
        return call


def keyset(rng):
    coeffs = [rng.randrange(1, C.R) for _ in range(F + 1)]
    sks = {i: tc.poly_eval(coeffs, i + 1) for i in range(N)}
    pks = {i: cbls.g1_mul(G1, sks[i]) for i in range(N)}
    return coeffs, sks, pks, cbls.g1_mul(G1, coeffs[0])


def snapshot(ver):
    """the verdict cache, as plain sorted data"""
    return (sorted((h, sorted(d.items())) for h, d in ver._sig.items()),
            sorted((c, sorted(d.items())) for c, d in ver._dec.items()),
            sorted((c, sorted(d.items())) for c, d in ver._ct.items()))


def deliver(rng, queue, window, nodes, ver, queue_check, trace, outputs, faults, forged):
    """Windows of deliveries in seeded order: the window's shares are verified in one drain, then
    handled.  The forged share travels in the first window, before any receiver can have terminated."""
    first = [m for m in queue if m[3] == forged]
    queue[:] = [m for m in queue if m[3] != forged]
    while first or queue:
        batch = first + [queue.pop(rng.randrange(len(queue))) for _ in range(min(window - len(first), len(queue)))]
        first = []
        for sender, target, inst, payload in batch:
            queue_check(sender, target, inst, payload)
        ver.drain()
        trace.append(snapshot(ver))
        for sender, target, inst, payload in batch:
            step = nodes[target, inst].handle_message(sender, payload)
            assert step.messages == []
            outputs.setdefault((target, inst), []).extend(step.output)
            faults += [(target, inst, flt.node_id, flt.kind) for flt in step.fault_log]
        trace.append(snapshot(ver))


def run_sign(engine, g2_capacity, ndocs=3, liar=3):
    rng = random.Random(2024)
    coeffs, sks, pks, mpk = keyset(rng)
    hs = [cbls.g2_mul(G2, rng.randrange(1, C.R)) for _ in range(ndocs)]
    spy = Spy(engine)
    ver = BatchVerifier(spy, g2_capacity=g2_capacity)
    nodes, queue, outputs, faults, trace = {}, [], {}, [], []
    forged = cbls.g2_mul(hs[0], sks[liar])
    for i in range(N):
        for d, h in enumerate(hs):
            ni = NetworkInfo(i, range(N), F, mpk, pks, sign_g2=lambda H, sk=sks[i]: cbls.g2_mul(H, sk))
            nodes[i, d] = ts = ThresholdSign(ni, ver)
            ts.set_document_hash(h)
            step = ts.handle_input()
            for _, share in step.messages:
                if i == liar and d == 1:  # one forged share: document 0's share sent for document 1
                    share = forged
                queue += [(i, j, d, share) for j in range(N) if j != i]
            outputs.setdefault((i, d), []).extend(step.output)
            faults += [(i, d, flt.node_id, flt.kind) for flt in step.fault_log]

    def queue_check(sender, target, d, share):
        if not nodes[target, d].terminated:
            ver.queue_sig(pks[sender], hs[d], share)

    deliver(rng, queue, 7, nodes, ver, queue_check, trace, outputs, faults, forged)
    want = {(i, d): [cbls.g2_mul(hs[d], coeffs[0])] for i in range(N) for d in range(ndocs)}
    return dict(outputs=outputs, faults=faults, trace=trace, want=want,
                counters=(ver.calls, ver.checks, ver.max_batch, ver.lookups)), spy.names, ver


def run_decrypt(engine, g2_capacity, ncts=2, liar=3):
    rng = random.Random(4048)
    coeffs, sks, pks, mpk = keyset(rng)
    mpk_pt = (int.from_bytes(mpk[:48], "little"), int.from_bytes(mpk[48:], "little"))
    msgs = [bytes(rng.randrange(256) for _ in range(40 + 9 * k)) for k in range(ncts)]
    cts = []
    for msg in msgs:
        u, v, w = tc.encrypt(mpk_pt, msg, rng.randrange(1, C.R))
        cts.append(Ciphertext(g1a(C.g1_uncompressed(u)), v, g2a(C.g2_uncompressed(w)),
                              g2a(C.g2_uncompressed(tc.hash_g1_g2(u, v)))))
    spy = Spy(engine)
    ver = BatchVerifier(spy, g2_capacity=g2_capacity)
    nodes, queue, outputs, faults, trace = {}, [], {}, [], []
    forged = cbls.g1_mul(G1, 999)
    for i in range(N):
        for k, ct in enumerate(cts):
            ni = NetworkInfo(i, range(N), F, mpk, pks, decrypt_share=lambda U, sk=sks[i]: cbls.g1_mul(U, sk))
            nodes[i, k] = td = ThresholdDecrypt(ni, ver)
            td.set_ciphertext(ct)
            step = td.handle_input()
            for _, share in step.messages:
                if i == liar and k == 0:  # one forged share
                    share = forged
                queue += [(i, j, k, share) for j in range(N) if j != i]
            outputs.setdefault((i, k), []).extend(step.output)
            faults += [(i, k, flt.node_id, flt.kind) for flt in step.fault_log]

    def queue_check(sender, target, k, share):
        if not nodes[target, k].terminated:
            ver.queue_dec(pks[sender], share, cts[k].huv, cts[k].w)

    deliver(rng, queue, 5, nodes, ver, queue_check, trace, outputs, faults, forged)
    want = {(i, k): [msgs[k]] for i in range(N) for k in range(ncts)}
    return dict(outputs=outputs, faults=faults, trace=trace, want=want,
                counters=(ver.calls, ver.checks, ver.max_batch, ver.lookups)), spy.names, ver


def test_threshold_sign_network_with_a_small_set(engine):
    plain, plain_calls, _ = run_sign(engine, 0)
    resident, set_calls, ver = run_sign(engine, 2)  # 3 documents open at once, 2 slots
    assert plain["outputs"] == plain["want"]
    assert plain["faults"] and all(f[1:] == (1, 3, "UnverifiedSignatureShareSender") for f in plain["faults"])
    assert resident == plain
    # the first run never names a set; the second verifies resident documents through it and the
    # document that found no slot through the stateless call
    assert not any("set" in name for name in plain_calls)
    assert "verify_sig_shares_set" in set_calls and "verify_sig_shares" in set_calls
    assert ver._g2.size()[1] == 2 and not ver._g2_slot and not ver._g2_pending  # every instance terminated


def test_threshold_decrypt_network_with_a_small_set(engine):
    plain, plain_calls, _ = run_decrypt(engine, 0)
    resident, set_calls, ver = run_decrypt(engine, 3)  # 2 ciphertexts = 4 points, 3 slots
    assert plain["outputs"] == plain["want"]
    assert plain["faults"] and all(f[1:] == (0, 3, "UnverifiedDecryptionShareSender") for f in plain["faults"])
    assert resident == plain
    assert not any("set" in name for name in plain_calls)
    assert "verify_dec_shares_set" in set_calls and "verify_dec_shares" in set_calls
    assert ver._g2.size()[1] == 3 and not ver._g2_slot and not ver._g2_pending
