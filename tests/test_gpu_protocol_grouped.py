"""BatchVerifier(grouped=True): a drain's signature-share and decryption-share checks go through the
grouped engine calls.  One ThresholdSign flow and one ThresholdDecrypt flow at N = 7, each with a faulty
share in the drained batch, give the same outputs, fault logs and messages with the option off and on."""
import random

import pytest

from oracle import bls12_381 as C
from oracle import cbls, tc
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a
from hbbft_amd.protocol import BatchVerifier, Ciphertext, NetworkInfo, ThresholdDecrypt, ThresholdSign

pytestmark = pytest.mark.gpu
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
N, F = 7, 2


class Spy:
    """The engine, recording the names of the calls made through it."""

    def __init__(self, engine):
        self._engine, self.names = engine, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._engine, name)


def keyset(rng):
    coeffs = [rng.randrange(1, C.R) for _ in range(F + 1)]
    sks = {i: tc.poly_eval(coeffs, i + 1) for i in range(N)}
    pks = {i: cbls.g1_mul(G1, sks[i]) for i in range(N)}
    return coeffs, sks, pks, cbls.g1_mul(G1, coeffs[0])


def record(log, step):
    log.append((list(step.output), list(step.fault_log), list(step.messages)))


def sign_flow(engine, grouped):
    rng = random.Random(1613)
    coeffs, sks, pks, mpk = keyset(rng)
    h = cbls.g2_mul(G2, rng.randrange(1, C.R))
    spy = Spy(engine)
    node = ThresholdSign(NetworkInfo(0, range(N), F, mpk, pks, sign_g2=lambda H: cbls.g2_mul(H, sks[0])),
                         BatchVerifier(spy, grouped=grouped))
    log = []
    # shares of nodes 1..5 arrive before the document (node 3 lies): verified in one drain at sign()
    for j in range(1, 6):
        share = cbls.g2_mul(G2, 4242) if j == 3 else cbls.g2_mul(h, sks[j])
        record(log, node.handle_message(j, share))
    node.set_document_hash(h)
    record(log, node.handle_input())
    record(log, node.handle_message(6, cbls.g2_mul(h, sks[6])))
    return log, cbls.g2_mul(h, coeffs[0]), spy.names, node.verifier


def decrypt_flow(engine, grouped):
    rng = random.Random(1614)
    coeffs, sks, pks, mpk = keyset(rng)
    msg = bytes(rng.randrange(256) for _ in range(64))
    mpk_pt = (int.from_bytes(mpk[:48], "little"), int.from_bytes(mpk[48:], "little"))
    u, v, w = tc.encrypt(mpk_pt, msg, rng.randrange(1, C.R))
    ct = Ciphertext(g1a(C.g1_uncompressed(u)), v, g2a(C.g2_uncompressed(w)), g2a(C.g2_uncompressed(tc.hash_g1_g2(u, v))))
    spy = Spy(engine)
    node = ThresholdDecrypt(NetworkInfo(0, range(N), F, mpk, pks, decrypt_share=lambda U: cbls.g1_mul(U, sks[0])),
                            BatchVerifier(spy, grouped=grouped))
    log = []
    for j in range(1, 6):  # node 4 lies
        share = cbls.g1_mul(G1, 999) if j == 4 else cbls.g1_mul(ct.u, sks[j])
        record(log, node.handle_message(j, share))
    node.set_ciphertext(ct)
    record(log, node.handle_input())
    record(log, node.handle_message(6, cbls.g1_mul(ct.u, sks[6])))
    return log, msg, spy.names, node.verifier


def test_threshold_sign_grouped_matches_default(engine):
    off, want, names_off, v_off = sign_flow(engine, False)
    on, _, names_on, v_on = sign_flow(engine, True)
    assert on == off
    assert [flt.node_id for _, faults, _ in off for flt in faults] == [3]
    assert [out for outs, _, _ in off for out in outs] == [want]
    assert "verify_sig_shares_grouped" in names_on and "verify_sig_shares" not in names_on
    assert "verify_sig_shares" in names_off and "verify_sig_shares_grouped" not in names_off
    assert (v_on.calls, v_on.checks, v_on.max_batch) == (v_off.calls, v_off.checks, v_off.max_batch)
    assert v_on.max_batch >= 5  # the early shares were one drain: a group of five with one bad share


def test_threshold_decrypt_grouped_matches_default(engine):
    off, msg, names_off, v_off = decrypt_flow(engine, False)
    on, _, names_on, v_on = decrypt_flow(engine, True)
    assert on == off
    assert [flt.node_id for _, faults, _ in off for flt in faults] == [4]
    assert [out for outs, _, _ in off for out in outs] == [msg]
    assert "verify_dec_shares_grouped" in names_on and "verify_dec_shares" not in names_on
    assert "verify_dec_shares" in names_off and "verify_dec_shares_grouped" not in names_off
    assert "verify_ciphertexts" in names_on  # ciphertext checks are unchanged
    assert (v_on.calls, v_on.checks, v_on.max_batch) == (v_off.calls, v_off.checks, v_off.max_batch)


def test_grouped_takes_no_g2_set(engine):
    with pytest.raises(ValueError):
        BatchVerifier(engine, g2_capacity=4, grouped=True)
    assert BatchVerifier(engine).grouped is False
