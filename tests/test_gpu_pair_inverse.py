"""HBH_IMPL_PAIR (the lane-pair kernel k_pair_verify) with the branch-free binary-GCD inverse
(csrc/words.hpp INV_UNIFORM) in the six inversions of a check's final exponentiation: one in the easy
part (pfp.hpp h6_inv) and one per exponentiation by |x| (k_pair.hip h_exp_tail).

Every lane pair gets operands of its own, so a wave holds 32 different norms and 32 different GCD
traces.  Value bytes: dbg_pairing at 1, 33 and 129 pairs equals the C oracle's pairing and
HBH_IMPL_WAVE's bytes; pairs with P = O, Q = O or both give f = 1 (norm 1, and the exponentiations take
the Granger-Scott path) next to ordinary ones.  Verdicts: the sign shape at 65 checks (two waves and
one pair), a key per check, valid, wrong and infinity cases mixed, equals the oracle's verify_g2.
Bar: bit-exact bytes.
"""
import random

import pytest

from oracle import bls12_381 as C
from oracle import cbls
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a

pytestmark = pytest.mark.gpu

IMPL_AUTO, IMPL_PAIR, IMPL_WAVE = 3, 4, 5
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
O1, O2 = bytes(96), bytes(192)
NPAIR = 129
P_INF, Q_INF, BOTH_INF = (3, 40), (5, 77), (7, 128)   # 3, 5, 7 lie in the 33-pair prefix too
ONE = b"".join(c.to_bytes(48, "little") for six in C.F12_ONE for f2 in six for c in f2)


@pytest.fixture(scope="module")
def pairs():
    """129 pairs with distinct random operands and the oracle's values, made once; the sizes take prefixes"""
    rng = random.Random(0x696e76)
    P = [cbls.g1_mul(G1, rng.randrange(1, C.R)) for _ in range(NPAIR)]
    Q = [cbls.g2_mul(G2, rng.randrange(1, C.R)) for _ in range(NPAIR)]
    for i in P_INF + BOTH_INF:
        P[i] = O1
    for i in Q_INF + BOTH_INF:
        Q[i] = O2
    want = [ONE if (p == O1 or q == O2) else cbls.pairing(p, q) for p, q in zip(P, Q)]
    assert len(set(want)) == NPAIR - len(P_INF + Q_INF + BOTH_INF) + 1
    return P, Q, want


def with_impl(engine, impl, call):
    engine.set_pairing_impl(impl)
    try:
        return call()
    finally:
        engine.set_pairing_impl(IMPL_AUTO)


@pytest.mark.parametrize("n", [1, 33, 129])
def test_pairing_value_bytes(engine, pairs, n):
    P, Q, want = (col[:n] for col in pairs)
    pair = with_impl(engine, IMPL_PAIR, lambda: engine.dbg_pairing(P, Q))
    wave = with_impl(engine, IMPL_WAVE, lambda: engine.dbg_pairing(P, Q))
    assert list(pair) == want
    assert list(pair) == list(wave)


def test_sign_verdicts_65(engine):
    """two waves and one pair; a key, a signature and a verdict per check"""
    rng = random.Random(0x363535)
    n, ndoc = 65, 3
    H = [cbls.g2_mul(G2, rng.randrange(1, C.R)) for _ in range(ndoc)]
    kinds = ["valid", "wrong", "valid", "other_doc", "g2_inf", "valid", "g1_inf", "both_inf"]
    pks, sigs, didx = [], [], []
    for i in range(n):
        sk, d, kind = rng.randrange(1, C.R), i % ndoc, kinds[i % len(kinds)]
        pk, sig = cbls.g1_mul(G1, sk), cbls.g2_mul(H[d], sk)
        if kind == "wrong":
            sig = cbls.g2_mul(H[d], (sk + 1) % C.R)
        elif kind == "other_doc":
            sig = cbls.g2_mul(H[(d + 1) % ndoc], sk)
        elif kind == "g2_inf":
            sig = O2
        elif kind == "g1_inf":
            pk = O1
        elif kind == "both_inf":
            pk, sig = O1, O2
        pks.append(pk)
        sigs.append(sig)
        didx.append(d)
    want = [int(cbls.verify_g2(pk, sig, H[d])) for pk, sig, d in zip(pks, sigs, didx)]
    assert want[:8] == [1, 0, 1, 0, 0, 1, 0, 1]
    got = with_impl(engine, IMPL_PAIR, lambda: list(engine.verify_sig_shares(pks, sigs, H, didx)))
    assert got == want
