"""HBH_IMPL_PAIR (the lane-pair kernel k_pair_verify), whose walked G2 side keeps T in homogeneous
coordinates (csrc/pfp.hpp h_dbl_step_h / h_add_step_h): every verdict equals the C oracle's and
HBH_IMPL_WAVE's on the same inputs.  HBH_IMPL_QUAD and HBH_IMPL_OCT run the same kernel body
(csrc/pair_side.hpp lane_verify) on four and eight lanes per check with the Jacobian walk, and are
held to the same verdicts: 33 crosses an octo workgroup (32 checks) and two quad waves (16 each).

Shapes: sign (verify_sig_shares: H tabled once at least 4 checks share a hash, sigma walked, P2 the
generator), walk on both sides (verify_signatures: one hash per check) and decrypt
(verify_dec_shares: both sides tabled, no walk -- the control for the Miller loop's first step and
the end of the final exponentiation, which any rewrite of the kernel around the walk touches).
Sizes: 1, 2, 33 (crosses a wave of 32 checks) and 129 (the second workgroup holds one check).
Below 4 checks per shared point the engine walks that side too.

Bar: bit-exact verdict bytes; bit-exact canonical Fp12 coefficients where the value is written.
"""
import random

import pytest

from oracle import bls12_381 as C
from oracle import cbls
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a

pytestmark = pytest.mark.gpu

IMPL_AUTO, IMPL_PAIR, IMPL_WAVE, IMPL_QUAD, IMPL_OCT = 3, 4, 5, 6, 7
SIZES = [1, 2, 33, 129]
NDOC = 4   # shared G2 points per call: 33 / 4 and 129 / 4 checks per point get a line table
NKEY = 5
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
O1, O2 = bytes(96), bytes(192)
KINDS = ["valid", "other_doc", "neg", "second_inf", "pk_inf", "g2", "2g2", "both_inf"]


def inv_r(a):
    return pow(a, C.R - 2, C.R)


class Material:
    """Keys and shared points with known discrete logarithms, made once per session."""

    def __init__(self):
        rng = random.Random(0x70616972)
        self.sk = [rng.randrange(1, C.R) for _ in range(NKEY)]
        self.pk = [cbls.g1_mul(G1, k) for k in self.sk]
        # document 0 hashes to g2 itself, document 1 to 2 g2: tables and walks of small multiples
        self.h = [1, 2] + [rng.randrange(1, C.R) for _ in range(NDOC - 2)]
        self.H = [cbls.g2_mul(G2, h) for h in self.h]
        # ciphertexts (U, W) = (r g1, r H_uv)
        self.r = [rng.randrange(1, C.R) for _ in range(NDOC)]
        self.U = [cbls.g1_mul(G1, r) for r in self.r]
        self.W = [cbls.g2_mul(H, r) for H, r in zip(self.H, self.r)]


@pytest.fixture(scope="module")
def mat():
    return Material()


def sign_item(m, i):
    """(pk, sigma, document) of check i: e(pk, H_d) == e(g1, sigma)"""
    d, j, kind = i % NDOC, i % NKEY, KINDS[i % len(KINDS)]
    pk, sig = m.pk[j], cbls.g2_mul(m.H[d], m.sk[j])
    if kind == "other_doc":
        sig = cbls.g2_mul(m.H[(d + 1) % NDOC], m.sk[j])
    elif kind == "neg":
        sig = cbls.g2_mul(m.H[d], C.R - m.sk[j])
    elif kind == "second_inf":
        sig = O2
    elif kind == "pk_inf":
        pk = O1
    elif kind == "g2":      # sigma = g2 under the key g1 / h_d
        pk, sig = cbls.g1_mul(G1, inv_r(m.h[d])), G2
    elif kind == "2g2":     # sigma = 2 g2 under the key 2 g1 / h_d
        pk, sig = cbls.g1_mul(G1, 2 * inv_r(m.h[d]) % C.R), cbls.g2_mul(G2, 2)
    elif kind == "both_inf":
        pk, sig = O1, O2
    return pk, sig, d


def dec_item(m, i):
    """(share, pk, ciphertext) of check i: e(share, H_uv) == e(pk, W)"""
    c, j, kind = i % NDOC, i % NKEY, KINDS[i % len(KINDS)]
    share, pk = cbls.g1_mul(m.U[c], m.sk[j]), m.pk[j]
    if kind == "other_doc":
        share = cbls.g1_mul(m.U[(c + 1) % NDOC], m.sk[j])
    elif kind == "neg":
        share = cbls.g1_mul(m.U[c], C.R - m.sk[j])
    elif kind == "second_inf":
        share = O1
    elif kind == "pk_inf":
        pk = O1
    elif kind == "g2":      # another share's key
        pk = m.pk[(j + 1) % NKEY]
    elif kind == "2g2":     # the doubled share under the doubled key
        share, pk = cbls.g1_mul(m.U[c], 2 * m.sk[j] % C.R), cbls.g1_mul(G1, 2 * m.sk[j] % C.R)
    elif kind == "both_inf":
        share, pk = O1, O1
    return share, pk, c


def both(engine, call):
    out = []
    try:
        for impl in (IMPL_PAIR, IMPL_WAVE, IMPL_QUAD, IMPL_OCT):
            engine.set_pairing_impl(impl)
            out.append(list(call()))
    finally:
        engine.set_pairing_impl(IMPL_AUTO)
    return out


def expect_mixed(want, n):
    """the batch holds accepted and rejected checks once it is long enough to hold every kind"""
    if n >= len(KINDS):
        assert 0 < sum(want) < n


@pytest.mark.parametrize("n", SIZES)
def test_sign_shape(engine, mat, n):
    items = [sign_item(mat, i) for i in range(n)]
    pks, sigs, didx = [a for a, _, _ in items], [b for _, b, _ in items], [d for _, _, d in items]
    want = [int(cbls.verify_g2(pk, sig, mat.H[d])) for pk, sig, d in items]
    pair, wave, quad, octo = both(engine, lambda: engine.verify_sig_shares(pks, sigs, mat.H, didx))
    assert pair == want
    assert wave == want
    assert quad == want
    assert octo == want
    expect_mixed(want, n)


@pytest.mark.parametrize("n", SIZES)
def test_walk_both_sides(engine, mat, n):
    items = [sign_item(mat, i) for i in range(n)]
    pks, sigs, hashes = [a for a, _, _ in items], [b for _, b, _ in items], [mat.H[d] for _, _, d in items]
    want = [int(cbls.verify_g2(pk, sig, h)) for pk, sig, h in zip(pks, sigs, hashes)]
    pair, wave, quad, octo = both(engine, lambda: engine.verify_signatures(pks, sigs, hashes))
    assert pair == want
    assert wave == want
    assert quad == want
    assert octo == want
    expect_mixed(want, n)


@pytest.mark.parametrize("n", SIZES)
def test_decrypt_shape(engine, mat, n):
    items = [dec_item(mat, i) for i in range(n)]
    shares, pks, cidx = [a for a, _, _ in items], [b for _, b, _ in items], [c for _, _, c in items]
    want = [int(cbls.pairing_eq(s, mat.H[c], pk, mat.W[c])) for s, pk, c in items]
    pair, wave, quad, octo = both(engine, lambda: engine.verify_dec_shares(shares, pks, mat.H, mat.W, cidx))
    assert pair == want
    assert wave == want
    assert quad == want
    assert octo == want
    expect_mixed(want, n)


def test_expected_verdicts_by_kind(mat):
    """the oracle's verdict for each input kind is the one the kind is built to give"""
    sign = {KINDS[i]: int(cbls.verify_g2(pk, sig, mat.H[d])) for i in range(len(KINDS))
            for pk, sig, d in [sign_item(mat, i)]}
    assert sign == {"valid": 1, "other_doc": 0, "neg": 0, "second_inf": 0, "pk_inf": 0, "g2": 1, "2g2": 1,
                    "both_inf": 1}
    dec = {KINDS[i]: int(cbls.pairing_eq(s, mat.H[c], pk, mat.W[c])) for i in range(len(KINDS))
           for s, pk, c in [dec_item(mat, i)]}
    assert dec == {"valid": 1, "other_doc": 0, "neg": 0, "second_inf": 0, "pk_inf": 0, "g2": 0, "2g2": 1,
                   "both_inf": 1}


def test_pairing_value_33(engine, mat):
    """value_out set (the path of test_pairing_value_matches_oracle): PAIR, QUAD and OCT write the
    oracle's bytes (e(P, Q)^3) at 33 pairs, also for P = O, Q = O and the small multiples of g2."""
    rng = random.Random(33)
    P = [cbls.g1_mul(G1, rng.randrange(1, C.R)) for _ in range(33)]
    Q = [cbls.g2_mul(G2, rng.randrange(1, C.R)) for _ in range(33)]
    P[3], Q[5] = O1, O2
    Q[7], Q[8] = G2, cbls.g2_mul(G2, 2)
    one = b"".join(c.to_bytes(48, "little") for six in C.F12_ONE for f2 in six for c in f2)
    want = [one if (p == O1 or q == O2) else cbls.pairing(p, q) for p, q in zip(P, Q)]
    try:
        for impl in (IMPL_PAIR, IMPL_QUAD, IMPL_OCT):
            engine.set_pairing_impl(impl)
            assert engine.dbg_pairing(P, Q) == want, impl
    finally:
        engine.set_pairing_impl(IMPL_AUTO)
