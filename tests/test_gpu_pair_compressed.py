"""HBH_IMPL_PAIR (the lane-pair kernel k_pair_verify) with the final exponentiation's powers of |x|
taken through compressed cyclotomic squarings (csrc/k_pair.hip h_exp_abs_x): every verdict equals
the C oracle's and HBH_IMPL_WAVE's on the same inputs, and the pairing value's bytes equal both.
HBH_IMPL_QUAD and HBH_IMPL_OCT share the kernel body and the final-exponentiation chain
(csrc/pair_side.hpp lane_verify, final_exp) with the plain Granger-Scott loop, and are held to the
same verdicts and bytes.

The compressed form cannot express an element whose a1 coefficient is zero; the kernel then runs the
Granger-Scott loop for that exponentiation.  A check with a G1 or G2 operand at infinity has f = 1
on that side; with both pairs masked, g = 1 compresses to four zeros and takes that path.  Every
batch below of 8 checks or more holds such checks next to valid and rejected ones, so at 33 and 129
both paths run divergently inside one wave.

Shapes: sign (verify_sig_shares: H tabled, sigma walked, P2 the generator), walk on both sides
(verify_signatures) and decrypt (verify_dec_shares: both sides tabled).
Sizes: 1 (one lane pair), 2, 33 (a partial second wave) and 129 (the second workgroup holds one
check).  Bar: bit-exact verdict bytes; bit-exact canonical Fp12 coefficients for the value.
"""
import random

import pytest

from oracle import bls12_381 as C
from oracle import cbls
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a

pytestmark = pytest.mark.gpu

IMPL_AUTO, IMPL_PAIR, IMPL_WAVE, IMPL_QUAD, IMPL_OCT = 3, 4, 5, 6, 7
SIZES = [1, 2, 33, 129]
NDOC = 4   # shared G2 points per call: at 33 and 129 each gets a line table
NKEY = 5
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
O1, O2 = bytes(96), bytes(192)
# valid, a wrong share, a share for another document, a G2 / a G1 operand at infinity, both
KINDS = ["valid", "wrong", "other_doc", "g2_inf", "g1_inf", "valid", "both_inf"]
WANT = {"valid": 1, "wrong": 0, "other_doc": 0, "g2_inf": 0, "g1_inf": 0, "both_inf": 1}


class Material:
    """Keys and shared points, made once per module."""

    def __init__(self):
        rng = random.Random(0x636f6d70)
        self.sk = [rng.randrange(1, C.R) for _ in range(NKEY)]
        self.pk = [cbls.g1_mul(G1, k) for k in self.sk]
        self.H = [cbls.g2_mul(G2, rng.randrange(1, C.R)) for _ in range(NDOC)]
        self.r = [rng.randrange(1, C.R) for _ in range(NDOC)]
        self.U = [cbls.g1_mul(G1, r) for r in self.r]
        self.W = [cbls.g2_mul(H, r) for H, r in zip(self.H, self.r)]
        self.sign, self.dec = {}, {}   # items and the oracle's verdicts, shared by the sizes

    def sign_item(self, i):
        """(pk, sigma, document, oracle verdict) of check i: e(pk, H_d) == e(g1, sigma)"""
        if i not in self.sign:
            d, j, kind = i % NDOC, i % NKEY, KINDS[i % len(KINDS)]
            pk, sig = self.pk[j], cbls.g2_mul(self.H[d], self.sk[j])
            if kind == "wrong":
                sig = cbls.g2_mul(self.H[d], (self.sk[j] + 1) % C.R)
            elif kind == "other_doc":
                sig = cbls.g2_mul(self.H[(d + 1) % NDOC], self.sk[j])
            elif kind == "g2_inf":
                sig = O2
            elif kind == "g1_inf":
                pk = O1
            elif kind == "both_inf":
                pk, sig = O1, O2
            want = int(cbls.verify_g2(pk, sig, self.H[d]))
            assert want == WANT[kind], (i, kind)
            self.sign[i] = (pk, sig, d, want)
        return self.sign[i]

    def dec_item(self, i):
        """(share, pk, ciphertext, oracle verdict) of check i: e(share, H_uv) == e(pk, W)"""
        if i not in self.dec:
            c, j, kind = i % NDOC, i % NKEY, KINDS[i % len(KINDS)]
            share, pk = cbls.g1_mul(self.U[c], self.sk[j]), self.pk[j]
            if kind == "wrong":
                share = cbls.g1_mul(self.U[c], (self.sk[j] + 1) % C.R)
            elif kind == "other_doc":
                share = cbls.g1_mul(self.U[(c + 1) % NDOC], self.sk[j])
            elif kind == "g2_inf":   # decrypt has no per-check G2 operand: the share at infinity
                share = O1
            elif kind == "g1_inf":
                pk = O1
            elif kind == "both_inf":
                share, pk = O1, O1
            want = int(cbls.pairing_eq(share, self.H[c], pk, self.W[c]))
            assert want == WANT[kind], (i, kind)
            self.dec[i] = (share, pk, c, want)
        return self.dec[i]


@pytest.fixture(scope="module")
def mat():
    return Material()


def both(engine, call):
    out = []
    try:
        for impl in (IMPL_PAIR, IMPL_WAVE, IMPL_QUAD, IMPL_OCT):
            engine.set_pairing_impl(impl)
            out.append(call())
    finally:
        engine.set_pairing_impl(IMPL_AUTO)
    return out


def expect_mixed(want, n):
    """the batch holds accepted and rejected checks once it is long enough to hold every kind"""
    if n >= len(KINDS):
        assert 0 < sum(want) < n


@pytest.mark.parametrize("n", SIZES)
def test_sign_shape(engine, mat, n):
    items = [mat.sign_item(i) for i in range(n)]
    pks, sigs, didx, want = (list(col) for col in zip(*items))
    pair, wave, quad, octo = both(engine, lambda: list(engine.verify_sig_shares(pks, sigs, mat.H, didx)))
    assert pair == want
    assert wave == want
    assert quad == want
    assert octo == want
    expect_mixed(want, n)


@pytest.mark.parametrize("n", SIZES)
def test_walk_both_sides(engine, mat, n):
    items = [mat.sign_item(i) for i in range(n)]
    pks, sigs, didx, want = (list(col) for col in zip(*items))
    hashes = [mat.H[d] for d in didx]
    pair, wave, quad, octo = both(engine, lambda: list(engine.verify_signatures(pks, sigs, hashes)))
    assert pair == want
    assert wave == want
    assert quad == want
    assert octo == want
    expect_mixed(want, n)


@pytest.mark.parametrize("n", SIZES)
def test_decrypt_shape(engine, mat, n):
    items = [mat.dec_item(i) for i in range(n)]
    shares, pks, cidx, want = (list(col) for col in zip(*items))
    pair, wave, quad, octo = both(engine, lambda: list(engine.verify_dec_shares(shares, pks, mat.H, mat.W, cidx)))
    assert pair == want
    assert wave == want
    assert quad == want
    assert octo == want
    expect_mixed(want, n)


def test_pairing_value_33(engine):
    """value_out set: PAIR, QUAD and OCT write WAVE's and the oracle's bytes (e(P, Q)^3) at 33 pairs;
    P = O and Q = O give 1, whose exponentiations all take the Granger-Scott path."""
    rng = random.Random(0x3333)
    P = [cbls.g1_mul(G1, rng.randrange(1, C.R)) for _ in range(33)]
    Q = [cbls.g2_mul(G2, rng.randrange(1, C.R)) for _ in range(33)]
    P[3], Q[5] = O1, O2
    P[32], Q[32] = O1, O2
    one = b"".join(c.to_bytes(48, "little") for six in C.F12_ONE for f2 in six for c in f2)
    want = [one if (p == O1 or q == O2) else cbls.pairing(p, q) for p, q in zip(P, Q)]
    pair, wave, quad, octo = both(engine, lambda: engine.dbg_pairing(P, Q))
    assert pair == wave
    assert pair == want
    assert quad == want
    assert octo == want
