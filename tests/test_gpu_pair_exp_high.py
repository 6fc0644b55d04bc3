"""HBH_IMPL_PAIR (k_pair_verify) with t^105 of its exponentiation by x taken as (t^7)^15 with
conjugates for inverses (csrc/k_pair.hip h_exp_high).  h_exp_tail and h_exp_high are in every one of
the kernel's instantiations; tests/test_pair_exp_high_model.py has the chain over the oracle's Fp12,
here the kernel's bytes.

Three shapes, through verify_pairing_eq_dev (which does not look at the indices on the host):
  sign     e(pk_i, H[d_i]) == e(g1, sigma_i)   shared H table, walked sigma, P2 the generator
  decrypt  e(s_i, Huv[c_i]) == e(pk_i, W[c_i])  two tables, both P read
  ctverify e(g1, W_i) == e(U_i, H_i)            both sides walked, P1 the generator
Sizes 1, 2, 33 (a partial second wave) and 129 (one check in a second workgroup); below 4 checks per
shared point the engine walks a shared side too.  A batch cycles through a valid check, a wrong
share, a share for another document, a G2 and a G1 operand at infinity and both (f = 1 compresses
to zeros and takes the fallback loop, which does not go through h_exp_high); the secret keys include
1 and r - 1.  From 2 checks on, check 1 (valid otherwise) names the index one past its table in a
second run: its verdict must be 0 and every other one must stay.

Bar: verdict bytes equal the C oracle's (oracle/cbls) and HBH_IMPL_QUAD's, whose exponentiation is
the plain bit loop; the canonical Fp12 value bytes of dbg_pairing at the same four sizes equal the
oracle's and HBH_IMPL_QUAD's; two calls in flight on two streams return their own verdicts; the sign
and decrypt checks through a resident G2 set (hbh_g2_set_add) equal the oracle's under PAIR.
"""
import random

import pytest
import torch

from oracle import bls12_381 as C
from oracle import cbls
from hbbft_amd._lib import IMPL_AUTO, IMPL_PAIR, IMPL_QUAD
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a
from tests.test_gpu_pair_park import OOB_SLOT, Batch, enqueue, prepare, run

pytestmark = pytest.mark.gpu

R = C.R
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
O1, O2 = bytes(96), bytes(192)
ONE = b"".join(c.to_bytes(48, "little") for six in C.F12_ONE for f2 in six for c in f2)
SIZES = [1, 2, 33, 129]
NMAX = max(SIZES)
NDOC = 4
KINDS = ["valid", "valid", "wrong", "other_doc", "g2_inf", "g1_inf", "both_inf"]
WANT = {"valid": 1, "wrong": 0, "other_doc": 0, "g2_inf": 0, "g1_inf": 0, "both_inf": 1}
assert KINDS[OOB_SLOT] == "valid"  # a verdict of 0 there comes from the index alone
SHAPES = ["sign", "decrypt", "ctverify"]


def with_impl(engine, impl, call):
    engine.set_pairing_impl(impl)
    try:
        return call()
    finally:
        engine.set_pairing_impl(IMPL_AUTO)


class Inputs:
    def __init__(self):
        rng = random.Random(0x313035)
        self.sk = sk = [rng.randrange(1, R) for _ in range(3)] + [1, R - 1]
        self.pk = pk = [cbls.g1_mul(G1, k) for k in sk]
        self.H = H = [cbls.g2_mul(G2, rng.randrange(1, R)) for _ in range(NDOC - 1)] + [G2]
        r = [rng.randrange(1, R) for _ in range(NDOC)]
        U = [cbls.g1_mul(G1, x) for x in r]
        self.W = W = [cbls.g2_mul(h, x) for h, x in zip(H, r)]
        self.kind = kind = [KINDS[i % len(KINDS)] for i in range(NMAX)]
        self.doc = doc = [i % NDOC for i in range(NMAX)]
        key = [i % len(sk) for i in range(NMAX)]

        self.pks, self.sigs, self.shares, self.dpk = [], [], [], []
        for i in range(NMAX):
            d, j = doc[i], key[i]
            p, s = pk[j], cbls.g2_mul(H[d], sk[j])
            ds, dp = cbls.g1_mul(U[d], sk[j]), pk[j]
            if kind[i] == "wrong":
                s, ds = cbls.g2_mul(H[d], (sk[j] + 2) % R), cbls.g1_mul(U[d], (sk[j] + 2) % R)
            elif kind[i] == "other_doc":
                s, ds = cbls.g2_mul(H[(d + 1) % NDOC], sk[j]), cbls.g1_mul(U[(d + 1) % NDOC], sk[j])
            elif kind[i] == "g2_inf":   # decrypt has no per-check G2 operand: the share at infinity
                s, ds = O2, O1
            elif kind[i] == "g1_inf":
                p, dp = O1, O1
            elif kind[i] == "both_inf":
                p, s, ds, dp = O1, O2, O1, O1
            self.pks.append(p)
            self.sigs.append(s)
            self.shares.append(ds)
            self.dpk.append(dp)
        sign = Batch(self.pks, H, doc, None, self.sigs, None)
        decrypt = Batch(self.shares, H, doc, self.dpk, W, doc)

        ct = [(rng.randrange(1, R), cbls.g2_mul(G2, rng.randrange(1, R))) for _ in range(12)]
        ws, us, hs = [], [], []
        for i in range(NMAX):
            x, h = ct[i % 12]
            u, w = cbls.g1_mul(G1, x), cbls.g2_mul(h, x)
            if kind[i] == "wrong":
                w = cbls.g2_mul(h, (x + 1) % R)
            elif kind[i] == "other_doc":
                w = cbls.g2_mul(ct[(i + 1) % 12][1], x)
            elif kind[i] == "g2_inf":
                w = O2
            elif kind[i] == "g1_inf":
                u = O1
            elif kind[i] == "both_inf":
                u, w = O1, O2
            ws.append(w)
            us.append(u)
            hs.append(h)
        ctverify = Batch(None, ws, None, us, hs, list(range(NMAX)))
        self.batches = {"sign": sign, "decrypt": decrypt, "ctverify": ctverify}
        for b in self.batches.values():  # the oracle's verdict for each kind is the one it is built to give
            assert list(b.want) == [WANT[k] for k in kind]


@pytest.fixture(scope="module")
def inputs():
    return Inputs()


@pytest.fixture(scope="module")
def pairs():
    """NMAX pairs with the oracle's values, made once; small scalars, P = O, Q = O and both among them"""
    rng = random.Random(0x6c656166)
    small = [1, 2, 3, R - 1, R - 2]
    ks = small + [rng.randrange(1, R) for _ in range(NMAX - len(small))]
    js = [rng.randrange(1, R) for _ in range(NMAX - len(small))] + small
    P = [cbls.g1_mul(G1, j) for j in js]
    Q = [cbls.g2_mul(G2, k) for k in ks]
    P[6], Q[7], P[32], Q[128] = O1, O2, O1, O2
    P[40], Q[40] = O1, O2
    want = [ONE if (p == O1 or q == O2) else cbls.pairing(p, q) for p, q in zip(P, Q)]
    return P, Q, want


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", SHAPES)
def test_verdicts(engine, inputs, shape, n):
    b = inputs.batches[shape]
    for oob in (0, 1) if n >= 2 else (0,):  # in range; the index one past the table
        want = bytearray(b.want[:n])
        if oob:
            want[OOB_SLOT] = 0
        pair = with_impl(engine, IMPL_PAIR, lambda: run(engine, b, n, oob))
        quad = with_impl(engine, IMPL_QUAD, lambda: run(engine, b, n, oob))
        assert pair == bytes(want), oob
        assert pair == quad, oob
    if n >= len(KINDS):
        assert 0 < sum(b.want[:n]) < n


@pytest.mark.parametrize("n", SIZES)
def test_value_bytes(engine, pairs, n):
    P, Q, want = (col[:n] for col in pairs)
    pair = with_impl(engine, IMPL_PAIR, lambda: engine.dbg_pairing(P, Q))
    assert list(pair) == want
    assert list(with_impl(engine, IMPL_QUAD, lambda: engine.dbg_pairing(P, Q))) == list(pair)
    assert any(w != ONE for w in want)


def test_two_streams(engine, inputs):
    """calls with different inputs in flight on two streams, as the benchmark runs them: each returns
    its own verdicts"""
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    a, b, c = (inputs.batches[s] for s in SHAPES)
    pa, pb, pc = prepare(a, 129), prepare(b, 129, 1), prepare(c, 33)
    torch.cuda.synchronize()

    def go():
        va = enqueue(engine, sa.cuda_stream, pa)
        vb = enqueue(engine, sb.cuda_stream, pb)
        vc = enqueue(engine, sa.cuda_stream, pc)
        torch.cuda.synchronize()
        return va, vb, vc

    va, vb, vc = with_impl(engine, IMPL_PAIR, go)
    assert bytes(va.cpu().numpy()) == a.want[:129]
    want_b = bytearray(b.want[:129])
    want_b[OOB_SLOT] = 0
    assert bytes(vb.cpu().numpy()) == bytes(want_b)
    assert bytes(vc.cpu().numpy()) == c.want[:33]


@pytest.mark.parametrize("n", [2, 129])
def test_resident_g2_set(engine, inputs, n):
    """the sign and decrypt checks with their shared points prepared once into a resident set; the
    checks with no operand at infinity (a valid share, a wrong one, one for another document)"""
    keep = [i for i in range(n) if inputs.kind[i] in ("valid", "wrong", "other_doc")]
    col = lambda c: [c[i] for i in keep]
    gs = engine.g2_set(2 * NDOC)
    try:
        slots = gs.add(inputs.H + inputs.W)
        hi, wi = [slots[inputs.doc[i]] for i in keep], [slots[NDOC + inputs.doc[i]] for i in keep]
        sig = with_impl(engine, IMPL_PAIR,
                        lambda: engine.verify_sig_shares_set(col(inputs.pks), col(inputs.sigs), gs, hi))
        dec = with_impl(engine, IMPL_PAIR,
                        lambda: engine.verify_dec_shares_set(col(inputs.shares), col(inputs.dpk), gs, hi, wi))
    finally:
        gs.close()
    want = [WANT[inputs.kind[i]] for i in keep]
    assert list(sig) == want
    assert list(dec) == want
