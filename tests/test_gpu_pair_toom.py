"""HBH_IMPL_PAIR (the lane-pair kernel k_pair_verify) with the five-product Fp6 multiplication in its
Miller loop (csrc/pfp.hpp h6_mul6): the Miller value carries a power of 6, which the final
exponentiation removes, so every verdict byte and every byte of the pairing value is what it was.

Three shapes, through verify_pairing_eq_dev (which does not look at the indices on the host):
  sign     e(pk_i, H[d_i]) == e(g1, sigma_i)   shared H table, walked sigma, P2 the generator
  decrypt  e(s_i, Huv[c_i]) == e(pk_i, W[c_i])  two tables, both P read
  ctverify e(g1, W_i) == e(U_i, H_i)            both sides walked, P1 the generator
Sizes 1 (one lane pair), 2, 33 (a partial second wave) and 129 (the second workgroup holds one
check); below 4 checks per shared point (1, 2) the engine walks a shared side too.  Every batch
cycles through a valid check, a wrong share, a share for another document, a G2 and a G1 operand at
infinity and both (as test_gpu_pair_compressed.py has them); from 2 checks on, check 1 (valid
otherwise) names an index one past its table in a second run, and one far past it in a third: its
verdict must be 0 and every other one must stay.

Bar: the verdict bytes equal the C oracle's (oracle/cbls) and those of HBH_IMPL_QUAD, whose Miller
loop keeps the exact Karatsuba products; the canonical Fp12 value bytes, which the C ABI writes
through dbg_pairing (both sides walked, both P read), equal the oracle's at the same sizes.
"""
import random

import pytest
import torch

from oracle import bls12_381 as C
from oracle import cbls
from hbbft_amd._lib import IMPL_AUTO, IMPL_PAIR, IMPL_QUAD
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a
# the columns of verify_pairing_eq_dev on the device, and a call of it (check OOB_SLOT, valid there as
# here, names an index past its table when oob is set)
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
NKEY = 5
KINDS = ["valid", "valid", "wrong", "other_doc", "g2_inf", "g1_inf", "both_inf"]
WANT = {"valid": 1, "wrong": 0, "other_doc": 0, "g2_inf": 0, "g1_inf": 0, "both_inf": 1}
assert KINDS[OOB_SLOT] == "valid"  # a verdict of 0 there comes from the index alone
SHAPES = ["sign", "decrypt", "ctverify"]


def checked(batch):
    """the oracle's verdict for each kind is the one the kind is built to give"""
    assert list(batch.want) == [WANT[KINDS[i % len(KINDS)]] for i in range(len(batch.want))]
    return batch


def make_batches():
    rng = random.Random(0x746f6f6d)
    sk = [rng.randrange(1, R) for _ in range(NKEY)]
    pk = [cbls.g1_mul(G1, k) for k in sk]
    H = [cbls.g2_mul(G2, rng.randrange(1, R)) for _ in range(NDOC)]
    r = [rng.randrange(1, R) for _ in range(NDOC)]
    U = [cbls.g1_mul(G1, x) for x in r]
    W = [cbls.g2_mul(h, x) for h, x in zip(H, r)]
    kind = [KINDS[i % len(KINDS)] for i in range(NMAX)]
    doc = [i % NDOC for i in range(NMAX)]
    key = [i % NKEY for i in range(NMAX)]

    pks, sigs = [], []
    for i in range(NMAX):
        d, j = doc[i], key[i]
        p, s = pk[j], cbls.g2_mul(H[d], sk[j])
        if kind[i] == "wrong":
            s = cbls.g2_mul(H[d], (sk[j] + 1) % R)
        elif kind[i] == "other_doc":
            s = cbls.g2_mul(H[(d + 1) % NDOC], sk[j])
        elif kind[i] == "g2_inf":
            s = O2
        elif kind[i] == "g1_inf":
            p = O1
        elif kind[i] == "both_inf":
            p, s = O1, O2
        pks.append(p)
        sigs.append(s)
    sign = checked(Batch(pks, H, doc, None, sigs, None))

    shares, dpk = [], []
    for i in range(NMAX):
        c, j = doc[i], key[i]
        s, p = cbls.g1_mul(U[c], sk[j]), pk[j]
        if kind[i] == "wrong":
            s = cbls.g1_mul(U[c], (sk[j] + 1) % R)
        elif kind[i] == "other_doc":
            s = cbls.g1_mul(U[(c + 1) % NDOC], sk[j])
        elif kind[i] == "g2_inf":   # decrypt has no per-check G2 operand: the share at infinity
            s = O1
        elif kind[i] == "g1_inf":
            p = O1
        elif kind[i] == "both_inf":
            s, p = O1, O1
        shares.append(s)
        dpk.append(p)
    decrypt = checked(Batch(shares, H, doc, dpk, W, doc))

    # ctverify: a ciphertext per check; side 2 goes through an index map of its own points, which is
    # what lets a check name an index past them
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
    ctverify = checked(Batch(None, ws, None, us, hs, list(range(NMAX))))
    return {"sign": sign, "decrypt": decrypt, "ctverify": ctverify}


@pytest.fixture(scope="module")
def batches():
    return make_batches()


@pytest.fixture(scope="module")
def pairs():
    """NMAX pairs with the oracle's values, made once; P = O, Q = O and both among them"""
    rng = random.Random(0x76616c36)
    P = [cbls.g1_mul(G1, rng.randrange(1, R)) for _ in range(NMAX)]
    Q = [cbls.g2_mul(G2, rng.randrange(1, R)) for _ in range(NMAX)]
    P[1], Q[5], P[40], Q[128] = O1, O2, O1, O2
    P[9], Q[9] = O1, O2
    want = [ONE if (p == O1 or q == O2) else cbls.pairing(p, q) for p, q in zip(P, Q)]
    return P, Q, want


def with_impl(engine, impl, call):
    engine.set_pairing_impl(impl)
    try:
        return call()
    finally:
        engine.set_pairing_impl(IMPL_AUTO)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", SHAPES)
def test_verdicts(engine, batches, shape, n):
    b = batches[shape]
    for oob in (0, 1, 2) if n >= 2 else (0,):  # in range; == table size; far out of range
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
    assert list(with_impl(engine, IMPL_PAIR, lambda: engine.dbg_pairing(P, Q))) == want


def test_two_streams(engine, batches):
    """calls with different inputs in flight on two streams, as the benchmark runs them: each returns
    its own verdicts"""
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    a, b, c = batches["sign"], batches["decrypt"], batches["ctverify"]
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
