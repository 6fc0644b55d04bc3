"""HBH_IMPL_PAIR (k_pair_verify) with the cyclotomic squarings of its final exponentiation on the
Fp4 squaring leaf (csrc/pfp.hpp h_sqr4_l: three unreduced lane-pair squares, two Montgomery
reductions).  Every one of the kernel's instantiations runs hc_sqr (285 times a check) and
h12_cyclo_sqr (36 times) on it; tests/test_pair_sqr4_model.py has the leaf over the oracle's
arithmetic and in limb form, here the kernel's bytes.

Three shapes, through verify_pairing_eq_dev (which does not look at the indices on the host):
  sign     e(pk_i, H[d_i]) == e(g1, sigma_i)   shared H table, walked sigma, P2 the generator
  decrypt  e(s_i, Huv[c_i]) == e(pk_i, W[c_i])  two tables, both P read
  ctverify e(g1, W_i) == e(U_i, H_i)            both sides walked, P1 the generator
Sizes 1, 2, 33 (a wave holds 32 checks) and 129 (a workgroup holds 128).  A batch cycles through
valid checks, a wrong share, a share for another document and operands at infinity; from 2 checks
on, check 1 (valid otherwise) names the index one past its table in a second run: its verdict must be
0 and every other one must stay.  The first two checks of a batch are valid ones, so sizes 1 and 2
run a second time with the wrong share in slot 0.

Bar: verdict bytes equal the C oracle's (oracle/cbls) and HBH_IMPL_QUAD's, whose squarings are the
lane quad's own (h12_cyclo_sqr_q, nine reduced squares); the canonical Fp12 value bytes of
dbg_pairing at the same sizes equal the oracle's.

The fallback: with P at infinity on both pairs the Miller value is 1, which compresses to four
zeros; a parked a1 is 0, the product of the denominators says so, and h_exp_gs runs the
Granger-Scott square-and-multiply loop -- on the leaf as well.  One case has checks with P at infinity
on one pair (f is the other pair's Miller value: the compressed path), on the other, and on both,
next to valid ones in the same wave; its verdicts are the oracle's, and so are the values of a
dbg_pairing batch whose pairs are mostly at infinity.
"""
import random

import pytest

from oracle import cbls
from hbbft_amd._lib import IMPL_AUTO, IMPL_PAIR, IMPL_QUAD
from tests.test_gpu_pair_exp_high import G1, G2, NDOC, O1, O2, ONE, R, SHAPES, SIZES, Inputs
from tests.test_gpu_pair_park import OOB_SLOT, Batch, run

pytestmark = pytest.mark.gpu

assert SIZES == [1, 2, 33, 129] and SHAPES == ["sign", "decrypt", "ctverify"]
NMAX = max(SIZES)


def with_impl(engine, impl, call):
    engine.set_pairing_impl(impl)
    try:
        return call()
    finally:
        engine.set_pairing_impl(IMPL_AUTO)


@pytest.fixture(scope="module")
def inputs():
    return Inputs()  # the oracle's verdicts are cached per check (test_gpu_pair_park.oracle_eq)


@pytest.fixture(scope="module")
def pairs():
    """NMAX pairs with the oracle's values, made once"""
    rng = random.Random(0x73717234)
    small = [1, 2, R - 1]
    ks = small + [rng.randrange(1, R) for _ in range(NMAX - len(small))]
    js = [rng.randrange(1, R) for _ in range(NMAX - len(small))] + small
    P = [cbls.g1_mul(G1, j) for j in js]
    Q = [cbls.g2_mul(G2, k) for k in ks]
    P[3], Q[4], P[31], Q[32], P[127], Q[128] = O1, O2, O1, O2, O1, O2
    P[64], Q[64] = O1, O2
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
    if n >= 33:
        assert 0 in b.want[:n] and 1 in b.want[:n]  # an invalid share is among them


def permuted(b, perm):
    """the checks perm of a batch, in that order (a shared table stays whole)"""
    pick = lambda col: None if col is None else [col[i] for i in perm]
    return Batch(pick(b.p1), b.q1 if b.idx1 is not None else pick(b.q1), pick(b.idx1),
                 pick(b.p2), b.q2 if b.idx2 is not None else pick(b.q2), pick(b.idx2))


@pytest.mark.parametrize("shape", SHAPES)
def test_small_sizes_with_an_invalid_share(engine, inputs, shape):
    """sizes 1 and 2 of the batches above are valid checks only: here the wrong share stands in slot 0
    and a valid check in slot 1, which names the index one past its table in a second run.  (One
    check cannot hold both: at size 1 it is the wrong share.)"""
    assert inputs.kind[2] == "wrong" and inputs.kind[0] == "valid" and OOB_SLOT == 1
    b = permuted(inputs.batches[shape], [2, 0])
    assert b.want == bytes([0, 1])
    for n, oob, want in ((1, 0, b"\0"), (2, 0, b"\0\1"), (2, 1, b"\0\0")):
        pair = with_impl(engine, IMPL_PAIR, lambda: run(engine, b, n, oob))
        assert pair == want, (n, oob)
        assert pair == with_impl(engine, IMPL_QUAD, lambda: run(engine, b, n, oob)), (n, oob)


@pytest.mark.parametrize("n", SIZES)
def test_value_bytes(engine, pairs, n):
    P, Q, want = (col[:n] for col in pairs)
    pair = with_impl(engine, IMPL_PAIR, lambda: engine.dbg_pairing(P, Q))
    assert list(pair) == want
    assert any(w != ONE for w in want)


def test_fallback_loop(engine, inputs, pairs):
    """f = 1: the Granger-Scott fallback of the exponentiation by x"""
    rng = random.Random(0x66616c6c)
    n = 33
    kinds = ["valid", "p1_inf", "both_inf", "p2_inf", "both_inf"]
    H = inputs.H
    r = [rng.randrange(1, R) for _ in range(NDOC)]
    U = [cbls.g1_mul(G1, x) for x in r]
    W = [cbls.g2_mul(h, x) for h, x in zip(H, r)]
    shares, dpk, doc = [], [], []
    for i in range(n):
        d, k = i % NDOC, inputs.sk[i % len(inputs.sk)]
        kind = kinds[i % len(kinds)]
        shares.append(O1 if kind in ("p1_inf", "both_inf") else cbls.g1_mul(U[d], k))
        dpk.append(O1 if kind in ("p2_inf", "both_inf") else cbls.g1_mul(G1, k))
        doc.append(d)
    b = Batch(shares, H, doc, dpk, W, doc)
    assert list(b.want) == [{"valid": 1, "p1_inf": 0, "p2_inf": 0, "both_inf": 1}[kinds[i % len(kinds)]] for i in range(n)]
    for m in (2, 3, n):  # both P at infinity alone behind a valid check; then a whole wave and one more
        pair = with_impl(engine, IMPL_PAIR, lambda: run(engine, b, m))
        assert pair == b.want[:m]
        assert pair == with_impl(engine, IMPL_QUAD, lambda: run(engine, b, m))
    # values: a wave of pairs at infinity (P, Q, both) around two that are not
    P0, Q0, want0 = pairs
    P, Q, want = [], [], []
    for i in range(n):
        if i in (5, 30):
            p, q, w = P0[i], Q0[i], want0[i]
        else:
            p, q = [(O1, Q0[0]), (P0[0], O2), (O1, O2)][i % 3]
            w = ONE
        P.append(p)
        Q.append(q)
        want.append(w)
    assert sum(w != ONE for w in want) == 2
    assert list(with_impl(engine, IMPL_PAIR, lambda: engine.dbg_pairing(P, Q))) == want
