"""HBH_IMPL_PAIR (the lane-pair kernel k_pair_verify) with its Miller-loop state parked in the lane's
column of the LDS stash (csrc/pfp.hpp PairPark): a walked side's T and a read side's P wait there
while f is squared and multiplied by the lines, and the stash is reused by the final exponentiation.

Three shapes, one per slot assignment of the park:
  sign     e(pk_i, H[d_i]) == e(g1, sigma_i)   shared H table, walked sigma, P2 the generator (T + P)
  decrypt  e(s_i, Huv[c_i]) == e(pk_i, W[c_i])  two tables, both P read                          (P + P)
  ctverify e(g1, W_i) == e(U_i, H_i)            both sides walked, P1 the generator              (T + P,
                                                the other T in registers)
Sizes 1, 2, 127, 128, 129, 257: a workgroup is 128 checks, so a lone pair, a full workgroup, one
check in a second workgroup and a ragged third one.  Below 4 checks per shared point (n = 1, 2) the
engine walks a shared side too.  Every batch cycles through a valid check, an invalid one, a P at
infinity, a walked Q at infinity and a table point at infinity; from n = 2 on, check 1 (valid
otherwise) names a Q index past its table, in a second run: its verdict must be 0 and every other
verdict must stay what it was.  The calls go through verify_pairing_eq_dev, which does not look at
the indices on the host.

Values: the C ABI writes the 144-word Fp12 value only through dbg_pairing (both sides walked, both P
read, the second pair masked out), so the value bytes are compared there, at the same sizes, with
P = O and Q = O among the pairs; the three shapes above are held to their verdict bytes.

Bar: bit-exact verdict bytes and bit-exact canonical Fp12 coefficients against the C oracle
(oracle/cbls).
"""
import functools
import random

import numpy as np
import pytest
import torch

from oracle import bls12_381 as C
from oracle import cbls
from hbbft_amd._lib import IMPL_AUTO, IMPL_PAIR
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a

pytestmark = pytest.mark.gpu

R = C.R
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
O1, O2 = bytes(96), bytes(192)
ONE = b"".join(c.to_bytes(48, "little") for six in C.F12_ONE for f2 in six for c in f2)
SIZES = [1, 2, 127, 128, 129, 257]
NMAX = max(SIZES)
NDOC = 4      # shared G2 points per call; the last one is the point at infinity
NKEY = 4     # kinds x points x keys repeat every 24 checks: a wave of 32 checks holds every combination
KINDS = ["valid", "valid", "invalid", "p_inf", "walk_q_inf", "table_inf", "valid", "invalid"]
OOB_SLOT = 1  # a valid check: a verdict of 0 there comes from the index alone
SHAPES = ["sign", "decrypt", "ctverify"]


def dev(b, dtype=torch.uint8):
    t = torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).to("cuda:0")
    return t if dtype == torch.uint8 else t.view(dtype)


@functools.lru_cache(maxsize=None)
def oracle_eq(p1, q1, p2, q2):
    return int(cbls.pairing_eq(p1, q1, p2, q2))


class Batch:
    """One shape's NMAX checks as the four columns of verify_pairing_eq_dev and the oracle's verdicts;
    a size takes a prefix.  p = None: the generator for every check; idx = None: one Q per check."""

    def __init__(self, p1, q1, idx1, p2, q2, idx2):
        self.p1, self.q1, self.idx1, self.p2, self.q2, self.idx2 = p1, q1, idx1, p2, q2, idx2
        n = len(q1) if idx1 is None else len(idx1)
        at = lambda q, idx, i: q[i] if idx is None else q[idx[i]]
        self.want = bytes(oracle_eq(G1 if p1 is None else p1[i], at(q1, idx1, i),
                                    G1 if p2 is None else p2[i], at(q2, idx2, i)) for i in range(n))


def make_batches():
    rng = random.Random(0x7061726b)
    sk = [rng.randrange(1, R) for _ in range(NKEY)]
    pk = [cbls.g1_mul(G1, k) for k in sk]
    H = [cbls.g2_mul(G2, rng.randrange(1, R)) for _ in range(NDOC - 1)] + [O2]
    r = [rng.randrange(1, R) for _ in range(NDOC)]
    U = [cbls.g1_mul(G1, x) for x in r]
    W = [O2 if h == O2 else cbls.g2_mul(h, x) for h, x in zip(H, r)]
    kind = [KINDS[i % len(KINDS)] for i in range(NMAX)]
    # the shared point of check i: the point at infinity for "table_inf" alone
    doc = [NDOC - 1 if kind[i] == "table_inf" else i % (NDOC - 1) for i in range(NMAX)]
    key = [i % NKEY for i in range(NMAX)]

    # sign: (pk, H[d]) against (g1, sigma)
    pks, sigs = [], []
    for i in range(NMAX):
        d, j = doc[i], key[i]
        p = O1 if kind[i] == "p_inf" else pk[j]
        s = cbls.g2_mul(H[d % (NDOC - 1)], sk[j])  # "table_inf": e(pk, O) = 1 against a sigma that is not O
        if kind[i] == "invalid":
            s = cbls.g2_mul(H[(d + 1) % (NDOC - 1)], sk[j])
        elif kind[i] == "walk_q_inf":
            s = O2
        pks.append(p)
        sigs.append(s)
    sign = Batch(pks, H, doc, None, sigs, None)

    # decrypt: (share, Huv[c]) against (pk, W[c]); no side walks once the tables are built
    shares, dpk = [], []
    for i in range(NMAX):
        c, j = doc[i], key[i]
        s, p = cbls.g1_mul(U[c], sk[j]), pk[j]
        if kind[i] == "invalid":
            p = pk[(j + 1) % NKEY]
        elif kind[i] == "p_inf":
            s = O1
        elif kind[i] == "walk_q_inf":
            s, p = O1, O1
        shares.append(s)
        dpk.append(p)
    decrypt = Batch(shares, H, doc, dpk, W, doc)

    # ctverify: (g1, W_i) against (U_i, H_i), a ciphertext per check; side 2 goes through an index map
    # of its own points (walked: a point per check), which is what lets a check name an index past it
    ct = [(rng.randrange(1, R), cbls.g2_mul(G2, rng.randrange(1, R))) for _ in range(24)]
    ws, us, hs = [], [], []
    for i in range(NMAX):
        x, h = ct[i % 24]
        u, w = cbls.g1_mul(G1, x), cbls.g2_mul(h, x)
        if kind[i] == "invalid":
            w = cbls.g2_mul(h, (x + 1) % R)
        elif kind[i] == "p_inf":
            u = O1
        elif kind[i] == "walk_q_inf":
            w = O2
        elif kind[i] == "table_inf":   # no table in this shape: the other walked point at infinity
            h = O2
        ws.append(w)
        us.append(u)
        hs.append(h)
    ctverify = Batch(None, ws, None, us, hs, list(range(NMAX)))
    return {"sign": sign, "decrypt": decrypt, "ctverify": ctverify}


@pytest.fixture(scope="module")
def batches():
    return make_batches()


@pytest.fixture(scope="module")
def pairs():
    """NMAX pairs with the oracle's values, made once; P = O, Q = O and both among the first two and
    in every later workgroup"""
    rng = random.Random(0x76616c)
    P = [cbls.g1_mul(G1, rng.randrange(1, R)) for _ in range(NMAX)]
    Q = [cbls.g2_mul(G2, rng.randrange(1, R)) for _ in range(NMAX)]
    for i in (1, 126, 130):
        P[i] = O1
    for i in (5, 127, 256):
        Q[i] = O2
    P[9], Q[9] = O1, O2
    want = [ONE if (p == O1 or q == O2) else cbls.pairing(p, q) for p, q in zip(P, Q)]
    return P, Q, want


def prepare(b, n, oob=0):
    """the first n checks of b on the device (oob: check OOB_SLOT names an index past its tables)"""
    def col(pts):
        return None if pts is None else dev(b"".join(pts))

    def idx(ix, table):
        if ix is None:
            return None
        ix = list(ix[:n])
        if oob:
            ix[OOB_SLOT] = table if oob == 1 else 1 << 30
        return dev(np.array(ix, dtype=np.uint32).tobytes(), torch.int32)

    q1 = b.q1[:n] if b.idx1 is None else b.q1
    q2 = b.q2[:n] if b.idx2 is None else b.q2
    cols = [col(b.p1[:n] if b.p1 else None), col(q1), idx(b.idx1, len(q1)),
            col(b.p2[:n] if b.p2 else None), col(q2), idx(b.idx2, len(q2))]
    d_v = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    return n, cols, len(q1), len(q2), d_v


def enqueue(engine, stream, prep):
    n, cols, nq1, nq2, d_v = prep
    ptr = [None if t is None else t.data_ptr() for t in cols]
    engine.verify_pairing_eq_dev(stream, n, ptr[0], ptr[1], nq1, ptr[2], ptr[3], ptr[4], nq2, ptr[5], d_v.data_ptr())
    return d_v


def run(engine, b, n, oob=0):
    prep = prepare(b, n, oob)
    torch.cuda.synchronize()  # the inputs were copied on torch's stream
    d_v = enqueue(engine, None, prep)
    torch.cuda.synchronize()
    return bytes(d_v.cpu().numpy())


@pytest.fixture()
def pair_engine(engine):
    engine.set_pairing_impl(IMPL_PAIR)
    try:
        yield engine
    finally:
        engine.set_pairing_impl(IMPL_AUTO)


def test_oracle_verdicts_by_kind(batches):
    """the oracle's verdict for each kind is the one the kind is built to give, in every shape"""
    for shape in SHAPES:
        got = {KINDS[i]: batches[shape].want[i] for i in (0, 2, 3, 4, 5)}
        assert got["valid"] == 1 and got["invalid"] == 0, shape
        assert got["p_inf"] == 0, shape
    assert batches["sign"].want[4] == 0 and batches["sign"].want[5] == 0   # one side 1, the other not
    assert batches["decrypt"].want[4] == 1 and batches["decrypt"].want[5] == 1  # both sides 1
    assert batches["ctverify"].want[4] == 0 and batches["ctverify"].want[5] == 0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", SHAPES)
def test_verdicts(pair_engine, batches, shape, n):
    b = batches[shape]
    got = run(pair_engine, b, n)
    assert got == b.want[:n]
    if n >= 2:
        want = bytearray(b.want[:n])
        want[OOB_SLOT] = 0
        for oob in (1, 2):  # == table size; far out of range
            assert run(pair_engine, b, n, oob) == bytes(want), oob


@pytest.mark.parametrize("n", SIZES)
def test_value_bytes(pair_engine, pairs, n):
    P, Q, want = (col[:n] for col in pairs)
    assert list(pair_engine.dbg_pairing(P, Q)) == want


def test_two_streams_back_to_back(pair_engine, batches):
    """two calls with different inputs in flight on two streams, as the benchmark runs them: each
    returns its own verdicts"""
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    a, b, c = batches["sign"], batches["decrypt"], batches["ctverify"]
    pa, pb, pc = prepare(a, 257), prepare(b, 129, 1), prepare(c, 129)
    torch.cuda.synchronize()
    va = enqueue(pair_engine, sa.cuda_stream, pa)
    vb = enqueue(pair_engine, sb.cuda_stream, pb)
    vc = enqueue(pair_engine, sa.cuda_stream, pc)
    torch.cuda.synchronize()
    assert bytes(va.cpu().numpy()) == a.want[:257]
    want_b = bytearray(b.want[:129])
    want_b[OOB_SLOT] = 0
    assert bytes(vb.cpu().numpy()) == bytes(want_b)
    assert bytes(vc.cpu().numpy()) == c.want[:129]
