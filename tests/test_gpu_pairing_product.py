"""The Miller-product kernel of the batched checks (pair_side.hpp lane_miller_prod) through
hbh_dbg_pairing_product: out[g] = (prod of e(P_i, Q_i) over group g)^3, one group per 256 items, against
the oracle's pairings multiplied in Python (oracle/bls12_381.py f12_mul) -- byte for byte.

Sizes, per forced width W with T = 256 (PAIR), 128 (QUAD), 64 (OCT) items per tile: 1, 2, 3 (an odd last
slot), T - 1, T, T + 1 (a second tile, or for PAIR a second group of one item), and for PAIR 257.
Inactive pairs (P = O or Q = O) at the first slot's two sides, the last item and a whole wave in the
middle contribute 1; a tile of inactive pairs only gives 1."""
import random

import pytest

from hbbft_amd._lib import BATCH_GROUP, IMPL_AUTO, IMPL_OCT, IMPL_PAIR, IMPL_QUAD
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a
from oracle import bls12_381 as C
from oracle import cbls

pytestmark = pytest.mark.gpu

G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
O1, O2 = bytes(96), bytes(192)
WIDTHS = {IMPL_PAIR: 256, IMPL_QUAD: 128, IMPL_OCT: 64}  # items per tile
LANES = {IMPL_PAIR: 2, IMPL_QUAD: 4, IMPL_OCT: 8}
NMAX = 257
assert BATCH_GROUP == 256


def f12_of(raw):
    c = [int.from_bytes(raw[48 * k:48 * k + 48], "little") for k in range(12)]
    return tuple(tuple((c[6 * h + 2 * j], c[6 * h + 2 * j + 1]) for j in range(3)) for h in range(2))


def raw_of(f):
    return b"".join(c.to_bytes(48, "little") for six in f for f2 in six for c in f2)


ONE = raw_of(C.F12_ONE)


def cube(f):
    return C.f12_mul(C.f12_mul(f, f), f)


def want_groups(vals):
    """vals: e(P_i, Q_i) per item (Fp12 tuples; F12_ONE for an inactive pair) -> the 576-byte values"""
    out = []
    for g in range(0, len(vals), BATCH_GROUP):
        acc = C.F12_ONE
        for f in vals[g:g + BATCH_GROUP]:
            acc = C.f12_mul(acc, f)
        out.append(raw_of(cube(acc)))
    return out


def with_impl(engine, impl, call):
    engine.set_pairing_impl(impl)
    try:
        return call()
    finally:
        engine.set_pairing_impl(IMPL_AUTO)


@pytest.fixture(scope="module")
def pairs():
    """NMAX pairs, made once, with the C oracle's value of each: cbls.pairing gives e(P, Q)^3 (the
    format of dbg_pairing), and (prod e_i)^3 = prod e_i^3, so the expected value of a group is the
    product of these (test_oracle_value_is_the_cube ties it to the pure-Python pairing, cubed)."""
    rng = random.Random(0x6d70726f)
    js = [1, 2, C.R - 1] + [rng.randrange(1, C.R) for _ in range(NMAX - 3)]
    ks = [rng.randrange(1, C.R) for _ in range(NMAX - 3)] + [C.R - 1, 2, 1]
    P = [cbls.g1_mul(G1, j) for j in js]
    Q = [cbls.g2_mul(G2, k) for k in ks]
    e3 = [f12_of(cbls.pairing(p, q)) for p, q in zip(P, Q)]  # cbls.pairing: e(P, Q)^3, dbg_pairing's value
    return P, Q, e3


def want_from_cubes(e3):
    """(prod e_i)^3 = prod e_i^3 per group"""
    out = []
    for g in range(0, len(e3), BATCH_GROUP):
        acc = C.F12_ONE
        for f in e3[g:g + BATCH_GROUP]:
            acc = C.f12_mul(acc, f)
        out.append(raw_of(acc))
    return out


def test_oracle_value_is_the_cube(pairs):
    """cbls.pairing is e^3 in dbg_pairing's format: the pure-Python pairing of one pair, cubed"""
    P, Q, e3 = pairs
    p = C.g1_mul(C.G1_GEN, 2)
    q = C.g2_mul(C.G2_GEN, C.R - 1)
    assert (P[1], Q[NMAX - 3]) == (g1a(C.g1_uncompressed(p)), g2a(C.g2_uncompressed(q)))
    assert raw_of(cube(C.pairing(p, q))) == cbls.pairing(P[1], Q[NMAX - 3])
    assert want_groups([C.pairing(p, q)]) == want_from_cubes([f12_of(cbls.pairing(P[1], Q[NMAX - 3]))])


def sizes(impl):
    t = WIDTHS[impl]
    return sorted({1, 2, 3, t - 1, t, t + 1} | ({257} if impl == IMPL_PAIR else set()))


@pytest.mark.parametrize("impl, n", [(impl, n) for impl in WIDTHS for n in sizes(impl)])
def test_product_values(engine, pairs, impl, n):
    P, Q, e3 = (col[:n] for col in pairs)
    want = want_from_cubes(e3)
    assert len(want) == (2 if n > BATCH_GROUP else 1)
    got = with_impl(engine, impl, lambda: engine.dbg_pairing_product(P, Q))
    assert got == want
    assert all(w != ONE for w in want)


@pytest.mark.parametrize("impl", list(WIDTHS))
def test_mostly_inactive(engine, pairs, impl):
    P0, Q0, e30 = pairs
    t = WIDTHS[impl]
    wave = 2 * 64 // LANES[impl]  # items of one wave
    P, Q, e3 = list(P0[:t]), list(Q0[:t]), list(e30[:t])
    dead = {0: "p", 1: "q", t - 1: "pq"}
    dead.update({i: "pqb"[i % 3] for i in range(wave, 2 * wave)})  # the second wave, whole
    for i, kind in dead.items():
        if kind in ("p", "b"):
            P[i] = O1
        if kind in ("q", "b"):
            Q[i] = O2
        if kind == "pq":
            P[i], Q[i] = O1, O2
        e3[i] = C.F12_ONE
    assert 2 * wave < t - 1 and len(dead) == wave + 3
    want = want_from_cubes(e3)
    assert with_impl(engine, impl, lambda: engine.dbg_pairing_product(P, Q)) == want
    assert want != want_from_cubes(e30[:t]) and want != [ONE]


@pytest.mark.parametrize("impl", list(WIDTHS))
def test_all_inactive(engine, pairs, impl):
    P0, Q0, _ = pairs
    t = WIDTHS[impl]
    P = [O1 if i % 3 != 1 else P0[i] for i in range(t)]
    Q = [O2 if i % 3 != 0 else Q0[i] for i in range(t)]
    assert all(p == O1 or q == O2 for p, q in zip(P, Q)) and any(p != O1 for p in P) and any(q != O2 for q in Q)
    assert with_impl(engine, impl, lambda: engine.dbg_pairing_product(P, Q)) == [ONE]


def test_auto_and_empty(engine, pairs):
    P, Q, e3 = (col[:5] for col in pairs)
    assert engine.dbg_pairing_product(P, Q) == want_from_cubes(e3)
    assert engine.dbg_pairing_product([], []) == []
