"""The group sums behind the grouped share checks (k_group_sum / k_group_join through
hbh_dbg_group_sums): sum of r_i P_i per group, byte-equal to the C oracle.

One call holds groups of 1, 2, 3, GROUP_TILE - 1, GROUP_TILE, GROUP_TILE + 1 and 2 GROUP_TILE + 5 items
(one tile short of full, full, one item into a second tile, three tiles) and 64 items, an absent table
entry and a group {P, -P} with equal scalars (sum O), with the items shuffled.  Three two-item groups
meet the exceptional additions at the last tree level whatever the order: {P, P} with equal scalars
(P + P on equal coordinates), {aG, 2aG} with scalars {2 rho, rho} (distinct points, equal products: a
doubling of operands with different Z) and {aG, -2aG} with the same scalars (the scalars are 128-bit,
so the opposite product comes from the negated point: a cancellation of operands with different Z);
on G2 the same with s H.  test_group_sums_exceptional_pairs runs them alone under either form of the
sums.  Scalars: 1, 2, 2^64 - 1,
2^64, |x|, |x| + 1, |x|^2 - 1, |x|^2, 2^128 - 1 (the digit boundaries of the base-|x| split of the G2 sum)
and random 128-bit values; some points are at infinity.  G1 sums are expected from cbls.g1_mul / g1_add; the G2
points are s_i H with known s_i, so a group's sum is (sum r_i s_i mod r) H by cbls.g2_mul."""
import random

import pytest

from hbbft_amd import _lib
from oracle import bls12_381 as C
from oracle import cbls
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a

pytestmark = pytest.mark.gpu
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
X = 0xd201000000010000  # |x|, the BLS parameter
SPECIAL = [1, 2, (1 << 64) - 1, 1 << 64, X, X + 1, X * X - 1, X * X, (1 << 128) - 1]


def neg_g1(p):
    y = int.from_bytes(p[48:], "little")
    return p[:48] + ((C.P - y) % C.P).to_bytes(48, "little")


def neg_g2(q):
    ys = [int.from_bytes(q[o:o + 48], "little") for o in (96, 144)]
    return q[:96] + b"".join(((C.P - y) % C.P).to_bytes(48, "little") for y in ys)


@pytest.fixture(scope="module")
def case():
    rng = random.Random(1601)
    T = _lib.GROUP_TILE
    # entry 3 is absent; entry 9 is {P, -P}; 10: {P, P}; 11: {aG, 2aG} x {2 rho, rho}; 12: {aG, -2aG} x {2 rho, rho}
    sizes = [1, 2, 3, 0, T - 1, T, T + 1, 2 * T + 5, 64, 2, 2, 2, 2]
    h = cbls.g2_mul(G2, rng.randrange(1, C.R))
    items = []  # (group, g1 point, g2 point, s (g2 point = s h), scalar)
    j = 0
    for k, size in enumerate(sizes[:9]):
        for _ in range(size):
            r = SPECIAL[(j // 7) % len(SPECIAL)] if j % 7 == 0 else rng.randrange(1, 1 << 128)
            if j % 11 == 5:
                items.append((k, bytes(96), bytes(192), 0, r))
            else:
                a, s = rng.randrange(1, C.R), rng.randrange(1, C.R)
                items.append((k, cbls.g1_mul(G1, a), cbls.g2_mul(h, s), s, r))
            j += 1
    a, s, r = rng.randrange(1, C.R), rng.randrange(1, C.R), rng.randrange(1, 1 << 128)
    p, q = cbls.g1_mul(G1, a), cbls.g2_mul(h, s)
    items += [(9, p, q, s, r), (9, neg_g1(p), neg_g2(q), C.R - s, r)]
    a10, s, r10 = rng.randrange(1, C.R), rng.randrange(1, C.R), rng.randrange(1, 1 << 128)
    p, q = cbls.g1_mul(G1, a10), cbls.g2_mul(h, s)
    items += [(10, p, q, s, r10), (10, p, q, s, r10)]
    a, s, rho = rng.randrange(1, C.R), rng.randrange(1, C.R), rng.randrange(1, 1 << 100)
    p, q = cbls.g1_mul(G1, a), cbls.g2_mul(h, s)
    p2, q2 = cbls.g1_mul(G1, 2 * a % C.R), cbls.g2_mul(h, 2 * s % C.R)
    assert p2 != p and cbls.g1_mul(p, 2 * rho) == cbls.g1_mul(p2, rho)
    items += [(11, p, q, s, 2 * rho), (11, p2, q2, 2 * s % C.R, rho)]
    items += [(12, p, q, s, 2 * rho), (12, neg_g1(p2), neg_g2(q2), C.R - 2 * s % C.R, rho)]
    # every special scalar meets a finite point
    assert {r for _, p1, _, _, r in items if p1 != bytes(96)} >= set(SPECIAL)
    rng.shuffle(items)
    want1, want2 = [bytes(96)] * len(sizes), [bytes(192)] * len(sizes)
    acc = [0] * len(sizes)
    for k, p1, _, s, r in items:
        want1[k] = cbls.g1_add(want1[k], cbls.g1_mul(p1, r))
        acc[k] = (acc[k] + r * s) % C.R
    for k in range(len(sizes)):
        if acc[k]:
            want2[k] = cbls.g2_mul(h, acc[k])
    # the G1 sums of the doubling groups from their scalars: 2 r P and 4 rho a G
    assert want1[10] == cbls.g1_mul(G1, 2 * r10 * a10 % C.R) and want1[11] == cbls.g1_mul(G1, 4 * rho * a % C.R)
    return sizes, items, want1, want2


def test_group_sums_match_oracle(engine, case):
    sizes, items, want1, want2 = case
    got1, got2 = engine.dbg_group_sums([it[1] for it in items], [it[2] for it in items], len(sizes),
                                       [it[0] for it in items], [it[4] for it in items])
    assert got1 == want1
    assert got2 == want2
    assert got1[3] == bytes(96) and got2[3] == bytes(192)  # absent entry
    assert got1[9] == bytes(96) and got2[9] == bytes(192)  # P - P = O
    assert want1[0] != bytes(96) and want2[7] != bytes(192)
    assert got1[12] == bytes(96) and got2[12] == bytes(192)  # 2 rho aG - rho 2aG = O
    assert bytes(96) not in (got1[10], got1[11]) and bytes(192) not in (got2[10], got2[11])


@pytest.mark.parametrize("impl", [_lib.GSUM_CHAIN, _lib.GSUM_BUCKET])
def test_group_sums_exceptional_pairs(engine, case, impl):
    """The groups {P, -P}, {P, P}, {aG, 2aG} and {aG, -2aG} alone, under the chain and the bucket form."""
    sizes, items, want1, want2 = case
    pairs = [it for it in items if it[0] >= 9]
    assert len(pairs) == 8
    engine.set_group_sum_impl(impl)
    try:
        got1, got2 = engine.dbg_group_sums([it[1] for it in pairs], [it[2] for it in pairs], len(sizes),
                                           [it[0] for it in pairs], [it[4] for it in pairs])
    finally:
        engine.set_group_sum_impl(_lib.GSUM_AUTO)
    assert got1[9:] == want1[9:] and got2[9:] == want2[9:]
    assert got1[:9] == [bytes(96)] * 9 and got2[:9] == [bytes(192)] * 9
    assert want1[9] == want1[12] == bytes(96) and want2[9] == want2[12] == bytes(192)


def test_group_sums_short_tiles(engine, case):
    """A call whose longest tile holds at most 64 items runs 64-slot workgroups (the first call above,
    with tiles of GROUP_TILE items, runs GROUP_TILE-slot ones): the same sums."""
    sizes, items, want1, want2 = case
    small = [it for it in items if sizes[it[0]] <= 64]
    assert {it[0] for it in small} == {0, 1, 2, 8, 9, 10, 11, 12}
    got1, got2 = engine.dbg_group_sums([it[1] for it in small], [it[2] for it in small], len(sizes),
                                       [it[0] for it in small], [it[4] for it in small])
    for k in range(len(sizes)):
        assert got1[k] == (want1[k] if sizes[k] <= 64 else bytes(96))
        assert got2[k] == (want2[k] if sizes[k] <= 64 else bytes(192))


def test_group_sums_one_side_and_errors(engine, case):
    sizes, items, want1, want2 = case
    idx, rs = [it[0] for it in items], [it[4] for it in items]
    got1, none = engine.dbg_group_sums([it[1] for it in items], None, len(sizes), idx, rs)
    assert none is None and got1 == want1
    none, got2 = engine.dbg_group_sums(None, [it[2] for it in items], len(sizes), idx, rs)
    assert none is None and got2 == want2
    assert engine.dbg_group_sums([], [], 3, [], []) == ([bytes(96)] * 3, [bytes(192)] * 3)
    with pytest.raises(_lib.HbhError):
        engine.dbg_group_sums([items[0][1]], None, 2, [2], [1])  # group index past the table
