"""The bucket form of the group sums (k_group_bucket through hbh_dbg_group_sums under a forced
HBH_GSUM_BUCKET): sum of r_i P_i per group, byte-equal to the C oracle and to the chain form.

One call holds groups of 1, 2, 3, GROUP_TILE - 1, GROUP_TILE, GROUP_TILE + 1, 2 GROUP_TILE + 5 and 64 items,
an absent table entry, the group {P, -P} with equal scalars (sum O), a group of 8 copies of one point
with one scalar (every nonzero digit makes a bucket take P + P, then 2P + P, ...), a group {P, -P} with
different scalars that share digits (a bucket takes P - P = O and goes on), a group of points at infinity
only, and a group in which every digit-boundary scalar of the host test (1, 2, 3, 2^64 - 1, 2^64, |x| - 1,
|x|, |x| + 1, |x|^2 - 1, |x|^2, 2^126, 3 * 2^126, 2^128 - 1) meets a finite point; the items are shuffled.
G1 sums are expected from cbls.g1_mul / g1_add; the G2 points are s_i H with known s_i, so a group's sum is
(sum r_i s_i mod r) H by cbls.g2_mul."""
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
SPECIAL = [1, 2, 3, (1 << 64) - 1, 1 << 64, X - 1, X, X + 1, X * X - 1, X * X, 1 << 126, 3 << 126, (1 << 128) - 1]
O1, O2 = bytes(96), bytes(192)


def neg_g1(p):
    y = int.from_bytes(p[48:], "little")
    return p[:48] + ((C.P - y) % C.P).to_bytes(48, "little")


def neg_g2(q):
    ys = [int.from_bytes(q[o:o + 48], "little") for o in (96, 144)]
    return q[:96] + b"".join(((C.P - y) % C.P).to_bytes(48, "little") for y in ys)


@pytest.fixture(scope="module")
def case():
    rng = random.Random(1701)
    T = _lib.GROUP_TILE
    # entry 3 is absent; 9: {P, -P}, equal scalars; 10: 8 copies; 11: {P, -P}, scalars sharing digits;
    # 12: infinity only; 13: the special scalars
    sizes = [1, 2, 3, 0, T - 1, T, T + 1, 2 * T + 5, 64, 2, 8, 2, 3, len(SPECIAL)]
    h = cbls.g2_mul(G2, rng.randrange(1, C.R))
    items = []  # (group, g1 point, g2 point, s (g2 point = s h), scalar)

    def point():
        a, s = rng.randrange(1, C.R), rng.randrange(1, C.R)
        return cbls.g1_mul(G1, a), cbls.g2_mul(h, s), s

    j = 0
    for k, size in enumerate(sizes[:9]):
        for _ in range(size):
            r = SPECIAL[(j // 7) % len(SPECIAL)] if j % 7 == 0 else rng.randrange(1, 1 << 128)
            if j % 11 == 5:
                items.append((k, O1, O2, 0, r))
            else:
                items.append((k,) + point() + (r,))
            j += 1
    p, q, s = point()
    r = rng.randrange(1, 1 << 128)
    items += [(9, p, q, s, r), (9, neg_g1(p), neg_g2(q), C.R - s, r)]
    p, q, s = point()
    r = rng.randrange(1 << 127, 1 << 128) | 0xe4e4  # digits 0, 1, 2, 3 all occur
    items += [(10, p, q, s, r)] * 8
    p, q, s = point()
    r = rng.randrange(1, 1 << 128)
    items += [(11, p, q, s, r), (11, neg_g1(p), neg_g2(q), C.R - s, r ^ (0xffff << 40) ^ (1 << 127))]
    items += [(12, O1, O2, 0, rng.randrange(1, 1 << 128)) for _ in range(3)]
    for r in SPECIAL:
        items.append((13,) + point() + (r,))
    assert [sum(1 for it in items if it[0] == k) for k in range(len(sizes))] == sizes
    rng.shuffle(items)
    want1, want2 = [O1] * len(sizes), [O2] * len(sizes)
    acc = [0] * len(sizes)
    for k, p1, _, s, r in items:
        want1[k] = cbls.g1_add(want1[k], cbls.g1_mul(p1, r))
        acc[k] = (acc[k] + r * s) % C.R
    for k in range(len(sizes)):
        if acc[k]:
            want2[k] = cbls.g2_mul(h, acc[k])
    return sizes, items, want1, want2


def sums(engine, impl, items, ngroups, g1=True, g2=True):
    engine.set_group_sum_impl(impl)
    try:
        return engine.dbg_group_sums([it[1] for it in items] if g1 else None, [it[2] for it in items] if g2 else None,
                                     ngroups, [it[0] for it in items], [it[4] for it in items])
    finally:
        engine.set_group_sum_impl(_lib.GSUM_AUTO)


def test_bucket_sums_match_oracle_and_chain(engine, case):
    sizes, items, want1, want2 = case
    got1, got2 = sums(engine, _lib.GSUM_BUCKET, items, len(sizes))
    assert got1 == want1
    assert got2 == want2
    for k in (3, 9, 12):  # absent entry, P - P, infinity only
        assert got1[k] == O1 and got2[k] == O2
    for k in (0, 7, 10, 11, 13):
        assert want1[k] != O1 and want2[k] != O2
    # the same bytes from either form
    assert sums(engine, _lib.GSUM_CHAIN, items, len(sizes)) == (got1, got2)


def test_bucket_sums_short_tiles(engine, case):
    """A call whose longest tile holds at most 64 items (the chain form then runs 64-slot workgroups; the
    bucket form stages a G1 tile in one round): the same sums."""
    sizes, items, want1, want2 = case
    small = [it for it in items if sizes[it[0]] <= 64]
    assert {it[0] for it in small} == {0, 1, 2, 8, 9, 10, 11, 12, 13}
    got1, got2 = sums(engine, _lib.GSUM_BUCKET, small, len(sizes))
    for k in range(len(sizes)):
        assert got1[k] == (want1[k] if sizes[k] <= 64 else O1)
        assert got2[k] == (want2[k] if sizes[k] <= 64 else O2)


def test_bucket_sums_one_side(engine, case):
    sizes, items, want1, want2 = case
    got1, none = sums(engine, _lib.GSUM_BUCKET, items, len(sizes), g2=False)
    assert none is None and got1 == want1
    none, got2 = sums(engine, _lib.GSUM_BUCKET, items, len(sizes), g1=False)
    assert none is None and got2 == want2
