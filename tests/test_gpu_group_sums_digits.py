"""The group sums under the digit forms of the scalars (k_group_digits / k_group_join through
hbh_dbg_group_sums_form): sum of r_i P_i per group with r_i read as X4 digits (both groups) or X2 digits
(G1), byte-equal to the C oracle.

The call's shape is that of test_gpu_group_sums.py: groups of 1, 2, 3, GROUP_TILE - 1, GROUP_TILE,
GROUP_TILE + 1, 2 GROUP_TILE + 5 and 64 items, an absent table entry, the items shuffled, some points at
infinity, and the two-item groups {P, -P} and {P, P} with equal scalars, {aG, 2aG} x {2 rho, rho} (equal
products from distinct points: a doubling at the tree) and {aG, -2aG} x {2 rho, rho} (a cancellation); rho's
digits are below 2^31, so 2 rho is the tuple of the doubled digits.  Digit tuples: every digit in
{0, 1, max} in all combinations (the all-zero tuple included: it contributes O), a single mid-valued digit in
each position and leading-zero high digits, each meeting a finite point, and random tuples for the rest.
G1 sums are expected from cbls.g1_mul / g1_add with the integer r_i; the G2 points are s_i H with known
s_i, so a group's sum is (sum r_i s_i mod r) H by cbls.g2_mul."""
import itertools
import random

import pytest

from hbbft_amd import _lib
from hbbft_amd._lib import GFORM_INT128, GFORM_X2, GFORM_X4
from hbbft_amd.engine import digit_scalar, g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a
from oracle import bls12_381 as C
from oracle import cbls

pytestmark = pytest.mark.gpu
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
O1, O2 = bytes(96), bytes(192)


def neg_g1(p):
    y = int.from_bytes(p[48:], "little")
    return p[:48] + ((C.P - y) % C.P).to_bytes(48, "little")


def neg_g2(q):
    ys = [int.from_bytes(q[o:o + 48], "little") for o in (96, 144)]
    return q[:96] + b"".join(((C.P - y) % C.P).to_bytes(48, "little") for y in ys)


def edge_tuples(form):
    nd, top = (4, 2 ** 32 - 1) if form == GFORM_X4 else (2, 2 ** 64 - 1)
    out = [list(t) for t in itertools.product((0, 1, top), repeat=nd)]
    for j in range(nd):
        for v in (2, (top + 1) // 2, 0x12345678):
            out.append([v if k == j else 0 for k in range(nd)])
    rng = random.Random(2203)
    for lead in range(1, nd):  # leading-zero high digits
        out.append([rng.randrange(1, top + 1) if k < lead else 0 for k in range(nd)])
    return out


def build(form, seed):
    rng = random.Random(seed)
    T = _lib.GROUP_TILE
    nd, bits = (4, 32) if form == GFORM_X4 else (2, 64)
    # entry 3 is absent; entry 9 is {P, -P}; 10: {P, P}; 11: {aG, 2aG} x {2 rho, rho}; 12: {aG, -2aG} x {2 rho, rho}
    sizes = [1, 2, 3, 0, T - 1, T, T + 1, 2 * T + 5, 64, 2, 2, 2, 2]
    h = cbls.g2_mul(G2, rng.randrange(1, C.R))
    edges = edge_tuples(form)
    items = []  # (group, g1 point, g2 point, s (g2 point = s h), digits)
    j = 0
    for k, size in enumerate(sizes[:9]):
        for _ in range(size):
            if j % 11 == 5:
                items.append((k, O1, O2, 0, [rng.randrange(1 << bits) for _ in range(nd)]))
            else:
                dg = edges.pop() if edges and j % 3 != 1 else [rng.randrange(1 << bits) for _ in range(nd)]
                a, s = rng.randrange(1, C.R), rng.randrange(1, C.R)
                items.append((k, cbls.g1_mul(G1, a), cbls.g2_mul(h, s), s, dg))
            j += 1
    assert not edges  # every edge tuple met a finite point
    rand = lambda hi: [rng.randrange(hi) for _ in range(nd)]  # noqa: E731
    a, s, dg = rng.randrange(1, C.R), rng.randrange(1, C.R), rand(1 << bits)
    p, q = cbls.g1_mul(G1, a), cbls.g2_mul(h, s)
    items += [(9, p, q, s, dg), (9, neg_g1(p), neg_g2(q), C.R - s, dg)]
    a, s, dg = rng.randrange(1, C.R), rng.randrange(1, C.R), rand(1 << bits)
    p, q = cbls.g1_mul(G1, a), cbls.g2_mul(h, s)
    items += [(10, p, q, s, dg), (10, p, q, s, dg)]
    a, s, rho = rng.randrange(1, C.R), rng.randrange(1, C.R), [rng.randrange(1, 1 << (bits - 1)) for _ in range(nd)]
    rho2 = [2 * d for d in rho]
    assert digit_scalar(form, rho2)[1] == 2 * digit_scalar(form, rho)[1]
    p, q = cbls.g1_mul(G1, a), cbls.g2_mul(h, s)
    p2, q2 = cbls.g1_mul(G1, 2 * a % C.R), cbls.g2_mul(h, 2 * s % C.R)
    items += [(11, p, q, s, rho2), (11, p2, q2, 2 * s % C.R, rho)]
    items += [(12, p, q, s, rho2), (12, neg_g1(p2), neg_g2(q2), C.R - 2 * s % C.R, rho)]
    rng.shuffle(items)
    want1, want2 = [O1] * len(sizes), [O2] * len(sizes)
    acc = [0] * len(sizes)
    for k, p1, _, s, dg in items:
        r = digit_scalar(form, dg)[1]
        assert r < C.R
        want1[k] = cbls.g1_add(want1[k], cbls.g1_mul(p1, r)) if r else want1[k]
        acc[k] = (acc[k] + r * s) % C.R
    for k in range(len(sizes)):
        if acc[k]:
            want2[k] = cbls.g2_mul(h, acc[k])
    assert want1[9] == want1[12] == O1 and O1 not in (want1[10], want1[11])
    return sizes, items, want1, want2


@pytest.fixture(scope="module")
def case4():
    return build(GFORM_X4, 2204)


@pytest.fixture(scope="module")
def case2():
    return build(GFORM_X2, 2205)


def sums(engine, form, items, ngroups, g1=True, g2=True):
    return engine.dbg_group_sums_form(form, [it[1] for it in items] if g1 else None, [it[2] for it in items] if g2 else None,
                                      ngroups, [it[0] for it in items], [digit_scalar(form, it[4])[0] for it in items])


def test_x4_sums_match_oracle(engine, case4):
    sizes, items, want1, want2 = case4
    got1, got2 = sums(engine, GFORM_X4, items, len(sizes))
    assert got1 == want1
    assert got2 == want2
    assert got1[3] == O1 and got2[3] == O2  # absent entry
    assert got1[9] == O1 and got2[9] == O2  # P - P = O
    assert got1[12] == O1 and got2[12] == O2  # 2 rho aG - rho 2aG = O
    assert O1 not in (got1[0], got1[10], got1[11]) and O2 not in (got2[7], got2[10], got2[11])


def test_x2_sums_match_oracle(engine, case2):
    sizes, items, want1, _ = case2
    got1, none = sums(engine, GFORM_X2, items, len(sizes), g2=False)
    assert none is None and got1 == want1
    assert got1[3] == got1[9] == got1[12] == O1 and O1 not in (got1[0], got1[10], got1[11])


def test_short_tiles(engine, case4, case2):
    """A call whose longest tile holds at most 64 items runs 64-slot workgroups: the same sums."""
    for form, (sizes, items, want1, want2) in ((GFORM_X4, case4), (GFORM_X2, case2)):
        small = [it for it in items if sizes[it[0]] <= 64]
        assert {it[0] for it in small} == {0, 1, 2, 8, 9, 10, 11, 12}
        got1, got2 = sums(engine, form, small, len(sizes), g2=form == GFORM_X4)
        for k in range(len(sizes)):
            assert got1[k] == (want1[k] if sizes[k] <= 64 else O1)
            if form == GFORM_X4:
                assert got2[k] == (want2[k] if sizes[k] <= 64 else O2)


def test_one_sided_calls_and_errors(engine, case4):
    sizes, items, want1, want2 = case4
    got1, none = sums(engine, GFORM_X4, items, len(sizes), g2=False)
    assert none is None and got1 == want1
    none, got2 = sums(engine, GFORM_X4, items, len(sizes), g1=False)
    assert none is None and got2 == want2
    assert engine.dbg_group_sums_form(GFORM_X4, [], [], 3, [], []) == ([O1] * 3, [O2] * 3)
    one = items[0]
    with pytest.raises(_lib.HbhError):  # no call sums G2 points under X2
        engine.dbg_group_sums_form(GFORM_X2, [one[1]], [one[2]], 2, [0], [1])
    with pytest.raises(_lib.HbhError):
        engine.dbg_group_sums_form(GFORM_X2, None, [one[2]], 2, [0], [1])
    with pytest.raises(_lib.HbhError):  # unknown form
        engine.dbg_group_sums_form(3, [one[1]], None, 2, [0], [1])
    with pytest.raises(_lib.HbhError):  # group index past the table
        engine.dbg_group_sums_form(GFORM_X4, [one[1]], None, 2, [2], [1])
    assert engine.dbg_group_sums_form(GFORM_X2, [G1], None, 1, [0], [1]) == ([G1], None)  # still works


def test_int128_form_is_dbg_group_sums(engine, case4):
    sizes, items, _, _ = case4
    rng = random.Random(2206)
    sub = items[:200]
    args = ([it[1] for it in sub], [it[2] for it in sub], len(sizes), [it[0] for it in sub],
            [rng.randrange(1, 1 << 128) for _ in sub])
    assert engine.dbg_group_sums_form(GFORM_INT128, *args) == engine.dbg_group_sums(*args)
    # the same bytes read as X4 digits are another residue: the form decides
    assert engine.dbg_group_sums_form(GFORM_X4, *args) != engine.dbg_group_sums(*args)
