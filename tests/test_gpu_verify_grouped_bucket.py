"""The grouped share checks with the bucket form of their group sums (hbh_engine_set_group_sum_impl,
HBH_GSUM_BUCKET): signature and decryption shares, 8 groups of 12 plus two singles.  The verdicts must
equal the per-share call's in every case, the statistics say which path each item took, and with
supplied scalars they are field for field the chain form's.  Every test restores HBH_GSUM_AUTO."""
import contextlib
import random

import pytest

from hbbft_amd import _lib
from hbbft_amd._lib import HbhError
from oracle import bls12_381 as C
from oracle import cbls
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a

pytestmark = pytest.mark.gpu
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
NODES = 16
SIZES = [12] * 8 + [1, 1]  # 98 items; entries 8 and 9 hold one item each
N = sum(SIZES)


@contextlib.contextmanager
def forced(engine, impl):
    engine.set_group_sum_impl(impl)
    try:
        yield
    finally:
        engine.set_group_sum_impl(_lib.GSUM_AUTO)


@pytest.fixture(scope="module")
def keys():
    rng = random.Random(1702)
    sks = [rng.randrange(1, C.R) for _ in range(NODES)]
    return sks, [cbls.g1_mul(G1, sk) for sk in sks]


@pytest.fixture(scope="module")
def sig_case(keys):
    """rows[d] = the items (pk, sig, doc, valid, node) of document d, all valid; the documents' hashes."""
    sks, pks = keys
    rng = random.Random(1703)
    hs = [cbls.g2_mul(G2, rng.randrange(1, C.R)) for _ in SIZES]
    rows = [[(pks[i], cbls.g2_mul(hs[d], sks[i]), d, 1, i) for i in rng.sample(range(NODES), size)]
            for d, size in enumerate(SIZES)]
    return hs, rows


@pytest.fixture(scope="module")
def dec_case(keys):
    """rows[c] = the items (share, pk, ct, valid, node) of ciphertext c; (U, H_uv, W) per ciphertext with
    U = r g1, W = r H_uv, so that e(sk U, H_uv) == e(sk g1, W)."""
    sks, pks = keys
    rng = random.Random(1704)
    cts = []
    for _ in SIZES:
        r, huv = rng.randrange(1, C.R), cbls.g2_mul(G2, rng.randrange(1, C.R))
        cts.append((cbls.g1_mul(G1, r), huv, cbls.g2_mul(huv, r)))
    rows = [[(cbls.g1_mul(cts[c][0], sks[i]), pks[i], c, 1, i) for i in rng.sample(range(NODES), size)]
            for c, size in enumerate(SIZES)]
    return cts, rows


def spoil(rng, rows, groups, make):
    """One item of each named group becomes invalid: make(group, item) -> its replacement point."""
    rows = [list(row) for row in rows]
    for g in groups:
        pos = rng.randrange(len(rows[g]))
        it = rows[g][pos]
        rows[g][pos] = make(g, it) + (g, 0, it[4])
    return rows


def flat(rng, rows):
    items = [it for row in rows for it in row]
    rng.shuffle(items)
    return items


def run_sig(engine, hs, items, scalars=None):
    args = ([it[0] for it in items], [it[1] for it in items], hs, [it[2] for it in items])
    return engine.verify_sig_shares_grouped(*args, scalars=scalars), engine.verify_sig_shares(*args)


def run_dec(engine, cts, items, scalars=None):
    args = ([it[0] for it in items], [it[1] for it in items], [c[1] for c in cts], [c[2] for c in cts],
            [it[2] for it in items])
    return engine.verify_dec_shares_grouped(*args, scalars=scalars), engine.verify_dec_shares(*args)


def bad_sig(keys, hs):
    """Document d's invalid share: the node's share of another document (odd d), the point at infinity
    (d = 0, 4, 8) or an unrelated point."""
    sks, _ = keys

    def make(d, it):
        if d % 2:
            return it[0], cbls.g2_mul(hs[(d + 1) % len(hs)], sks[it[4]])
        return it[0], bytes(192) if d % 4 == 0 else cbls.g2_mul(G2, 1000 + d)
    return make


def bad_dec(keys, cts):
    """Ciphertext c's invalid share: another node's share (odd c), the point at infinity (c = 0, 4, 8) or an
    unrelated point."""
    sks, _ = keys

    def make(c, it):
        if c % 2:
            return cbls.g1_mul(cts[c][0], sks[(it[4] + 1) % NODES]), it[1]
        return bytes(96) if c % 4 == 0 else cbls.g1_mul(G1, 2000 + c), it[1]
    return make


def test_sig_mixed_all_valid_all_failing(engine, keys, sig_case):
    hs, rows = sig_case
    rng = random.Random(1705)
    with forced(engine, _lib.GSUM_BUCKET):
        # mixed: groups 1, 2, 4, 7 and single 9 hold an invalid share
        items = flat(rng, spoil(rng, rows, [1, 2, 4, 7, 9], bad_sig(keys, hs)))
        (got, stats), per_share = run_sig(engine, hs, items)
        want = bytes(it[3] for it in items)
        assert got == per_share == want and want.count(0) == 5
        assert stats == (8, 4, 2, 4 * 12 + 2)
        # all valid: only the singles take the per-share check
        items = flat(rng, rows)
        (got, stats), per_share = run_sig(engine, hs, items)
        assert got == per_share == bytes([1]) * N
        assert stats == (8, 8, 2, 2) and stats.fallback_items == stats.singles
        # every group failing
        items = flat(rng, spoil(rng, rows, range(len(SIZES)), bad_sig(keys, hs)))
        (got, stats), per_share = run_sig(engine, hs, items)
        want = bytes(it[3] for it in items)
        assert got == per_share == want and want.count(0) == len(SIZES)
        assert stats == (8, 0, 2, N)


def test_dec_mixed_all_valid_all_failing(engine, keys, dec_case):
    cts, rows = dec_case
    rng = random.Random(1706)
    with forced(engine, _lib.GSUM_BUCKET):
        items = flat(rng, spoil(rng, rows, [0, 3, 5, 6, 8], bad_dec(keys, cts)))
        (got, stats), per_share = run_dec(engine, cts, items)
        want = bytes(it[3] for it in items)
        assert got == per_share == want and want.count(0) == 5
        assert stats == (8, 4, 2, 4 * 12 + 2)
        items = flat(rng, rows)
        (got, stats), per_share = run_dec(engine, cts, items)
        assert got == per_share == bytes([1]) * N
        assert stats == (8, 8, 2, 2)
        items = flat(rng, spoil(rng, rows, range(len(SIZES)), bad_dec(keys, cts)))
        (got, stats), per_share = run_dec(engine, cts, items)
        want = bytes(it[3] for it in items)
        assert got == per_share == want and want.count(0) == len(SIZES)
        assert stats == (8, 0, 2, N)


def test_cancelling_pair_and_stats_equal_chain(engine, keys, sig_case, dec_case):
    """sigma_a + delta and sigma_b - delta in one group cancel in the plain sum: with supplied scalars all 1
    the group passes under either form (supplied scalars are used as given); with distinct supplied scalars
    it fails.  With supplied scalars the statistics are the chain form's, field for field."""
    sks, pks = keys
    hs, rows = sig_case
    cts, drows = dec_case
    delta = 0x1234567
    srow, drow = list(rows[3]), list(drows[3])
    for k, sign in ((0, 1), (1, -1)):
        i = srow[k][4]
        srow[k] = (pks[i], cbls.g2_mul(hs[3], (sks[i] + sign * delta) % C.R), 3, 0, i)
        i = drow[k][4]
        drow[k] = (cbls.g1_mul(cts[3][0], (sks[i] + sign * delta) % C.R), pks[i], 3, 0, i)
    rng = random.Random(1707)
    sitems = flat(rng, [rows[0], srow, rows[8]])
    ditems = flat(rng, [drows[0], drow, drows[8]])
    n = len(sitems)
    out = {}
    for impl in (_lib.GSUM_BUCKET, _lib.GSUM_CHAIN):
        with forced(engine, impl):
            out[impl] = [run(engine, tab, items, scalars=sc)[0]
                         for run, tab, items in ((run_sig, hs, sitems), (run_dec, cts, ditems))
                         for sc in ([1] * n, list(range(1, n + 1)))]
    for (got, stats), (cgot, cstats) in zip(out[_lib.GSUM_BUCKET], out[_lib.GSUM_CHAIN]):
        assert got == cgot
        assert (stats.groups, stats.groups_passed, stats.singles, stats.fallback_items) == \
               (cstats.groups, cstats.groups_passed, cstats.singles, cstats.fallback_items)
    for items, (ones, distinct) in ((sitems, out[_lib.GSUM_BUCKET][:2]), (ditems, out[_lib.GSUM_BUCKET][2:])):
        assert ones[0] == bytes([1]) * n and ones[1] == (2, 2, 1, 1)
        assert distinct[0] == bytes(it[3] for it in items) and distinct[1] == (2, 1, 1, 12 + 1)


def test_bad_impl_value_keeps_the_form(engine, keys, sig_case):
    hs, rows = sig_case
    items = rows[0] + rows[1]
    args = ([it[0] for it in items], [it[1] for it in items], hs, [it[2] for it in items])
    with forced(engine, _lib.GSUM_BUCKET):
        for bad in (-1, 3, 99):
            with pytest.raises(HbhError):
                engine.set_group_sum_impl(bad)
        assert _lib.lib().hbh_engine_set_group_sum_impl(engine._h, 7) == 1  # HBH_ERR_ARG
        # the refused values changed nothing: the call goes on working under the form set before
        got, stats = engine.verify_sig_shares_grouped(*args)
        assert got == bytes([1]) * len(items) and stats == (2, 2, 0, 0)
    for impl in (_lib.GSUM_AUTO, _lib.GSUM_CHAIN, _lib.GSUM_BUCKET, _lib.GSUM_AUTO):
        engine.set_group_sum_impl(impl)
