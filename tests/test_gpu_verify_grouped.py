"""The grouped share checks (hbh_verify_sig_shares_grouped / hbh_verify_dec_shares_grouped): one pairing
check per document / ciphertext on a random linear combination of its shares, the per-share check for
the groups that fail and for the items alone in their group.  The verdicts must equal the per-share
call's and the construction's in every case; the statistics say which path each item took."""
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
NODES = 64


@pytest.fixture(scope="module")
def keys():
    rng = random.Random(1602)
    sks = [rng.randrange(1, C.R) for _ in range(NODES)]
    return sks, [cbls.g1_mul(G1, sk) for sk in sks]


def interleave(rng, rows):
    """One list of the per-group rows' items in a shuffled (interleaved) order."""
    flat = [it for row in rows for it in row]
    rng.shuffle(flat)
    return flat


# ------------------------------------------------------------------ signature shares
SIG_SIZES = [1, 60, 50, 45, 40, 35, 30, 25, 14]  # 300 shares in 9 documents; document 0 holds one share


@pytest.fixture(scope="module")
def sig_case(keys):
    """items (pk, sig, doc, valid) of an all-valid batch, by document; the documents' hashes."""
    sks, pks = keys
    rng = random.Random(1603)
    hs = [cbls.g2_mul(G2, rng.randrange(1, C.R)) for _ in SIG_SIZES]
    rows = [[(pks[i], cbls.g2_mul(hs[d], sks[i]), d, 1) for i in rng.sample(range(NODES), size)]
            for d, size in enumerate(SIG_SIZES)]
    return hs, rows


def corrupt_sig(rng, keys, hs, rows, plan):
    """plan: {document: [kind, ...]}; one item per kind becomes invalid."""
    sks, pks = keys
    rows = [list(row) for row in rows]
    for d, kinds in plan.items():
        for pos, kind in zip(rng.sample(range(len(rows[d])), len(kinds)), kinds):
            pk = rows[d][pos][0]
            i = pks.index(pk)
            if kind == "wrong_doc":
                sig = cbls.g2_mul(hs[(d + 1) % len(hs)], sks[i])
            elif kind == "other_key":
                sig = cbls.g2_mul(hs[d], sks[(i + 1) % NODES])
            elif kind == "random":
                sig = cbls.g2_mul(G2, rng.randrange(1, C.R))
            else:
                sig = bytes(192)  # infinity
            rows[d][pos] = (pk, sig, d, 0)
    return rows


def run_sig(engine, hs, items, scalars=None):
    args = ([it[0] for it in items], [it[1] for it in items], hs, [it[2] for it in items])
    return engine.verify_sig_shares_grouped(*args, scalars=scalars), engine.verify_sig_shares(*args)


def test_sig_mixed_validity(engine, keys, sig_case):
    hs, rows = sig_case
    rng = random.Random(1604)
    plan = {1: ["wrong_doc"], 3: ["other_key", "random"], 5: ["infinity"], 8: ["random", "wrong_doc", "other_key"]}
    items = interleave(rng, corrupt_sig(rng, keys, hs, rows, plan))
    assert len(items) == 300
    (got, stats), per_share = run_sig(engine, hs, items)
    want = bytes(it[3] for it in items)
    assert got == per_share == want
    assert want.count(0) == 7
    bad = [k for k, it in enumerate(items) if not it[3]]
    for k in bad + rng.sample(range(len(items)), 20 - len(bad)):  # 20 samples against the oracle
        pk, sig, d, valid = items[k]
        assert cbls.verify_g2(pk, sig, hs[d]) == bool(valid) == bool(got[k])
    assert stats.groups == 8 and stats.groups_passed == 4 and stats.singles == 1
    assert stats.fallback_items == sum(SIG_SIZES[d] for d in plan) + 1


def test_sig_all_valid_runs_group_checks_only(engine, sig_case):
    hs, rows = sig_case
    rng = random.Random(1605)
    items = interleave(rng, rows)
    (got, stats), per_share = run_sig(engine, hs, items)
    assert got == per_share == bytes([1]) * 300
    assert stats == (8, 8, 1, 1)  # fallback_items == singles
    # without the single: no per-share check at all.  With profiling on, a call's pairing stage is one
    # launch set per pairing call -- the 8 group checks here, against the 299 checks of the per-share call
    items = [it for it in items if it[2] != 0]
    args = ([it[0] for it in items], [it[1] for it in items], hs, [it[2] for it in items])
    engine.set_profiling(True)
    try:
        got, stats = engine.verify_sig_shares_grouped(*args)
        grouped = [engine.stage_time(s)[1] for s in (_lib.STAGE_PREPARE, _lib.STAGE_PAIRING, _lib.STAGE_CURVE)]
        engine.set_profiling(True)  # clears the counters
        per_share = engine.verify_sig_shares(*args)
        plain = [engine.stage_time(s)[1] for s in (_lib.STAGE_PREPARE, _lib.STAGE_PAIRING, _lib.STAGE_CURVE)]
    finally:
        engine.set_profiling(False)
    assert got == per_share == bytes([1]) * 299
    assert stats == (8, 8, 0, 0)
    assert grouped == [0, 1, 1]  # one pairing call (the groups), the sums under CURVE, no fallback call
    assert plain[1] == 1 and plain[2] == 0


def test_sig_cancelling_pair(engine, keys, sig_case):
    """sigma_a + delta and sigma_b - delta in one document: the two errors cancel in the plain sum, so
    with supplied scalars all 1 the group passes and both are reported valid (supplied scalars are the
    caller's responsibility); with the engine's random scalars the group fails and both are 0."""
    sks, pks = keys
    hs, rows = sig_case
    d, delta = 4, 0x1234567
    row = list(rows[d])
    ia, ib = pks.index(row[0][0]), pks.index(row[1][0])
    row[0] = (pks[ia], cbls.g2_mul(hs[d], (sks[ia] + delta) % C.R), d, 0)
    row[1] = (pks[ib], cbls.g2_mul(hs[d], (sks[ib] - delta) % C.R), d, 0)
    items = interleave(random.Random(1606), [rows[2], row])
    (got, stats), per_share = run_sig(engine, hs, items)
    want = bytes(it[3] for it in items)
    assert got == per_share == want and want.count(0) == 2
    assert stats == (2, 1, 0, SIG_SIZES[d])
    (got, stats), _ = run_sig(engine, hs, items, scalars=[1] * len(items))
    assert got == bytes([1]) * len(items)
    assert stats == (2, 2, 0, 0)
    # distinct supplied scalars decide by the group equation again
    (got, stats), _ = run_sig(engine, hs, items, scalars=list(range(1, len(items) + 1)))
    assert got == want and stats == (2, 1, 0, SIG_SIZES[d])


def test_sig_every_group_failing(engine, keys, sig_case):
    hs, rows = sig_case
    rng = random.Random(1607)
    kinds = ["wrong_doc", "other_key", "random", "infinity"]
    plan = {d: [kinds[d % 4]] for d in range(len(SIG_SIZES))}
    items = interleave(rng, corrupt_sig(rng, keys, hs, rows, plan))
    (got, stats), per_share = run_sig(engine, hs, items)
    want = bytes(it[3] for it in items)
    assert got == per_share == want and want.count(0) == 9
    assert stats == (8, 0, 1, 300)


def test_sig_identity_map_is_all_singles(engine, keys, sig_case):
    """doc_idx None (one hash per item, as verify_signatures calls it): no two items share an entry, so
    nothing is combined and every item takes the per-share check."""
    hs, rows = sig_case
    items = list(rows[8])
    items[5] = (items[5][0], cbls.g2_mul(G2, 777), 8, 0)
    args = ([it[0] for it in items], [it[1] for it in items], [hs[8]] * len(items), None)
    got, stats = engine.verify_sig_shares_grouped(*args)
    assert got == engine.verify_sig_shares(*args) == bytes(it[3] for it in items)
    assert stats == (0, 0, len(items), len(items))


def test_grouped_argument_errors(engine, keys, sig_case):
    hs, rows = sig_case
    items = rows[8]
    args = ([it[0] for it in items], [it[1] for it in items], hs, [it[2] for it in items])
    with pytest.raises(HbhError):  # a supplied zero scalar
        engine.verify_sig_shares_grouped(*args, scalars=[3] * (len(items) - 1) + [0])
    assert engine.verify_sig_shares_grouped([], [], hs, []) == (b"", (0, 0, 0, 0))  # n = 0
    assert engine.verify_sig_shares_grouped([], [], hs, [], scalars=[]) == (b"", (0, 0, 0, 0))
    bad_idx = args[3][:-1] + [len(hs)]
    with pytest.raises(HbhError):
        engine.verify_sig_shares(*args[:3], bad_idx)
    with pytest.raises(HbhError):
        engine.verify_sig_shares_grouped(*args[:3], bad_idx)
    with pytest.raises(HbhError):
        engine.verify_dec_shares_grouped([G1], [G1], [G2], [G2], [1])
    with pytest.raises(ValueError):
        engine.verify_sig_shares_grouped(*args, scalars=[1])
    # the call still works after the errors
    assert engine.verify_sig_shares_grouped(*args)[0] == bytes([1]) * len(items)


# ------------------------------------------------------------------ decryption shares
DEC_SIZES = [1, 40, 35, 30, 14]  # 120 shares over 5 ciphertexts; ciphertext 0 holds one share


@pytest.fixture(scope="module")
def dec_case(keys):
    """items (share, pk, ct, valid) of an all-valid batch by ciphertext; (U, H_uv, W) per ciphertext with
    U = r g1, W = r H_uv, so that e(sk U, H_uv) == e(sk g1, W)."""
    sks, pks = keys
    rng = random.Random(1608)
    cts = []
    for _ in DEC_SIZES:
        r, huv = rng.randrange(1, C.R), cbls.g2_mul(G2, rng.randrange(1, C.R))
        cts.append((cbls.g1_mul(G1, r), huv, cbls.g2_mul(huv, r)))
    rows = [[(cbls.g1_mul(cts[c][0], sks[i]), pks[i], c, 1) for i in rng.sample(range(NODES), size)]
            for c, size in enumerate(DEC_SIZES)]
    return cts, rows


def corrupt_dec(rng, keys, cts, rows, plan):
    sks, pks = keys
    rows = [list(row) for row in rows]
    for c, kinds in plan.items():
        for pos, kind in zip(rng.sample(range(len(rows[c])), len(kinds)), kinds):
            pk = rows[c][pos][1]
            i = pks.index(pk)
            if kind == "wrong_ct":
                share = cbls.g1_mul(cts[(c + 1) % len(cts)][0], sks[i])
            elif kind == "other_key":
                share = cbls.g1_mul(cts[c][0], sks[(i + 1) % NODES])
            elif kind == "random":
                share = cbls.g1_mul(G1, rng.randrange(1, C.R))
            else:
                share = bytes(96)
            rows[c][pos] = (share, pk, c, 0)
    return rows


def run_dec(engine, cts, items, scalars=None):
    args = ([it[0] for it in items], [it[1] for it in items], [c[1] for c in cts], [c[2] for c in cts],
            [it[2] for it in items])
    return engine.verify_dec_shares_grouped(*args, scalars=scalars), engine.verify_dec_shares(*args)


def test_dec_mixed_validity(engine, keys, dec_case):
    cts, rows = dec_case
    rng = random.Random(1609)
    plan = {1: ["wrong_ct", "infinity"], 3: ["other_key", "random"]}
    items = interleave(rng, corrupt_dec(rng, keys, cts, rows, plan))
    assert len(items) == 120
    (got, stats), per_share = run_dec(engine, cts, items)
    want = bytes(it[3] for it in items)
    assert got == per_share == want and want.count(0) == 4
    for k in [k for k, it in enumerate(items) if not it[3]] + rng.sample(range(120), 6):
        share, pk, c, valid = items[k]
        assert cbls.pairing_eq(share, cts[c][1], pk, cts[c][2]) == bool(valid)
    assert stats == (4, 2, 1, DEC_SIZES[1] + DEC_SIZES[3] + 1)


def test_dec_all_valid(engine, dec_case):
    cts, rows = dec_case
    items = interleave(random.Random(1610), rows)
    (got, stats), per_share = run_dec(engine, cts, items)
    assert got == per_share == bytes([1]) * 120
    assert stats == (4, 4, 1, 1)


def test_dec_cancelling_pair(engine, keys, dec_case):
    sks, pks = keys
    cts, rows = dec_case
    c, delta = 2, 0x7654321
    row = list(rows[c])
    ia, ib = pks.index(row[0][1]), pks.index(row[1][1])
    row[0] = (cbls.g1_mul(cts[c][0], (sks[ia] + delta) % C.R), pks[ia], c, 0)
    row[1] = (cbls.g1_mul(cts[c][0], (sks[ib] - delta) % C.R), pks[ib], c, 0)
    items = interleave(random.Random(1611), [rows[4], row])
    (got, stats), per_share = run_dec(engine, cts, items)
    want = bytes(it[3] for it in items)
    assert got == per_share == want and want.count(0) == 2
    assert stats == (2, 1, 0, DEC_SIZES[c])
    (got, stats), _ = run_dec(engine, cts, items, scalars=[1] * len(items))
    assert got == bytes([1]) * len(items) and stats == (2, 2, 0, 0)


def test_dec_every_group_failing(engine, keys, dec_case):
    cts, rows = dec_case
    rng = random.Random(1612)
    kinds = ["wrong_ct", "other_key", "random", "infinity"]
    plan = {c: [kinds[c % 4]] for c in range(len(DEC_SIZES))}
    items = interleave(rng, corrupt_dec(rng, keys, cts, rows, plan))
    (got, stats), per_share = run_dec(engine, cts, items)
    want = bytes(it[3] for it in items)
    assert got == per_share == want and want.count(0) == 5
    assert stats == (4, 0, 1, 120)
