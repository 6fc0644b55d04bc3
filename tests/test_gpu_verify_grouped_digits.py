"""The grouped share checks under the digit form of the scalars (hbh_engine_set_group_scalar_form
HBH_GSCALAR_DIGITS: X4 for signature shares, X2 for decryption shares), against the per-share call and
the construction.  One batch per kind: three documents / ciphertexts of 2, 5 and GROUP_TILE + 1 shares and
one single.  Every test restores the INT128 form.

The cancelling-pair tests are the "used as given, in the form's layout" contract: two invalid shares
whose errors are rho_b t and -rho_a t cancel exactly under the scalars whose DIGITS stand for rho_a and
rho_b, so the group passes under the digit form -- and fails when the same bytes are read as integers."""
import contextlib
import random

import pytest

from hbbft_amd import _lib
from hbbft_amd._lib import GFORM_X2, GFORM_X4, GSCALAR_DIGITS, GSCALAR_INT128, HbhError
from hbbft_amd.engine import digit_scalar, g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a
from hbbft_amd.protocol import BatchVerifier, Ciphertext, NetworkInfo, ThresholdDecrypt, ThresholdSign
from oracle import bls12_381 as C
from oracle import cbls, tc

pytestmark = pytest.mark.gpu
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
SIZES = [1, 2, 5, _lib.GROUP_TILE + 1]  # entry 0 holds the single
NODES = _lib.GROUP_TILE + 1
TOTAL = sum(SIZES)


@contextlib.contextmanager
def digits(engine):
    engine.set_group_scalar_form(GSCALAR_DIGITS)
    try:
        yield
    finally:
        engine.set_group_scalar_form(GSCALAR_INT128)


@pytest.fixture(scope="module")
def keys():
    rng = random.Random(2210)
    sks = [rng.randrange(1, C.R) for _ in range(NODES)]
    return sks, [cbls.g1_mul(G1, sk) for sk in sks]


def rand_digits(rng, form, n):
    nd, bits = (4, 32) if form == GFORM_X4 else (2, 64)
    out = []
    while len(out) < n:
        dg = [rng.randrange(1 << bits) for _ in range(nd)]
        if any(dg):
            out.append(dg)
    return out


def packed(form, tuples):
    return [digit_scalar(form, dg)[0] for dg in tuples]


# ------------------------------------------------------------------ signature shares (X4)
@pytest.fixture(scope="module")
def sig_case(keys):
    """rows[d] = [(node, pk, sig, d)] of an all-valid batch; the documents' hashes."""
    sks, pks = keys
    rng = random.Random(2211)
    hs = [cbls.g2_mul(G2, rng.randrange(1, C.R)) for _ in SIZES]
    rows = [[(i, pks[i], cbls.g2_mul(hs[d], sks[i]), d) for i in rng.sample(range(NODES), size)]
            for d, size in enumerate(SIZES)]
    return hs, rows


def sig_batch(rng, keys, hs, rows, errors):
    """The shuffled batch with share (d, pos) signed under sk + errors[(d, pos)]: (items, want)."""
    sks, _ = keys
    items = []
    for d, row in enumerate(rows):
        for pos, (i, pk, sig, _) in enumerate(row):
            e = errors.get((d, pos), 0) % C.R
            items.append((pk, cbls.g2_mul(hs[d], (sks[i] + e) % C.R) if e else sig, d, 0 if e else 1, (d, pos)))
    rng.shuffle(items)
    return items, bytes(it[3] for it in items)


def run_sig(engine, hs, items, scalars=None):
    args = ([it[0] for it in items], [it[1] for it in items], hs, [it[2] for it in items])
    return engine.verify_sig_shares_grouped(*args, scalars=scalars), engine.verify_sig_shares(*args)


def test_sig_mixes(engine, keys, sig_case):
    hs, rows = sig_case
    rng = random.Random(2212)
    valid, want1 = sig_batch(rng, keys, hs, rows, {})
    one_bad, want2 = sig_batch(rng, keys, hs, rows, {(3, 17): 5})
    all_bad, want3 = sig_batch(rng, keys, hs, rows, {(0, 0): 1, (1, 1): 2, (2, 0): 3, (3, 128): 4})
    assert len(valid) == TOTAL <= 150 and want2.count(0) == 1 and want3.count(0) == 4
    given = packed(GFORM_X4, rand_digits(rng, GFORM_X4, TOTAL))
    int128 = {}
    for name, items, want, stats_want in (("valid", valid, want1, (3, 3, 1, 1)),
                                          ("one bad", one_bad, want2, (3, 2, 1, SIZES[3] + 1)),
                                          ("all bad", all_bad, want3, (3, 0, 1, TOTAL))):
        (got, stats), per_share = run_sig(engine, hs, items)
        assert got == per_share == want and stats == stats_want
        int128[name] = stats
    with digits(engine):
        for name, items, want in (("valid", valid, want1), ("one bad", one_bad, want2), ("all bad", all_bad, want3)):
            for scalars in (None, given):  # drawn by the engine, and given digit tuples
                (got, stats), per_share = run_sig(engine, hs, items, scalars)
                assert got == per_share == want
                assert stats == int128[name]  # the statistics of the INT128 form on the same batch
        for k in [k for k, it in enumerate(all_bad) if not it[3]] + rng.sample(range(TOTAL), 4):
            pk, sig, d, ok, _ = all_bad[k]
            assert cbls.verify_g2(pk, sig, hs[d]) == bool(ok)


def test_sig_cancelling_pair_under_given_digits(engine, keys, sig_case):
    hs, rows = sig_case
    rng = random.Random(2213)
    tuples = rand_digits(rng, GFORM_X4, TOTAL)
    probe, _ = sig_batch(random.Random(2214), keys, hs, rows, {})
    ka = [it[4] for it in probe].index((3, 0))
    kb = [it[4] for it in probe].index((3, 1))
    rho_a, rho_b = digit_scalar(GFORM_X4, tuples[ka])[1], digit_scalar(GFORM_X4, tuples[kb])[1]
    t = rng.randrange(1, C.R)
    # rho_a (rho_b t) + rho_b (-rho_a t) = 0: the two errors cancel in the combination
    items, want = sig_batch(random.Random(2214), keys, hs, rows, {(3, 0): rho_b * t, (3, 1): -rho_a * t})
    assert [it[4] for it in items] == [it[4] for it in probe] and want.count(0) == 2
    scalars = packed(GFORM_X4, tuples)
    with digits(engine):
        (got, stats), per_share = run_sig(engine, hs, items, scalars)
        assert per_share == want
        assert got == bytes([1]) * TOTAL and stats == (3, 3, 1, 1)  # used as given: the group passes
        (got, stats), _ = run_sig(engine, hs, items)  # the engine's own draw decides by the shares
        assert got == want and stats == (3, 2, 1, SIZES[3] + 1)
        with pytest.raises(HbhError):  # an invalid form leaves the previous one in force
            engine.set_group_scalar_form(2)
        assert run_sig(engine, hs, items, scalars)[0] == (bytes([1]) * TOTAL, (3, 3, 1, 1))
    # the same bytes as 128-bit integers are other residues
    (got, stats), _ = run_sig(engine, hs, items, scalars)
    assert got == want and stats == (3, 2, 1, SIZES[3] + 1)


def test_sig_zero_tuple_is_an_error(engine, keys, sig_case):
    hs, rows = sig_case
    items, want = sig_batch(random.Random(2215), keys, hs, rows, {})
    scalars = packed(GFORM_X4, rand_digits(random.Random(2216), GFORM_X4, TOTAL))
    with digits(engine):
        with pytest.raises(HbhError):
            run_sig(engine, hs, items, scalars[:-1] + [0])
        one_digit = scalars[:-1] + [digit_scalar(GFORM_X4, [0, 0, 0, 1])[0]]  # a single high digit is a scalar
        assert run_sig(engine, hs, items, one_digit)[0] == (want, (3, 3, 1, 1))


# ------------------------------------------------------------------ decryption shares (X2)
@pytest.fixture(scope="module")
def dec_case(keys):
    """rows[c] = [(node, share, pk, c)]; (U, H_uv, W) per ciphertext with U = r g1, W = r H_uv."""
    sks, pks = keys
    rng = random.Random(2217)
    cts = []
    for _ in SIZES:
        r, huv = rng.randrange(1, C.R), cbls.g2_mul(G2, rng.randrange(1, C.R))
        cts.append((cbls.g1_mul(G1, r), huv, cbls.g2_mul(huv, r)))
    rows = [[(i, cbls.g1_mul(cts[c][0], sks[i]), pks[i], c) for i in rng.sample(range(NODES), size)]
            for c, size in enumerate(SIZES)]
    return cts, rows


def dec_batch(rng, keys, cts, rows, errors):
    sks, _ = keys
    items = []
    for c, row in enumerate(rows):
        for pos, (i, share, pk, _) in enumerate(row):
            e = errors.get((c, pos), 0) % C.R
            items.append((cbls.g1_mul(cts[c][0], (sks[i] + e) % C.R) if e else share, pk, c, 0 if e else 1, (c, pos)))
    rng.shuffle(items)
    return items, bytes(it[3] for it in items)


def run_dec(engine, cts, items, scalars=None):
    args = ([it[0] for it in items], [it[1] for it in items], [c[1] for c in cts], [c[2] for c in cts],
            [it[2] for it in items])
    return engine.verify_dec_shares_grouped(*args, scalars=scalars), engine.verify_dec_shares(*args)


def test_dec_mixes(engine, keys, dec_case):
    cts, rows = dec_case
    rng = random.Random(2218)
    valid, want1 = dec_batch(rng, keys, cts, rows, {})
    one_bad, want2 = dec_batch(rng, keys, cts, rows, {(2, 3): 7})
    all_bad, want3 = dec_batch(rng, keys, cts, rows, {(0, 0): 1, (1, 0): 2, (2, 4): 3, (3, 64): 4})
    given = packed(GFORM_X2, rand_digits(rng, GFORM_X2, TOTAL))
    int128 = {}
    for name, items, want, stats_want in (("valid", valid, want1, (3, 3, 1, 1)),
                                          ("one bad", one_bad, want2, (3, 2, 1, SIZES[2] + 1)),
                                          ("all bad", all_bad, want3, (3, 0, 1, TOTAL))):
        (got, stats), per_share = run_dec(engine, cts, items)
        assert got == per_share == want and stats == stats_want
        int128[name] = stats
    with digits(engine):
        for name, items, want in (("valid", valid, want1), ("one bad", one_bad, want2), ("all bad", all_bad, want3)):
            for scalars in (None, given):
                (got, stats), per_share = run_dec(engine, cts, items, scalars)
                assert got == per_share == want
                assert stats == int128[name]
        for k in [k for k, it in enumerate(all_bad) if not it[3]] + rng.sample(range(TOTAL), 4):
            share, pk, c, ok, _ = all_bad[k]
            assert cbls.pairing_eq(share, cts[c][1], pk, cts[c][2]) == bool(ok)


def test_dec_cancelling_pair_and_zero_tuple(engine, keys, dec_case):
    cts, rows = dec_case
    rng = random.Random(2219)
    tuples = rand_digits(rng, GFORM_X2, TOTAL)
    probe, _ = dec_batch(random.Random(2220), keys, cts, rows, {})
    ka = [it[4] for it in probe].index((3, 0))
    kb = [it[4] for it in probe].index((3, 1))
    rho_a, rho_b = digit_scalar(GFORM_X2, tuples[ka])[1], digit_scalar(GFORM_X2, tuples[kb])[1]
    t = rng.randrange(1, C.R)
    items, want = dec_batch(random.Random(2220), keys, cts, rows, {(3, 0): rho_b * t, (3, 1): -rho_a * t})
    assert [it[4] for it in items] == [it[4] for it in probe] and want.count(0) == 2
    scalars = packed(GFORM_X2, tuples)
    with digits(engine):
        (got, stats), per_share = run_dec(engine, cts, items, scalars)
        assert per_share == want
        assert got == bytes([1]) * TOTAL and stats == (3, 3, 1, 1)
        (got, stats), _ = run_dec(engine, cts, items)
        assert got == want and stats == (3, 2, 1, SIZES[3] + 1)
        with pytest.raises(HbhError):
            run_dec(engine, cts, items, [0] + scalars[1:])
        with pytest.raises(HbhError):
            engine.set_group_scalar_form(-1)
        assert run_dec(engine, cts, items, scalars)[0] == (bytes([1]) * TOTAL, (3, 3, 1, 1))
    (got, stats), _ = run_dec(engine, cts, items, scalars)  # INT128 again: other residues
    assert got == want and stats == (3, 2, 1, SIZES[3] + 1)


# ------------------------------------------------------------------ BatchVerifier(scalar_form=...)
N, F = 7, 2


class Spy:
    """The engine, recording the calls made through it."""

    def __init__(self, engine):
        self._engine, self.calls = engine, []

    def __getattr__(self, name):
        attr = getattr(self._engine, name)
        if name != "set_group_scalar_form":
            self.calls.append(name)
            return attr

        def setter(form):
            self.calls.append((name, form))
            return attr(form)
        return setter


def keyset(rng):
    coeffs = [rng.randrange(1, C.R) for _ in range(F + 1)]
    sks = {i: tc.poly_eval(coeffs, i + 1) for i in range(N)}
    pks = {i: cbls.g1_mul(G1, sks[i]) for i in range(N)}
    return coeffs, sks, pks, cbls.g1_mul(G1, coeffs[0])


def record(log, step):
    log.append((list(step.output), list(step.fault_log), list(step.messages)))


def sign_flow(engine, form):
    rng = random.Random(2221)
    coeffs, sks, pks, mpk = keyset(rng)
    h = cbls.g2_mul(G2, rng.randrange(1, C.R))
    spy = Spy(engine)
    node = ThresholdSign(NetworkInfo(0, range(N), F, mpk, pks, sign_g2=lambda H: cbls.g2_mul(H, sks[0])),
                         BatchVerifier(spy, grouped=True, scalar_form=form))
    log = []
    for j in range(1, 6):  # node 3 lies; the shares arrive before the document: one drain at the input
        record(log, node.handle_message(j, cbls.g2_mul(G2, 4242) if j == 3 else cbls.g2_mul(h, sks[j])))
    node.set_document_hash(h)
    record(log, node.handle_input())
    record(log, node.handle_message(6, cbls.g2_mul(h, sks[6])))
    return log, cbls.g2_mul(h, coeffs[0]), spy.calls


def decrypt_flow(engine, form):
    rng = random.Random(2222)
    coeffs, sks, pks, mpk = keyset(rng)
    msg = bytes(rng.randrange(256) for _ in range(64))
    mpk_pt = (int.from_bytes(mpk[:48], "little"), int.from_bytes(mpk[48:], "little"))
    u, v, w = tc.encrypt(mpk_pt, msg, rng.randrange(1, C.R))
    ct = Ciphertext(g1a(C.g1_uncompressed(u)), v, g2a(C.g2_uncompressed(w)), g2a(C.g2_uncompressed(tc.hash_g1_g2(u, v))))
    spy = Spy(engine)
    node = ThresholdDecrypt(NetworkInfo(0, range(N), F, mpk, pks, decrypt_share=lambda U: cbls.g1_mul(U, sks[0])),
                            BatchVerifier(spy, grouped=True, scalar_form=form))
    log = []
    for j in range(1, 6):  # node 4 lies
        record(log, node.handle_message(j, cbls.g1_mul(G1, 999) if j == 4 else cbls.g1_mul(ct.u, sks[j])))
    node.set_ciphertext(ct)
    record(log, node.handle_input())
    record(log, node.handle_message(6, cbls.g1_mul(ct.u, sks[6])))
    return log, msg, spy.calls


@pytest.mark.parametrize("flow, call, liar", [(sign_flow, "verify_sig_shares_grouped", 3),
                                              (decrypt_flow, "verify_dec_shares_grouped", 4)])
def test_batch_verifier_scalar_form(engine, flow, call, liar):
    try:
        base, want, calls_base = flow(engine, "int128")
        got, _, calls = flow(engine, "digits")
    finally:
        engine.set_group_scalar_form(GSCALAR_INT128)
    assert got == base  # the same Steps: outputs, fault logs, messages
    assert [flt.node_id for _, faults, _ in got for flt in faults] == [liar]
    assert [out for outs, _, _ in got for out in outs] == [want]
    assert call in calls and call in calls_base
    # each verifier put its own form in force before its grouped calls
    for seen, form in ((calls, GSCALAR_DIGITS), (calls_base, GSCALAR_INT128)):
        sets = [c for c in seen[:seen.index(call)] if isinstance(c, tuple)]
        assert sets and sets[-1] == ("set_group_scalar_form", form)
