"""Device-resident prepared G2 sets (hbh_g2_set_*, hbh_verify_*_set, include/hbbft_hip.h): the shared
G2 point of a check (H per document, H_uv and W per ciphertext) prepared once into HBM and named by
slot afterwards.

* sign shares and decryption shares through the set equal the stateless calls, the golden fixtures
  and the C oracle on every pairing kernel, at a small size (where the wave kernels now take both
  tables) and at 1,026 checks through AUTO;
* one resident side beside a per-call table or a per-check side equals verify_pairing_eq;
* slots are reused lowest first, a slot that is not live is an argument error, a full set refuses;
* the _dev call on a caller stream equals the host call;
* a _set call launches no table walk (HBH_STAGE_PREPARE), an add launches one;
* argument errors, zero-size calls, foreign and detached sets."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

from oracle import bls12_381 as C
from oracle import cbls, tc
from hbbft_amd import _lib
from hbbft_amd._lib import (IMPL_AUTO, IMPL_OCT, IMPL_PAIR, IMPL_QUAD, IMPL_WAVE, IMPL_WAVE2, IMPL_WAVEP, STAGE_PAIRING,
                            STAGE_PREPARE, HbhError)
from hbbft_amd.engine import Engine, g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = C.R
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
KINDS = {"WAVE2": IMPL_WAVE2, "WAVE": IMPL_WAVE, "WAVEP": IMPL_WAVEP, "OCT": IMPL_OCT, "QUAD": IMPL_QUAD,
         "PAIR": IMPL_PAIR, "AUTO": IMPL_AUTO}
NOT_LIVE = "hbbft_hip error 1: G2 set slot is not live"


def golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def forced(engine, impl, fn, *args):
    engine.set_pairing_impl(impl)
    try:
        return fn(*args)
    finally:
        engine.set_pairing_impl(IMPL_AUTO)


def dev(b, dtype=torch.uint8):
    t = torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).to("cuda:0")
    return t if dtype == torch.uint8 else t.view(dtype)


def u32(vals):
    a = (ctypes.c_uint32 * len(vals))(*vals)
    return a, ctypes.cast(a, ctypes.c_void_p)


@pytest.fixture(scope="module")
def sign_pool():
    """64 sign-share checks over 4 documents: the 20 of the n = 10 fixture (valid, random G2, another
    document's share, infinity) with the fixture's verdicts, and 44 over two more documents (valid,
    another document's share, another node's key, pk = sig = O, sig = O) with the C oracle's.
    Returns (hashes, [(pk, sig, doc, verdict)])."""
    d = golden("threshold_sign_n10_t3.json")
    hs, items = [], []
    for k, doc in enumerate(d["docs"]):
        hs.append(g2a(bytes.fromhex(doc["hash"])))
        for s in doc["shares"]:
            items.append((g1a(bytes.fromhex(d["pk_shares"][s["idx"]])), g2a(bytes.fromhex(s["sig"])), k, int(s["valid"])))
    assert len(items) == 20 and 0 < sum(it[3] for it in items) < 20
    rng = random.Random(1212)
    more = [cbls.g2_mul(G2, rng.randrange(1, R)) for _ in range(2)]
    sk = [rng.randrange(1, R) for _ in range(6)]
    pks = [cbls.g1_mul(G1, k) for k in sk]
    kinds = ["ok", "doc", "ok", "key", "ok", "inf", "ok", "ok", "sig_inf", "ok", "doc"]
    for i in range(44):
        kind, dd, j = kinds[i % len(kinds)], i % 2, i % 6
        pk, sig = pks[j], cbls.g2_mul(more[dd], sk[j])
        if kind == "doc":
            sig = cbls.g2_mul(more[1 - dd], sk[j])
        elif kind == "key":
            pk = pks[(j + 1) % 6]
        elif kind == "inf":
            pk, sig = bytes(96), bytes(192)
        elif kind == "sig_inf":
            sig = bytes(192)
        items.append((pk, sig, 2 + dd, int(cbls.verify_g2(pk, sig, more[dd]))))
        assert items[-1][3] == int(kind in ("ok", "inf"))
    random.Random(7).shuffle(items)  # every lane group sees several documents
    return hs + more, items


@pytest.fixture(scope="module")
def dec_pool():
    """40 decryption-share checks over 4 (H_uv, W) pairs: the two ciphertexts of the n = 10 fixture
    with the fixture's verdicts, and the same two with the fixture's tampered W, where the C oracle
    gives the verdict.  Returns ([(huv, w)], [(share, pk, ct, verdict)])."""
    d = golden("threshold_decrypt_n10_t3.json")
    pks = [g1a(bytes.fromhex(p)) for p in d["pk_shares"]]
    cts, items = [], []
    for ct in d["ciphertexts"]:
        cts.append((g2a(bytes.fromhex(ct["huv"])), g2a(bytes.fromhex(ct["w"]))))
    for ct in d["ciphertexts"]:
        cts.append((g2a(bytes.fromhex(ct["huv"])), g2a(bytes.fromhex(ct["bad_w"]))))
    for k, ct in enumerate(d["ciphertexts"]):
        for s in ct["shares"]:
            sh, pk = g1a(bytes.fromhex(s["share"])), pks[s["idx"]]
            items.append((sh, pk, k, int(s["valid"])))
            items.append((sh, pk, 2 + k, int(cbls.pairing_eq(sh, cts[2 + k][0], pk, cts[2 + k][1]))))
    assert len(items) == 40 and 0 < sum(it[3] for it in items[0::2]) < 20 and not any(it[3] for it in items[1::2])
    return cts, items


@pytest.mark.parametrize("kind", list(KINDS))
def test_sig_shares_every_kernel(engine, sign_pool, kind):
    hs, items = sign_pool
    pks, sigs, di = [it[0] for it in items], [it[1] for it in items], [it[2] for it in items]
    docs = engine.g2_set(6)
    try:
        slots = docs.add(hs)
        assert slots == [0, 1, 2, 3]
        got = forced(engine, KINDS[kind], engine.verify_sig_shares_set, pks, sigs, docs, [slots[k] for k in di])
        ref = forced(engine, KINDS[kind], engine.verify_sig_shares, pks, sigs, hs, di)
    finally:
        docs.close()
    assert list(ref) == [it[3] for it in items]
    assert got == ref


def dec_set_args(cts, items, slots):
    """slots: [H_uv slots..., W slots...] of one set, in the order of cts"""
    n = len(cts)
    return ([it[0] for it in items], [it[1] for it in items], [slots[it[2]] for it in items],
            [slots[n + it[2]] for it in items])


@pytest.mark.parametrize("kind", list(KINDS))
def test_dec_shares_both_sides_resident_small(engine, dec_pool, kind):
    """40 checks, far below HBH_WAVE_TT_MIN: WAVE, WAVEP and WAVE2 read both tables (the TT program)
    where the stateless call walks both sides."""
    cts, items = dec_pool
    gs = engine.g2_set(8)
    try:
        slots = gs.add([c[0] for c in cts] + [c[1] for c in cts])
        sh, pk, hi, wi = dec_set_args(cts, items, slots)
        got = forced(engine, KINDS[kind], engine.verify_dec_shares_set, sh, pk, gs, hi, wi)
        ref = forced(engine, KINDS[kind], engine.verify_dec_shares, sh, pk, [c[0] for c in cts], [c[1] for c in cts],
                     [it[2] for it in items])
    finally:
        gs.close()
    assert list(ref) == [it[3] for it in items]
    assert got == ref


def test_dec_shares_both_sides_resident_1026_auto(engine, dec_pool):
    """1,026 checks through AUTO (WAVEP's range, where two tabled sides take TT): the 40 fixture checks
    and 986 over five more ciphertexts whose verdicts are known by construction."""
    cts, items = dec_pool
    n, nodes, extra = 1026, 16, 5
    rng = random.Random(1026)
    sks = [rng.randrange(1, R) for _ in range(nodes)]
    pks = engine.g1_mul([G1] * nodes, sks)
    rs = [rng.randrange(1, R) for _ in range(extra)]
    hh = [rng.randrange(1, R) for _ in range(extra)]
    us = engine.g1_mul([G1] * extra, rs)
    huv = engine.g2_mul([G2] * extra, hh)
    ws = engine.g2_mul([G2] * extra, [h * r % R for h, r in zip(hh, rs)])
    m = n - len(items)
    bad = {0, 1, 511, 512, m - 2, m - 1} | set(range(5, m, 89))
    ct = [i % extra for i in range(m)]
    shares = engine.g1_mul([us[c] for c in ct], [rng.randrange(1, R) if i in bad else sks[i % nodes] for i in range(m)])
    all_cts = cts + list(zip(huv, ws))
    all_items = items + [(shares[i], pks[i % nodes], len(cts) + ct[i], int(i not in bad)) for i in range(m)]
    assert len(all_items) == n
    for i in (0, 1, 2, 512):
        it = all_items[len(items) + i]
        assert cbls.pairing_eq(it[0], all_cts[it[2]][0], it[1], all_cts[it[2]][1]) == bool(it[3])
    gs = engine.g2_set(2 * len(all_cts))
    try:
        slots = gs.add([c[0] for c in all_cts] + [c[1] for c in all_cts])
        got = engine.verify_dec_shares_set(*dec_set_args(all_cts, all_items, slots)[:2], gs,
                                           *dec_set_args(all_cts, all_items, slots)[2:])
    finally:
        gs.close()
    ref = engine.verify_dec_shares([it[0] for it in all_items], [it[1] for it in all_items], [c[0] for c in all_cts],
                                   [c[1] for c in all_cts], [it[2] for it in all_items])
    assert list(ref) == [it[3] for it in all_items]
    assert got == ref


@pytest.mark.parametrize("kind", ["WAVE2", "WAVE", "WAVEP", "OCT", "PAIR", "AUTO"])
def test_mixed_sides(engine, sign_pool, dec_pool, kind):
    impl = KINDS[kind]
    # side 1 resident (H_uv), side 2 a per-call shared table (W)
    cts, items = dec_pool
    sh, pk, ci = [it[0] for it in items], [it[1] for it in items], [it[2] for it in items]
    huv, ws = [c[0] for c in cts], [c[1] for c in cts]
    gs = engine.g2_set(5)
    try:
        assert gs.add([G2]) == [0]  # the ciphertexts' slots start at 1: slot != table index
        slots = gs.add(huv)
        got = forced(engine, impl, engine.verify_pairing_eq_set, sh, gs, None, [slots[c] for c in ci], pk, None, ws, ci)
        assert got == forced(engine, impl, engine.verify_pairing_eq, sh, huv, ci, pk, ws, ci)
        assert list(got) == [it[3] for it in items]
    finally:
        gs.close()
    # side 1 per check (sigma_i under the generator), side 2 resident (H): e(g1, sigma) == e(pk, H)
    hs, sitems = sign_pool
    pks, sigs, di = [it[0] for it in sitems], [it[1] for it in sitems], [it[2] for it in sitems]
    g1s = [G1] * len(sitems)
    gs = engine.g2_set(4)
    try:
        slots = gs.add(hs)
        got = forced(engine, impl, engine.verify_pairing_eq_set, g1s, None, sigs, None, pks, gs, None,
                     [slots[k] for k in di])
        assert got == forced(engine, impl, engine.verify_pairing_eq, g1s, sigs, None, pks, hs, di)
        assert list(got) == [it[3] for it in sitems]
    finally:
        gs.close()


def test_slots(engine, sign_pool):
    hs, items = sign_pool
    by_doc = {d: [it for it in items if it[2] == d and it[3] == 1 and any(it[0])][:3] for d in range(4)}
    gs, other = engine.g2_set(3), engine.g2_set(2)

    def run(doc_of_item, slot):
        """three valid shares of document doc_of_item against the point in `slot`"""
        its = by_doc[doc_of_item]
        return list(engine.verify_sig_shares_set([it[0] for it in its], [it[1] for it in its], gs, [slot] * len(its)))

    try:
        assert gs.size() == (0, 3)
        assert gs.add(hs[:3]) == [0, 1, 2] and gs.size() == (3, 3)
        assert run(1, 1) == [1, 1, 1] and run(3, 1) == [0, 0, 0]
        with pytest.raises(HbhError, match="G2 set full"):  # a full set adds nothing
            gs.add([hs[3]])
        assert gs.size() == (3, 3)
        gs.release([1])
        assert gs.size() == (2, 3)
        with pytest.raises(HbhError) as ei:  # released
            run(1, 1)
        assert str(ei.value) == NOT_LIVE
        with pytest.raises(HbhError) as ei:  # released twice
            gs.release([1])
        assert str(ei.value) == NOT_LIVE
        assert run(0, 0) == [1, 1, 1]  # a good call succeeds afterwards
        assert gs.add([hs[3]]) == [1] and gs.size() == (3, 3)  # the freed slot, and the verdicts follow the new point
        assert run(3, 1) == [1, 1, 1] and run(1, 1) == [0, 0, 0]
        assert run(0, 0) == [1, 1, 1] and run(2, 2) == [1, 1, 1]
        # a slot never added, a slot past the capacity
        assert other.add([hs[1]]) == [0]
        its = by_doc[1]
        for bad in (1, 2, 0xFFFFFFFF):
            with pytest.raises(HbhError) as ei:
                engine.verify_sig_shares_set([it[0] for it in its], [it[1] for it in its], other, [0, bad, 0])
            assert str(ei.value) == NOT_LIVE
        # two sets on one engine do not mix: slot 0 is H_0 in one and H_1 in the other
        assert run(0, 0) == [1, 1, 1] and run(1, 0) == [0, 0, 0]
        assert list(engine.verify_sig_shares_set([it[0] for it in its], [it[1] for it in its], other, [0, 0, 0])) == [1, 1, 1]
        # a point at infinity in a slot: the stateless verdicts (1 only for pk = O, a pairing with O is 1)
        assert other.add([bytes(192)]) == [1]
        mix = by_doc[1][:1] + [it for it in items if not any(it[0])][:1]
        want = engine.verify_sig_shares([it[0] for it in mix], [it[1] for it in mix], [bytes(192)], [0, 0])
        assert list(want) == [0, 1]
        assert engine.verify_sig_shares_set([it[0] for it in mix], [it[1] for it in mix], other, [1, 1]) == want
        # a coordinate >= p is refused and takes no slot
        gs.release([0])
        with pytest.raises(HbhError, match="coordinate >= p"):
            gs.add([hs[0][:48] + b"\xff" * 48 + hs[0][96:]])
        assert gs.size() == (2, 3)
        assert gs.add([hs[0]]) == [0] and run(0, 0) == [1, 1, 1]
    finally:
        gs.close()
        other.close()


def test_dev_on_caller_stream(engine, sign_pool):
    hs, items = sign_pool
    n = len(items)
    pks, sigs, di = [it[0] for it in items], [it[1] for it in items], [it[2] for it in items]
    gs = engine.g2_set(5)
    try:
        slots = gs.add(hs)
        host = engine.verify_sig_shares_set(pks, sigs, gs, [slots[k] for k in di])
        d_pk, d_sg = dev(b"".join(pks)), dev(b"".join(sigs))
        s = torch.cuda.Stream()
        torch.cuda.synchronize()

        def run(idx):
            d_i = dev(np.array(idx, dtype=np.uint32).tobytes(), torch.int32)
            d_v = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            engine.verify_pairing_eq_set_dev(s.cuda_stream, n, d_pk.data_ptr(), gs, None, 0, d_i.data_ptr(),
                                             None, None, d_sg.data_ptr(), n, None, d_v.data_ptr())
            torch.cuda.synchronize()
            return bytes(d_v.cpu().numpy())

        assert run([slots[k] for k in di]) == host
        first_valid = next(i for i, it in enumerate(items) if it[3])
        for past in (5, 1 << 30):  # == capacity; far out of range: verdict 0, nothing else changes
            idx = [slots[k] for k in di]
            idx[first_valid] = past
            want = bytearray(host)
            want[first_valid] = 0
            assert run(idx) == bytes(want)
    finally:
        gs.close()


def test_no_table_is_built(engine, sign_pool):
    hs, items = sign_pool
    pks, sigs, di = [it[0] for it in items], [it[1] for it in items], [it[2] for it in items]
    gs = engine.g2_set(4)
    try:
        engine.set_pairing_impl(IMPL_OCT)
        engine.set_profiling(True)
        ref = engine.verify_sig_shares(pks, sigs, hs, di)
        assert engine.stage_time(STAGE_PREPARE)[1] >= 1 and engine.stage_time(STAGE_PAIRING)[1] == 1
        engine.set_profiling(True)  # resets the counts
        slots = gs.add(hs)
        assert engine.stage_time(STAGE_PREPARE)[1] == 1 and engine.stage_time(STAGE_PAIRING)[1] == 0
        engine.set_profiling(True)
        got = engine.verify_sig_shares_set(pks, sigs, gs, [slots[k] for k in di])
        assert engine.stage_time(STAGE_PREPARE)[1] == 0 and engine.stage_time(STAGE_PAIRING)[1] == 1
        assert got == ref
    finally:
        engine.set_pairing_impl(IMPL_AUTO)
        engine.set_profiling(False)
        gs.close()


def expect(fn, args, msg):
    with pytest.raises(HbhError) as ei:
        _lib.check(fn(*args))
    assert str(ei.value) == "hbbft_hip error 1: %s" % msg, (fn.__name__, args)


def test_arguments_and_lifetime(engine, sign_pool):
    hs, items = sign_pool
    L, E, N = _lib.lib(), engine.handle, None
    Z = (ctypes.c_uint8 * 4096)()
    ZP = ctypes.cast(Z, ctypes.c_void_p)
    keep0, i0 = u32([0, 0])
    gs, out = ctypes.c_void_p(), ctypes.c_void_p()
    expect(L.hbh_g2_set_create, (N, 4, ctypes.byref(out)), "null pointer")
    expect(L.hbh_g2_set_create, (E, 4, N), "null pointer")
    expect(L.hbh_g2_set_create, (E, 0, ctypes.byref(out)), "G2 set capacity out of range")
    _lib.check(L.hbh_g2_set_create(E, 4, ctypes.byref(gs)))
    NULL, TABLE = "null pointer", "a side with a G2 set takes no Q table"
    try:
        for fn, args, msg in [
            (L.hbh_g2_set_add, (N, 1, ZP, ZP), "null G2 set"),
            (L.hbh_g2_set_add, (gs, 1, N, ZP), NULL),
            (L.hbh_g2_set_add, (gs, 1, ZP, N), NULL),
            (L.hbh_g2_set_release, (N, 1, i0), "null G2 set"),
            (L.hbh_g2_set_release, (gs, 1, N), NULL),
            (L.hbh_g2_set_release, (gs, 1, i0), "G2 set slot is not live"),
            (L.hbh_g2_set_size, (N, N, N), "null G2 set"),
            (L.hbh_verify_sig_shares_set, (N, 2, ZP, ZP, gs, i0, ZP), "null engine"),
            (L.hbh_verify_sig_shares_set, (E, 2, ZP, ZP, N, i0, ZP), "null G2 set"),
            (L.hbh_verify_sig_shares_set, (E, 2, N, ZP, gs, i0, ZP), NULL),
            (L.hbh_verify_sig_shares_set, (E, 2, ZP, N, gs, i0, ZP), NULL),
            (L.hbh_verify_sig_shares_set, (E, 2, ZP, ZP, gs, N, ZP), NULL),  # no identity map onto a set
            (L.hbh_verify_sig_shares_set, (E, 2, ZP, ZP, gs, i0, N), NULL),
            (L.hbh_verify_sig_shares_set, (E, 2, ZP, ZP, gs, i0, ZP), "G2 set slot is not live"),
            (L.hbh_verify_dec_shares_set, (E, 2, N, ZP, gs, i0, i0, ZP), NULL),
            (L.hbh_verify_dec_shares_set, (E, 2, ZP, ZP, N, i0, i0, ZP), "null G2 set"),
            (L.hbh_verify_dec_shares_set, (E, 2, ZP, ZP, gs, i0, N, ZP), NULL),
            (L.hbh_verify_dec_shares_set, (E, 2, ZP, ZP, gs, i0, i0, ZP), "G2 set slot is not live"),
            (L.hbh_verify_pairing_eq_set, (N, 2, ZP, gs, N, 0, i0, ZP, N, ZP, 2, N, ZP), "null engine"),
            (L.hbh_verify_pairing_eq_set, (E, 2, ZP, gs, ZP, 0, i0, ZP, N, ZP, 2, N, ZP), TABLE),
            (L.hbh_verify_pairing_eq_set, (E, 2, ZP, gs, N, 2, i0, ZP, N, ZP, 2, N, ZP), TABLE),
            (L.hbh_verify_pairing_eq_set, (E, 2, ZP, N, ZP, 2, N, ZP, gs, N, 0, N, ZP), NULL),
            (L.hbh_verify_pairing_eq_set, (E, 2, ZP, N, ZP, 3, N, ZP, N, ZP, 2, N, ZP),
             "identity index map requires table size == n"),  # no set: hbh_verify_pairing_eq's checks
            (L.hbh_verify_pairing_eq_set_dev, (N, N, 2, ZP, gs, N, 0, ZP, N, N, ZP, 2, N, ZP), "null engine"),
            (L.hbh_verify_pairing_eq_set_dev, (E, N, 2, ZP, gs, ZP, 0, ZP, N, N, ZP, 2, N, ZP), TABLE),
            (L.hbh_verify_pairing_eq_set_dev, (E, N, 2, ZP, gs, N, 0, N, N, N, ZP, 2, N, ZP), NULL),
            (L.hbh_verify_pairing_eq_set_dev, (E, N, 2, ZP, gs, N, 0, ZP, N, N, ZP, 2, N, N), NULL),
        ]:
            expect(fn, args, msg)
        # zero-size calls
        for fn, args in [
            (L.hbh_g2_set_add, (gs, 0, N, N)),
            (L.hbh_g2_set_release, (gs, 0, N)),
            (L.hbh_verify_pairing_eq_set, (E, 0, N, gs, N, 0, N, N, gs, N, 0, N, N)),
            (L.hbh_verify_pairing_eq_set, (E, 0, N, N, N, 0, N, N, N, N, 0, N, N)),
            (L.hbh_verify_sig_shares_set, (E, 0, N, N, gs, N, N)),
            (L.hbh_verify_dec_shares_set, (E, 0, N, N, gs, N, N, N)),
            (L.hbh_verify_pairing_eq_set_dev, (E, N, 0, N, gs, N, 0, N, N, N, N, 0, N, N)),
        ]:
            assert fn(*args) == 0, fn.__name__
        live, cap = ctypes.c_size_t(9), ctypes.c_size_t(9)
        _lib.check(L.hbh_g2_set_size(gs, ctypes.byref(live), ctypes.byref(cap)))
        assert (live.value, cap.value) == (0, 4)

        # a set of another engine; then that engine goes first and leaves the set detached
        e2, gs2 = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(L.hbh_engine_create(0, ctypes.byref(e2)))
        _lib.check(L.hbh_g2_set_create(e2, 2, ctypes.byref(gs2)))
        pt, (keep1, s1) = _lib.buf(hs[0]), u32([9])
        _lib.check(L.hbh_g2_set_add(gs2, 1, pt[1], s1))
        assert keep1[0] == 0
        OTHER, DETACHED = "G2 set belongs to another engine", "G2 set detached: its engine was destroyed"
        foreign = [(L.hbh_verify_sig_shares_set, (E, 2, ZP, ZP, gs2, i0, ZP)),
                   (L.hbh_verify_dec_shares_set, (E, 2, ZP, ZP, gs2, i0, i0, ZP)),
                   (L.hbh_verify_pairing_eq_set, (E, 2, ZP, N, ZP, 2, N, ZP, gs2, N, 0, i0, ZP)),
                   (L.hbh_verify_pairing_eq_set_dev, (E, N, 2, ZP, gs2, N, 0, ZP, N, N, ZP, 2, N, ZP)),
                   (L.hbh_verify_sig_shares_set, (E, 0, N, N, gs2, N, N))]
        for fn, args in foreign:
            expect(fn, args, OTHER)
        _lib.check(L.hbh_engine_destroy(e2))
        try:
            for fn, args in foreign + [(L.hbh_g2_set_add, (gs2, 1, pt[1], s1)), (L.hbh_g2_set_add, (gs2, 0, N, N)),
                                       (L.hbh_g2_set_release, (gs2, 1, s1)), (L.hbh_g2_set_release, (gs2, 0, N))]:
                expect(fn, args, DETACHED)
            _lib.check(L.hbh_g2_set_size(gs2, ctypes.byref(live), ctypes.byref(cap)))
            assert (live.value, cap.value) == (0, 0)
        finally:
            _lib.check(L.hbh_g2_set_destroy(gs2))
        assert L.hbh_g2_set_destroy(N) == 0
    finally:
        _lib.check(L.hbh_g2_set_destroy(gs))
    # the engine is usable after every failing call
    its = items[:4]
    assert list(engine.verify_sig_shares([it[0] for it in its], [it[1] for it in its], hs, [it[2] for it in its])) == \
        [it[3] for it in its]
