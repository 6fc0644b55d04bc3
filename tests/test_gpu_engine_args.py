"""The call contract of the C ABI's engine entry points (hbbft_amd/csrc/engine*.hip), pinned on the raw
ctypes binding: every argument error's code and message, the order of the checks where two apply,
zero-size calls, a detached commitment set, and the stage accounting of hbh_engine_stage_time.  A bad
call must leave the engine usable: correct results follow on the same engine."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import bls12_381 as C
from hbbft_amd import _lib
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Z = (ctypes.c_uint8 * 4096)()  # a non-null argument no failing call reads or writes
ZP = ctypes.cast(Z, ctypes.c_void_p)
N = None
KEEP = []

NULL = "null pointer"
THRESHOLD = "threshold out of range"
NODE = "node index out of range"
PART = "part index out of range"
COMMIT = "commitment index out of range"
IDENTITY = "identity index map requires table size == n"
INDEX = "index out of range"
DETACHED = "commitment set detached: its engine was destroyed"


def u32(*vals):
    a = (ctypes.c_uint32 * len(vals))(*vals)
    KEEP.append(a)
    return ctypes.cast(a, ctypes.c_void_p)


def expect(fn, args, msg, code=1):
    """fn(*args) fails with HbhError `hbbft_hip error <code>: <msg>` (1 = HBH_ERR_ARG)."""
    with pytest.raises(_lib.HbhError) as ei:
        _lib.check(fn(*args))
    assert str(ei.value) == "hbbft_hip error %d: %s" % (code, msg), (fn.__name__, args)


def bad_calls(L, E):
    """(function, arguments, message) of argument errors, from the entry points' checks."""
    ALL = 0xFFFFFFFF
    calls = [
        (L.hbh_verify_pairing_eq, (N, 2, ZP, ZP, 2, N, ZP, ZP, 2, N, ZP), "null engine"),
        (L.hbh_verify_pairing_eq, (E, 2, N, ZP, 2, N, ZP, ZP, 2, N, ZP), NULL),
        (L.hbh_verify_pairing_eq, (E, 2, ZP, ZP, 2, N, N, ZP, 2, N, ZP), NULL),
        (L.hbh_verify_pairing_eq, (E, 2, ZP, N, 2, N, ZP, ZP, 2, N, ZP), NULL),
        (L.hbh_verify_pairing_eq, (E, 2, ZP, ZP, 2, N, ZP, ZP, 2, N, N), NULL),
        (L.hbh_verify_pairing_eq, (E, 2, ZP, ZP, 3, N, ZP, ZP, 2, N, ZP), IDENTITY),
        (L.hbh_verify_pairing_eq, (E, 2, ZP, ZP, 2, N, ZP, ZP, 1, N, ZP), IDENTITY),
        (L.hbh_verify_pairing_eq, (E, 2, ZP, ZP, 2, u32(0, 2), ZP, ZP, 2, N, ZP), INDEX),
        (L.hbh_verify_pairing_eq, (E, 2, ZP, ZP, 2, N, ZP, ZP, 5, u32(5, 0), ZP), INDEX),
        (L.hbh_verify_pairing_eq_dev, (N, N, 2, ZP, ZP, 2, N, ZP, ZP, 2, N, ZP), "null engine"),
        (L.hbh_verify_pairing_eq_dev, (E, N, 2, ZP, N, 2, N, ZP, ZP, 2, N, ZP), NULL),
        (L.hbh_verify_pairing_eq_dev, (E, N, 2, ZP, ZP, 2, N, ZP, ZP, 2, N, N), NULL),
        (L.hbh_verify_pairing_eq_dev, (E, N, 2, ZP, ZP, 3, N, ZP, ZP, 2, N, ZP), IDENTITY),
        (L.hbh_verify_pairing_eq_dev, (E, N, 0, N, N, 0, N, N, N, 1, N, N), IDENTITY),
        (L.hbh_verify_sig_shares, (E, 2, N, ZP, ZP, 1, u32(0, 0), ZP), NULL),
        (L.hbh_verify_sig_shares, (E, 2, ZP, N, ZP, 1, u32(0, 0), ZP), NULL),
        (L.hbh_verify_sig_shares, (E, 2, ZP, ZP, N, 1, u32(0, 0), ZP), NULL),
        (L.hbh_verify_sig_shares, (E, 2, ZP, ZP, ZP, 1, u32(0, 0), N), NULL),
        (L.hbh_verify_sig_shares, (E, 2, ZP, ZP, ZP, 1, u32(0, 1), ZP), INDEX),
        (L.hbh_verify_sig_shares, (E, 2, ZP, ZP, ZP, 1, N, ZP), IDENTITY),
        (L.hbh_verify_dec_shares, (E, 2, N, ZP, ZP, ZP, 2, u32(0, 1), ZP), NULL),
        (L.hbh_verify_dec_shares, (E, 2, ZP, N, ZP, ZP, 2, u32(0, 1), ZP), NULL),
        (L.hbh_verify_dec_shares, (E, 2, ZP, ZP, N, ZP, 2, u32(0, 1), ZP), NULL),
        (L.hbh_verify_dec_shares, (E, 2, ZP, ZP, ZP, ZP, 2, u32(0, 3), ZP), INDEX),
        (L.hbh_verify_dec_shares, (E, 2, ZP, ZP, ZP, ZP, 3, N, ZP), IDENTITY),
        (L.hbh_verify_ciphertexts, (E, 2, N, ZP, ZP, ZP), NULL),
        (L.hbh_verify_ciphertexts, (E, 2, ZP, N, ZP, ZP), NULL),
        (L.hbh_verify_ciphertexts, (E, 2, ZP, ZP, ZP, N), NULL),
        (L.hbh_dbg_pairing, (E, 2, ZP, ZP, N), NULL),
        (L.hbh_dbg_pairing, (E, 2, N, ZP, ZP), NULL),
        (L.hbh_g1_mul, (E, 2, N, ZP, ZP), NULL),
        (L.hbh_g1_mul, (E, 2, ZP, ZP, N), NULL),
        (L.hbh_g2_mul, (E, 2, ZP, N, ZP), NULL),
        (L.hbh_g1_mul_gen, (E, 2, N, ZP), NULL),
        (L.hbh_g1_mul_gen, (E, 2, ZP, N), NULL),
        (L.hbh_g1_decompress, (E, 2, N, ZP, ZP), NULL),
        (L.hbh_g2_decompress, (E, 2, ZP, ZP, N), NULL),
        (L.hbh_g1_decompress_dev, (E, N, 2, N, ZP, ZP), NULL),
        (L.hbh_g2_decompress_dev, (E, N, 2, ZP, N, ZP), NULL),
        (L.hbh_g2_decompress_dev, (N, N, 2, ZP, ZP, ZP), "null engine"),
        (L.hbh_combine_verify_g2, (E, 1, 1, N, ZP, ZP, ZP, ZP, ZP, ZP), NULL),
        (L.hbh_combine_verify_g2, (E, 1, 1, u32(0, 1), ZP, N, ZP, ZP, ZP, ZP), NULL),
        (L.hbh_combine_verify_g2, (E, 1, 1, u32(0, ALL), ZP, ZP, ZP, ZP, ZP, ZP), NODE),
        (L.hbh_bivar_row, (E, 2, 1, 2, N, u32(0, 1), u32(1, 2), ZP), NULL),
        (L.hbh_bivar_row, (E, 2, 1, 2, ZP, u32(0, 2), u32(1, 2), ZP), PART),
        (L.hbh_commitment_eval, (E, 2, 1, 2, ZP, N, u32(1, 2), ZP), NULL),
        (L.hbh_commitment_eval, (E, 2, 1, 2, ZP, u32(2, 0), u32(1, 2), ZP), COMMIT),
        (L.hbh_bivar_ack_check, (E, 2, 1, 2, ZP, u32(0, 1), u32(1, 1), u32(1, 2), ZP, N), NULL),
        (L.hbh_bivar_ack_check, (E, 2, 1, 2, ZP, u32(0, 2), u32(1, 1), u32(1, 2), ZP, ZP), PART),
        (L.hbh_bivar_ack_check_dev, (E, N, 2, 1, ZP, 1, ZP, ZP, ZP, ZP, ZP, N), NULL),
        (L.hbh_bivar_ack_check_dev, (E, N, 2, 1, ZP, 0, ZP, ZP, ZP, ZP, ZP, ZP), NULL),  # no rows
        (L.hbh_commit_set_create, (N, 1, ctypes.byref(ctypes.c_void_p())), NULL),
        (L.hbh_commit_set_create, (E, 1, N), NULL),
        (L.hbh_engine_stage_time, (E, 3, ctypes.byref(ctypes.c_double()), ctypes.byref(ctypes.c_int())), "bad argument"),
    ]
    for fn in (L.hbh_interpolate_g1, L.hbh_interpolate_g2):
        calls += [(fn, (E, 1, 1, N, ZP, ZP, ZP), NULL), (fn, (E, 1, 1, u32(0, 1), ZP, ZP, N), NULL),
                  (fn, (E, 1, 1, u32(ALL, 1), ZP, ZP, ZP), NODE)]
    for fn in (L.hbh_interpolate_g1_dev, L.hbh_interpolate_g2_dev):
        calls += [(fn, (E, N, 1, 1, N, ZP, ZP, ZP), NULL), (fn, (E, N, 1, 1, ZP, ZP, ZP, N), NULL)]
    # the threshold is checked before sizes and pointers: with n = 0 and with null arguments
    for t in (-1, 4097):
        for n in (0, 1):
            calls += [
                (L.hbh_interpolate_g1, (E, n, t, N, N, N, N), THRESHOLD),
                (L.hbh_interpolate_g2, (E, n, t, N, N, N, N), THRESHOLD),
                (L.hbh_combine_verify_g2, (E, n, t, N, N, N, N, N, N, N), THRESHOLD),
                (L.hbh_bivar_row, (E, n, t, 1, N, N, N, N), THRESHOLD),
                (L.hbh_commitment_eval, (E, n, t, 1, N, N, N, N), THRESHOLD),
                (L.hbh_bivar_ack_check, (E, n, t, 1, N, N, N, N, N, N), THRESHOLD),
                (L.hbh_interpolate_g1_dev, (E, N, n, t, N, N, N, N), THRESHOLD),
                (L.hbh_interpolate_g2_dev, (E, N, n, t, N, N, N, N), THRESHOLD),
                (L.hbh_bivar_ack_check_dev, (E, N, n, t, N, 0, N, N, N, N, N, N), THRESHOLD),
            ]
        calls.append((L.hbh_commit_set_create, (E, t, ctypes.byref(ctypes.c_void_p())), THRESHOLD))
    for impl in (0, 1, 2, 9, -1):
        calls.append((L.hbh_engine_set_pairing_impl, (E, impl), "unknown or retired pairing implementation"))
    for impl in (4, -1):
        calls.append((L.hbh_engine_set_ack_impl, (E, impl), "unknown Ack-check implementation"))
    return calls


def zero_calls(L, E, CS):
    return [
        (L.hbh_verify_pairing_eq, (E, 0, N, N, 0, N, N, N, 0, N, N)),
        (L.hbh_verify_pairing_eq_dev, (E, N, 0, N, N, 0, N, N, N, 0, N, N)),
        (L.hbh_verify_sig_shares, (E, 0, N, N, N, 0, N, N)),
        (L.hbh_verify_dec_shares, (E, 0, N, N, N, N, 0, N, N)),
        (L.hbh_verify_ciphertexts, (E, 0, N, N, N, N)),
        (L.hbh_dbg_pairing, (E, 0, N, N, N)),
        (L.hbh_interpolate_g1, (E, 0, 1, N, N, N, N)),
        (L.hbh_interpolate_g2, (E, 0, 1, N, N, N, N)),
        (L.hbh_combine_verify_g2, (E, 0, 1, N, N, N, N, N, N, N)),
        (L.hbh_g1_mul, (E, 0, N, N, N)),
        (L.hbh_g2_mul, (E, 0, N, N, N)),
        (L.hbh_g1_mul_gen, (E, 0, N, N)),
        (L.hbh_bivar_row, (E, 0, 1, 0, N, N, N, N)),
        (L.hbh_g1_decompress, (E, 0, N, N, N)),
        (L.hbh_g2_decompress, (E, 0, N, N, N)),
        (L.hbh_commitment_eval, (E, 0, 1, 0, N, N, N, N)),
        (L.hbh_bivar_ack_check, (E, 0, 1, 0, N, N, N, N, N, N)),
        (L.hbh_interpolate_g1_dev, (E, N, 0, 1, N, N, N, N)),
        (L.hbh_interpolate_g2_dev, (E, N, 0, 1, N, N, N, N)),
        (L.hbh_g1_decompress_dev, (E, N, 0, N, N, N)),
        (L.hbh_g2_decompress_dev, (E, N, 0, N, N, N)),
        (L.hbh_bivar_ack_check_dev, (E, N, 0, 1, N, 0, N, N, N, N, N, N)),
        (L.hbh_commit_set_add, (CS, 0, N, N)),
        (L.hbh_bivar_row_set, (CS, 0, N, N, N)),
        (L.hbh_bivar_ack_check_set, (CS, 0, N, N, N, N, N)),
    ]


@pytest.fixture(scope="module")
def shares():
    """pk shares, signature shares, the document's hash and the verdicts of the n = 10 fixture"""
    with open(os.path.join(ROOT, "tests", "golden", "threshold_sign_n10_t3.json")) as f:
        d = json.load(f)
    doc = d["docs"][0]
    pks = [g1a(bytes.fromhex(d["pk_shares"][s["idx"]])) for s in doc["shares"]]
    sigs = [g2a(bytes.fromhex(s["sig"])) for s in doc["shares"]]
    return pks, sigs, g2a(bytes.fromhex(doc["hash"])), [int(s["valid"]) for s in doc["shares"]]


def good_call(engine, shares, n=2):
    pks, sigs, hm, want = shares
    assert list(engine.verify_sig_shares(pks[:n], sigs[:n], [hm], [0] * n)) == want[:n]


def test_argument_errors(engine, shares):
    L, E = _lib.lib(), engine.handle
    for fn, args, msg in bad_calls(L, E):
        expect(fn, args, msg)
    good_call(engine, shares)


def test_commit_set_argument_errors(engine, shares):
    L, E = _lib.lib(), engine.handle
    cs = ctypes.c_void_p()
    _lib.check(L.hbh_commit_set_create(E, 1, ctypes.byref(cs)))
    try:
        first = ctypes.c_size_t(99)
        for fn, args, msg in [
            (L.hbh_commit_set_add, (N, 1, ZP, N), "null commitment set"),
            (L.hbh_commit_set_add, (cs, 1, N, ctypes.byref(first)), NULL),
            (L.hbh_bivar_row_set, (N, 1, u32(0), u32(1), ZP), "null commitment set"),
            (L.hbh_bivar_row_set, (cs, 1, N, u32(1), ZP), NULL),
            (L.hbh_bivar_row_set, (cs, 1, u32(0), u32(1), N), NULL),
            (L.hbh_bivar_row_set, (cs, 1, u32(0), u32(1), ZP), PART),  # an empty set has no part 0
            (L.hbh_bivar_ack_check_set, (N, 1, u32(0), u32(1), u32(1), ZP, ZP), "null commitment set"),
            (L.hbh_bivar_ack_check_set, (cs, 1, u32(0), u32(1), u32(1), N, ZP), NULL),
            (L.hbh_bivar_ack_check_set, (cs, 1, u32(0), u32(1), u32(1), ZP, ZP), PART),
        ]:
            expect(fn, args, msg)
        assert first.value == 0  # written before the pointer check
    finally:
        _lib.check(L.hbh_commit_set_destroy(cs))
    good_call(engine, shares)


def test_detached_commit_set(engine, shares):
    """A set outlives a throw-away engine: every call on it is an argument error, destroying it is fine."""
    L = _lib.lib()
    e2, cs = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(L.hbh_engine_create(0, ctypes.byref(e2)))
    _lib.check(L.hbh_commit_set_create(e2, 1, ctypes.byref(cs)))
    _lib.check(L.hbh_engine_destroy(e2))
    try:
        for fn, args in [(L.hbh_commit_set_add, (cs, 1, ZP, N)), (L.hbh_commit_set_add, (cs, 0, N, N)),
                         (L.hbh_bivar_row_set, (cs, 1, u32(0), u32(1), ZP)), (L.hbh_bivar_row_set, (cs, 0, N, N, N)),
                         (L.hbh_bivar_ack_check_set, (cs, 1, u32(0), u32(1), u32(1), ZP, ZP)),
                         (L.hbh_bivar_ack_check_set, (cs, 0, N, N, N, N, N))]:
            expect(fn, args, DETACHED)
        np_, nr = ctypes.c_size_t(9), ctypes.c_size_t(9)
        _lib.check(L.hbh_commit_set_size(cs, ctypes.byref(np_), ctypes.byref(nr)))
        assert (np_.value, nr.value) == (0, 0)
    finally:
        _lib.check(L.hbh_commit_set_destroy(cs))
    good_call(engine, shares)


def test_zero_size_calls(engine, shares):
    L, E = _lib.lib(), engine.handle
    cs = ctypes.c_void_p()
    _lib.check(L.hbh_commit_set_create(E, 1, ctypes.byref(cs)))
    try:
        for fn, args in zero_calls(L, E, cs):
            assert fn(*args) == 0, fn.__name__
    finally:
        _lib.check(L.hbh_commit_set_destroy(cs))
    good_call(engine, shares)


def stages(engine):
    out = {}
    for name, stage in (("PREPARE", _lib.STAGE_PREPARE), ("PAIRING", _lib.STAGE_PAIRING), ("CURVE", _lib.STAGE_CURVE)):
        ms, launches = engine.stage_time(stage)
        assert math.isfinite(ms) and ms >= 0
        out[name] = launches
    return out


def test_stage_accounting(engine, shares):
    pks, sigs, hm, want = shares
    g1 = g1a(C.g1_uncompressed(C.G1_GEN))
    try:
        engine.set_profiling(True)
        assert stages(engine) == {"PREPARE": 0, "PAIRING": 0, "CURVE": 0}
        engine.g1_mul([g1, g1], [3, 5])
        assert stages(engine) == {"PREPARE": 0, "PAIRING": 0, "CURVE": 1}

        engine.set_profiling(True)  # resets the counts
        encs = b"".join(C.g1_compress(C.g1_mul(C.G1_GEN, k)) for k in (3, 5))
        d_in = torch.from_numpy(np.frombuffer(encs, dtype=np.uint8).copy()).to("cuda:0")
        d_out = torch.zeros(2 * 96, dtype=torch.uint8, device="cuda:0")
        d_ok = torch.zeros(2, dtype=torch.uint8, device="cuda:0")
        engine.g1_decompress_dev(None, 2, d_in.data_ptr(), d_out.data_ptr(), d_ok.data_ptr())
        torch.cuda.synchronize()
        assert d_ok.cpu().tolist() == [1, 1]
        assert stages(engine) == {"PREPARE": 0, "PAIRING": 0, "CURVE": 1}

        engine.set_profiling(True)
        engine.set_pairing_impl(_lib.IMPL_WAVE2)
        good_call(engine, shares, 2)
        assert stages(engine) == {"PREPARE": 0, "PAIRING": 1, "CURVE": 0}

        engine.set_profiling(True)
        engine.set_pairing_impl(_lib.IMPL_PAIR)  # one document shared by 8 checks: its line table is prepared
        good_call(engine, shares, 8)
        assert stages(engine) == {"PREPARE": 1, "PAIRING": 1, "CURVE": 0}
    finally:
        engine.set_pairing_impl(_lib.IMPL_AUTO)
        engine.set_profiling(False)
