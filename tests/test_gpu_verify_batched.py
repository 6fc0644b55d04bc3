"""The batched independent checks (hbh_verify_signatures_batched, hbh_verify_ciphertexts_uv_batched): one
final exponentiation per group of 256 items, the per-item check for failed groups and a single last item.

Keys, messages and ciphertexts come from the oracle (oracle/tc.py: hash_g2, encrypt); the expected verdict
of every item is the oracle's pairing check of that item (cbls.verify_g2 / cbls.pairing_eq against
tc.hash_g2 / tc.hash_g1_g2), never the unbatched engine call.  One pool of 513 items per kind is made once:
513 keys over 24 messages, and 24 ciphertexts repeated (two items holding the same ciphertext are still
two independent checks with scalars of their own)."""
import contextlib
import ctypes
import random

import numpy as np
import pytest

from hbbft_amd import _lib
from hbbft_amd._lib import (GFORM_X4, HASH_AUTO, HASH_DEVICE, HASH_HOST, IMPL_AUTO, IMPL_OCT, IMPL_PAIR, IMPL_QUAD,
                            STAGE_HASH, HbhError)
from hbbft_amd.engine import digit_scalar, g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a
from oracle import bls12_381 as C
from oracle import cbls, tc

pytestmark = pytest.mark.gpu
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
O1, O2 = bytes(96), bytes(192)
NPOOL, NMSG = 513, 24
SIZES = [1, 2, 3, 255, 256, 257, 258, 513]


def abi1(p):
    return g1a(C.g1_uncompressed(p))


def abi2(q):
    return g2a(C.g2_uncompressed(q))


class Sig:
    """items (pk, sig, msg) with the oracle's hash of each message"""
    call = "verify_signed_batched"

    def __init__(self):
        rng = random.Random(2501)
        self.base = [b"vote %d of era %d" % (k, rng.randrange(1 << 30)) for k in range(NMSG)]
        self.hashes = {m: abi2(tc.hash_g2(m)) for m in self.base}
        self.sks = [rng.randrange(1, C.R) for _ in range(NPOOL)]
        self.items = [(cbls.g1_mul(G1, sk), cbls.g2_mul(self.hashes[self.base[i % NMSG]], sk), self.base[i % NMSG])
                      for i, sk in enumerate(self.sks)]
        self.want = bytes(self.oracle(it) for it in self.items)

    def hash_of(self, msg):
        if msg not in self.hashes:
            self.hashes[msg] = abi2(tc.hash_g2(msg))
        return self.hashes[msg]

    def oracle(self, it):
        pk, sig, msg = it
        return int(cbls.verify_g2(pk, sig, self.hash_of(msg)))

    def run(self, engine, items, scalars=None):
        return engine.verify_signed_batched([it[0] for it in items], [it[1] for it in items], [it[2] for it in items],
                                            scalars=scalars)

    def tamper(self, it, kind):
        pk, sig, msg = it
        if kind == "sig":
            return pk, cbls.g2_mul(sig, 2), msg
        assert kind == "msg"
        return pk, sig, msg + b"!"

    KINDS = ("sig", "msg")

    def infinities(self, it):
        """(both at infinity: valid), (key at infinity alone: invalid), (signature at infinity alone: invalid)"""
        pk, sig, msg = it
        return (O1, O2, msg), (O1, sig, msg), (pk, O2, msg)

    def shifted(self, i, delta):
        """item i with its signature made under sk_i + delta"""
        pk, _, msg = self.items[i]
        return pk, cbls.g2_mul(self.hash_of(msg), (self.sks[i] + delta) % C.R), msg


class Ct:
    """items (U, V, W): NMSG ciphertexts of the oracle's encrypt, repeated"""
    call = "verify_ciphertexts_uv_batched"

    def __init__(self):
        rng = random.Random(2502)
        pk = C.g1_mul(C.G1_GEN, rng.randrange(1, C.R))
        self.hashes, self.base, self.nonce = {}, [], []
        for k in range(NMSG):
            r = rng.randrange(1, C.R)
            msg = bytes(rng.randrange(256) for _ in range(32 if k % 2 else 80))  # V of <= 64 bytes and hashed V
            u, v, w = tc.encrypt(pk, msg, r)
            self.hashes[(abi1(u), bytes(v))] = abi2(tc.hash_g1_g2(u, v))
            self.base.append((abi1(u), bytes(v), abi2(w)))
            self.nonce.append(r)
        self.items = [self.base[i % NMSG] for i in range(NPOOL)]
        self.want = bytes(self.oracle(it) for it in self.items)

    def hash_of(self, u, v):
        if (u, v) not in self.hashes:
            pt = None if u == O1 else (int.from_bytes(u[:48], "little"), int.from_bytes(u[48:], "little"))
            self.hashes[(u, v)] = abi2(tc.hash_g1_g2(pt, v))
        return self.hashes[(u, v)]

    def oracle(self, it):
        u, v, w = it  # Ciphertext::verify: e(g1, W) == e(U, hash_g1_g2(U, V))
        return int(cbls.pairing_eq(G1, w, u, self.hash_of(u, v)))

    def run(self, engine, items, scalars=None):
        return engine.verify_ciphertexts_uv_batched([it[0] for it in items], [it[1] for it in items],
                                                    [it[2] for it in items], scalars=scalars)

    def tamper(self, it, kind):
        u, v, w = it
        if kind == "u":
            return cbls.g1_mul(u, 2), v, w
        if kind == "v":
            return u, bytes([v[0] ^ 1]) + v[1:], w
        assert kind == "w"
        return u, v, cbls.g2_mul(w, 2)

    KINDS = ("u", "v", "w")

    def infinities(self, it):
        u, v, w = it
        return (O1, v, O2), (O1, v, w), (u, v, O2)

    def shifted(self, i, delta):
        """item i with W made under its nonce + delta"""
        u, v, _ = self.items[i]
        return u, v, cbls.g2_mul(self.hash_of(u, v), (self.nonce[i % NMSG] + delta) % C.R)


@pytest.fixture(scope="module")
def pools():
    p = {"sig": Sig(), "ct": Ct()}
    for pool in p.values():
        assert pool.want == bytes([1]) * NPOOL  # the oracle accepts every item of the pools
    return p


def expect(pool, items, changed):
    """the oracle's verdicts of `items` = the pool's items except at the positions `changed`"""
    want = bytearray(pool.want[:len(items)])
    for i in changed:
        want[i] = pool.oracle(items[i])
    return bytes(want)


def singles(n):
    return 1 if n % 256 == 1 else 0


def groups(n):
    return (n + 255) // 256 - singles(n)


@contextlib.contextmanager
def setting(setter, value, default):
    setter(value)
    try:
        yield
    finally:
        setter(default)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["sig", "ct"])
def test_all_valid(engine, pools, kind, n):
    pool = pools[kind]
    got, st = pool.run(engine, pool.items[:n])
    assert got == pool.want[:n] == bytes([1]) * n
    assert st == (groups(n), groups(n), singles(n), singles(n))


@pytest.mark.parametrize("n, pos", [(300, 0), (300, 7), (300, 255), (300, 280), (513, 300)])
@pytest.mark.parametrize("kind, how", [("sig", k) for k in Sig.KINDS] + [("ct", k) for k in Ct.KINDS])
def test_one_invalid(engine, pools, kind, how, n, pos):
    """item 0, an odd index (side 1 of a slot), the last item of a full group, the last partial group; at
    513 a single rides along"""
    pool = pools[kind]
    items = list(pool.items[:n])
    items[pos] = pool.tamper(items[pos], how)
    want = expect(pool, items, [pos])
    assert want.count(0) == 1 and want[pos] == 0
    got, st = pool.run(engine, items)
    assert got == want
    size = min(n, 256 * (pos // 256 + 1)) - 256 * (pos // 256)
    assert st == (groups(n), groups(n) - 1, singles(n), size + singles(n))


@pytest.mark.parametrize("kind", ["sig", "ct"])
def test_infinities(engine, pools, kind):
    pool = pools[kind]
    both, first_only, second_only = pool.infinities(pool.items[5])
    assert (pool.oracle(both), pool.oracle(first_only), pool.oracle(second_only)) == (1, 0, 0)
    n = 12
    # inside a passing group: both at infinity is a valid item
    items = list(pool.items[:n])
    items[5] = both
    got, st = pool.run(engine, items)
    assert got == expect(pool, items, [5]) == bytes([1]) * n and st == (1, 1, 0, 0)
    # inside a failing group, through the fallback: each lone infinity is invalid, both still valid
    for bad in (first_only, second_only):
        items = list(pool.items[:n])
        items[5], items[8] = both, bad
        want = expect(pool, items, [5, 8])
        assert want == bytes([1]) * 8 + b"\0" + bytes([1]) * 3
        got, st = pool.run(engine, items)
        assert got == want and st == (1, 0, 0, n)
    # a single at infinity (n = 1 takes the per-item check)
    for it, ok in ((both, 1), (first_only, 0), (second_only, 0)):
        assert pool.run(engine, [it]) == (bytes([ok]), (0, 0, 1, 1))


def rand_digits(rng, n):
    out = []
    while len(out) < n:
        dg = [rng.randrange(1 << 32) for _ in range(4)]
        if any(dg):
            out.append(dg)
    return out


@pytest.mark.parametrize("kind", ["sig", "ct"])
def test_given_digits(engine, pools, kind):
    """Scalars are used as given, read as X4 digits: two invalid items whose errors are rho_b t and
    -rho_a t on the same G2 base cancel under the scalars whose digits stand for rho_a and rho_b."""
    pool = pools[kind]
    rng = random.Random(2503)
    n, a = 40, 3
    b = a + NMSG  # the same message / ciphertext: the same G2 base
    tuples = rand_digits(rng, n)
    rho_a, rho_b = digit_scalar(GFORM_X4, tuples[a])[1], digit_scalar(GFORM_X4, tuples[b])[1]
    t = rng.randrange(1, C.R)
    items = list(pool.items[:n])
    items[a], items[b] = pool.shifted(a, rho_b * t), pool.shifted(b, -rho_a * t)
    want = expect(pool, items, [a, b])
    assert want.count(0) == 2 and want[a] == want[b] == 0
    scalars = [digit_scalar(GFORM_X4, dg)[0] for dg in tuples]
    got, st = pool.run(engine, items, scalars)
    assert got == bytes([1]) * n and st == (1, 1, 0, 0)  # used as given: the group passes
    got, st = pool.run(engine, items)  # the engine's own draw decides by the items
    assert got == want and st == (1, 0, 0, n)
    # the setters of the grouped share checks do not govern these calls
    with setting(engine.set_group_scalar_form, _lib.GSCALAR_DIGITS, _lib.GSCALAR_INT128):
        assert pool.run(engine, items, scalars) == (bytes([1]) * n, (1, 1, 0, 0))
    assert pool.run(engine, pool.items[:n], scalars) == (bytes([1]) * n, (1, 1, 0, 0))
    with pytest.raises(HbhError):
        pool.run(engine, items, scalars[:-1] + [0])
    one_digit = scalars[:-1] + [digit_scalar(GFORM_X4, [0, 0, 0, 1])[0]]  # a single high digit is a scalar
    assert pool.run(engine, pool.items[:n], one_digit) == (bytes([1]) * n, (1, 1, 0, 0))


@pytest.mark.parametrize("kind", ["sig", "ct"])
def test_hash_paths(engine, pools, kind):
    """n = 257 with one invalid item: the host stage, the device form, and the device form with one
    sampler round (most messages are left over and patched in from the host stage)"""
    pool = pools[kind]
    n, pos = 257, 100
    items = list(pool.items[:n])
    items[pos] = pool.tamper(items[pos], pool.KINDS[-1])
    want = expect(pool, items, [pos])
    stats = (1, 0, 1, 257)
    with setting(engine.set_hash_impl, HASH_HOST, HASH_AUTO):
        assert pool.run(engine, items) == (want, stats)
    with setting(engine.set_hash_impl, HASH_DEVICE, HASH_AUTO):
        engine.set_profiling(True)
        try:
            assert pool.run(engine, items) == (want, stats)  # the group fell back: still one hash entry
            assert engine.stage_time(STAGE_HASH)[1] == 1
            engine.set_profiling(True)  # clears the entries
            assert pool.run(engine, pool.items[:n]) == (pool.want[:n], (1, 1, 1, 1))
            assert engine.stage_time(STAGE_HASH)[1] == 1
        finally:
            engine.set_profiling(False)
        with setting(engine.dbg_set_hash_rounds, 1, 0):
            assert pool.run(engine, items) == (want, stats)
            assert pool.run(engine, pool.items[:n]) == (pool.want[:n], (1, 1, 1, 1))


@pytest.mark.parametrize("kind", ["sig", "ct"])
def test_widths(engine, pools, kind):
    pool = pools[kind]
    n, pos = 257, 33
    items = list(pool.items[:n])
    items[pos] = pool.tamper(items[pos], pool.KINDS[0])
    want = expect(pool, items, [pos])
    seen = []
    for impl in (IMPL_PAIR, IMPL_QUAD, IMPL_OCT, IMPL_AUTO):
        with setting(engine.set_pairing_impl, impl, IMPL_AUTO):
            seen.append(pool.run(engine, items))
            assert pool.run(engine, pool.items[:n]) == (pool.want[:n], (1, 1, 1, 1))
    assert seen == [(want, (1, 0, 1, 257))] * 4


def test_argument_errors(engine, pools):
    """null pointers, bad offsets and n = 0: the unbatched call's error, text and code"""
    L, E = _lib.lib(), engine.handle
    z = (ctypes.c_uint8 * 4096)()
    ZP, N = ctypes.cast(z, ctypes.c_void_p), None
    good = np.array([0, 1, 2], dtype=np.uint64)
    desc = np.array([0, 2, 1], dtype=np.uint64)
    po = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def error(fn, args):
        with pytest.raises(HbhError) as ei:
            _lib.check(fn(*args))
        return str(ei.value)

    # (pks / u, sigs / w, data, offsets, verdicts)
    cases = [(N, ZP, ZP, po(good), ZP), (ZP, N, ZP, po(good), ZP), (ZP, ZP, ZP, po(good), N), (ZP, ZP, ZP, N, ZP),
             (ZP, ZP, N, po(good), ZP), (ZP, ZP, ZP, po(desc), ZP)]
    for a, b, data, offs, v in cases:
        assert error(L.hbh_verify_signatures_batched, (E, 2, a, b, data, offs, N, v, N)) == \
            error(L.hbh_verify_signatures, (E, 2, a, b, data, offs, v))
        assert error(L.hbh_verify_ciphertexts_uv_batched, (E, 2, a, data, offs, b, N, v, N)) == \
            error(L.hbh_verify_ciphertexts_uv, (E, 2, a, data, offs, b, v))
    assert error(L.hbh_verify_signatures_batched, (N, 2, ZP, ZP, ZP, po(good), N, ZP, N)) == \
        error(L.hbh_verify_signatures, (N, 2, ZP, ZP, ZP, po(good), ZP))
    assert error(L.hbh_verify_ciphertexts_uv_batched, (N, 2, ZP, ZP, po(good), ZP, N, ZP, N)) == \
        error(L.hbh_verify_ciphertexts_uv, (N, 2, ZP, ZP, po(good), ZP, ZP))
    for fn in (L.hbh_dbg_pairing_product,):
        assert error(fn, (N, 2, ZP, ZP, ZP)) == "hbbft_hip error 1: null engine"
        for args in ((E, 2, N, ZP, ZP), (E, 2, ZP, N, ZP), (E, 2, ZP, ZP, N)):
            assert error(fn, args) == "hbbft_hip error 1: null pointer"
    # n = 0 succeeds with every pointer null and zeroes the statistics
    st = _lib.GroupedStats(7, 7, 7, 7)
    pst = ctypes.cast(ctypes.pointer(st), ctypes.c_void_p)
    _lib.check(L.hbh_verify_signatures_batched(E, 0, N, N, N, N, N, N, pst))
    assert (st.groups, st.groups_passed, st.singles, st.fallback_items) == (0, 0, 0, 0)
    _lib.check(L.hbh_verify_ciphertexts_uv_batched(E, 0, N, N, N, N, N, N, N))
    _lib.check(L.hbh_dbg_pairing_product(E, 0, N, N, N))
    for pool in pools.values():
        assert pool.run(engine, []) == (b"", (0, 0, 0, 0))
    # the engine is still usable
    assert pools["sig"].run(engine, pools["sig"].items[:2]) == (b"\1\1", (1, 1, 0, 0))
