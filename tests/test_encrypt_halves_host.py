"""hbh_encrypt split at its hash (csrc/host_hash.cpp through hoststage.encrypt_uv / encrypt_w): the two
halves with hash_g1_g2_bp between them give hoststage.encrypt's bytes.  CPU only.  Bar: byte-identical.

Message lengths 0, 32, 64, 65 and 1,096 cover both branches of hash_g1_g2's message (V as it is up to
64 bytes, sha3(V) above) and their edges; 1,096 is a serialised row of a degree-33 Part."""
import random

import pytest

from hbbft_amd import hoststage as hs
from hbbft_amd._lib import HbhError
from oracle import bls12_381 as C
from oracle import tc

LENGTHS = (0, 32, 64, 65, 1096)


def abi_g1(pt):
    return pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def abi_g2(pt):
    (x0, x1), (y0, y1) = pt
    return b"".join(v.to_bytes(48, "little") for v in (x0, x1, y0, y1))


def halves(keys, msgs, rs, threads=0):
    uv = hs.encrypt_uv(keys, msgs, rs, threads)
    q = hs.hash_g1_g2_bp([u for u, _ in uv], [v for _, v in uv], threads)
    ws = hs.encrypt_w(q, rs, threads)
    return [(u, v, w) for (u, v), w in zip(uv, ws)]


def payloads(rng, n):
    return [bytes(rng.randrange(256) for _ in range(LENGTHS[i % len(LENGTHS)])) for i in range(n)]


@pytest.fixture(scope="module")
def keys():
    rng = random.Random(151)
    return [abi_g1(C.g1_mul(C.G1_GEN, rng.randrange(1, C.R))) for _ in range(5)]


def test_one_shared_key_comb_path(keys):
    """20 items to one key: the key's comb (>= 16 uses); the oracle on one item of each |V| branch"""
    rng = random.Random(152)
    sk = rng.randrange(1, C.R)
    pk = C.g1_mul(C.G1_GEN, sk)
    msgs = payloads(rng, 20)
    rs = [rng.randrange(1, C.R) for _ in msgs]
    got = halves([abi_g1(pk)], msgs, rs)
    assert got == hs.encrypt([abi_g1(pk)], msgs, rs)
    for i in (1, 4):
        eu, ev, ew = tc.encrypt(pk, msgs[i], rs[i])
        assert got[i] == (abi_g1(eu), ev, abi_g2(ew))


def test_per_item_keys_glv_path(keys):
    """10 items over 5 keys: every key has 2 uses, below the comb threshold"""
    rng = random.Random(153)
    msgs = payloads(rng, 10)
    rs = [rng.randrange(1, C.R) for _ in msgs]
    ks = [keys[i % 5] for i in range(10)]
    assert halves(ks, msgs, rs, threads=2) == hs.encrypt(ks, msgs, rs, threads=2)


def test_mixed_keys(keys):
    """one key with 16 uses (comb) beside four keys with 2 or 3 uses (GLV) in one call"""
    rng = random.Random(154)
    ks = [keys[0]] * 16 + [keys[1 + i % 4] for i in range(10)]
    rng.shuffle(ks)
    assert ks.count(keys[0]) == 16 and max(ks.count(k) for k in keys[1:]) < 16
    msgs = payloads(rng, len(ks))
    rs = [rng.randrange(1, C.R) for _ in msgs]
    assert halves(ks, msgs, rs) == hs.encrypt(ks, msgs, rs)


def test_edge_nonces(keys):
    """1, r - 1 and r + 5 (reduced mod r, as hbh_encrypt reduces it), on both key paths"""
    rng = random.Random(155)
    rs = [1, C.R - 1, C.R + 5]
    msgs = payloads(rng, 3)
    for ks in ([keys[0]], keys[:3]):
        got = halves(ks, msgs, rs)
        assert got == hs.encrypt(ks, msgs, rs)
        assert got[2] == hs.encrypt(ks[-1:], msgs[2:], [5])[0]
    many = [1, C.R - 1, C.R + 5] * 6  # 18 uses of one key: the comb
    msgs = payloads(rng, len(many))
    assert halves([keys[1]], msgs, many) == hs.encrypt([keys[1]], msgs, many)


def test_encrypt_w_of_the_zero_point_is_zero(keys):
    rng = random.Random(156)
    q = hs.hash_g1_g2_bp([keys[0]], [b"v"])[0]
    rs = [rng.randrange(1, C.R) for _ in range(3)]
    ws = hs.encrypt_w([bytes(192), q, bytes(192)], rs)
    assert ws[0] == bytes(192) and ws[2] == bytes(192)
    z, lam = -C.X_ABS, C.P % C.R
    s_ = ((z * z - z - 1) + (z - 1) * lam + 2 * lam * lam) % C.R
    kcof = C.H2 * pow(s_, -1, C.R) % C.R
    assert ws[1] == hs.g2_mul([q], [kcof * rs[1] % C.R])[0]


def test_bad_arguments(keys):
    with pytest.raises(HbhError):
        hs.encrypt_w([b"\xff" * 192], [1])  # coordinates >= p
    with pytest.raises(HbhError):
        hs.encrypt_uv([b"\xff" * 96], [b"m"], [1])
    with pytest.raises(ValueError):
        hs.encrypt_uv(keys[:2], [b"a", b"b", b"c"], [1, 2, 3])
    assert hs.encrypt_uv(keys[:1], [], []) == [] and hs.encrypt_w([], []) == []
