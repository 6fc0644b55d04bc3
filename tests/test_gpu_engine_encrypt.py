"""PublicKey::encrypt_with_rng with the hash of the public (U, V) on the device (Engine.encrypt =
hbh_engine_encrypt: hbh_encrypt_uv on the host, the Q form of the device hash, hbh_encrypt_w on the host)
against hoststage.encrypt on the same nonces, byte for byte, and SyncKeyGen's _decrypt_batch with
device_hash=True on what it produced.  The hash form is forced to DEVICE."""
import random

import pytest

from hbbft_amd import _lib, hoststage
from hbbft_amd.sync_key_gen import G1_GEN, R_ORDER, Ciphertext, _decrypt_batch

pytestmark = pytest.mark.gpu

LENGTHS = (0, 32, 64, 65, 1096)
NKEYS = 5


@pytest.fixture(scope="module")
def material():
    """(secret keys, public keys, 130 messages, 130 nonces), computed once"""
    rng = random.Random(153)
    sks = [rng.randrange(1, R_ORDER) for _ in range(NKEYS)]
    pks = hoststage.g1_mul([G1_GEN] * NKEYS, sks)
    n = 130
    msgs = [bytes(rng.randrange(256) for _ in range(LENGTHS[i % len(LENGTHS)])) for i in range(n)]
    rs = [rng.randrange(1, R_ORDER) for _ in range(n)]
    rs[3], rs[4], rs[5] = 1, R_ORDER - 1, R_ORDER + 5
    return sks, pks, msgs, rs


@pytest.fixture
def dev(engine):
    engine.set_hash_impl(_lib.HASH_DEVICE)
    engine.set_profiling(True)
    yield engine
    engine.set_profiling(False)
    engine.dbg_set_hash_rounds(0)
    engine.set_hash_impl(_lib.HASH_AUTO)


def hash_launches(engine):
    return engine.stage_time(_lib.STAGE_HASH)[1]


def keys_for(pks, n, per_item):
    # per item: key i % 5, so at n = 130 every key has 26 uses (comb) and at n = 65 13 uses (GLV)
    return [pks[i % NKEYS] for i in range(n)] if per_item else [pks[0]]


# (one item: a single key and per-item keys are the same call)
@pytest.mark.parametrize("n,per_item", [(1, False), (65, False), (65, True), (130, False), (130, True)])
def test_bytes_equal_the_host_stage(dev, material, n, per_item):
    _, pks, msgs, rs = material
    keys = keys_for(pks, n, per_item)
    got = dev.encrypt(keys, msgs[:n], rs[:n])
    assert hash_launches(dev) == 1
    assert got == hoststage.encrypt(keys, msgs[:n], rs[:n])


def test_round_cap_leftovers_take_the_host_path(dev, material):
    _, pks, msgs, rs = material
    dev.dbg_set_hash_rounds(2)
    keys = keys_for(pks, 130, True)
    got = dev.encrypt(keys, msgs, rs)  # a quarter of 130 messages needs more than two candidates
    assert hash_launches(dev) == 1
    assert got == hoststage.encrypt(keys, msgs, rs)


def test_host_form_and_arguments(dev, material):
    _, pks, msgs, rs = material
    dev.set_hash_impl(_lib.HASH_HOST)
    dev.set_profiling(True)
    assert dev.encrypt(pks[:1], msgs[:65], rs[:65]) == hoststage.encrypt(pks[:1], msgs[:65], rs[:65])
    assert hash_launches(dev) == 0
    assert dev.encrypt(pks[:1], [], []) == []
    with pytest.raises(ValueError):
        dev.encrypt(pks[:2], msgs[:3], rs[:3])
    dev.set_hash_impl(_lib.HASH_DEVICE)
    with pytest.raises(_lib.HbhError):
        dev.encrypt([b"\xff" * 96], msgs[:1], rs[:1])  # key coordinates >= p


def test_decrypt_batch_device_hash(dev, material):
    sks, pks, msgs, rs = material
    n = 65
    cts = [Ciphertext(u, v, w) for u, v, w in dev.encrypt([pks[2]], msgs[:n], rs[:n])]
    tampered = {7: Ciphertext(cts[7].u, cts[7].v, cts[8].w), 20: Ciphertext(cts[21].u, cts[20].v, cts[20].w),
                33: Ciphertext(cts[33].u, cts[33].v[:-1] + bytes([cts[33].v[-1] ^ 0x80]), cts[33].w)}
    for k, c in tampered.items():
        cts[k] = c
    want = [None if k in tampered else msgs[k] for k in range(n)]
    dev.set_profiling(True)
    assert _decrypt_batch(dev, sks[2], cts, device_hash=True) == want
    assert hash_launches(dev) == 1
    assert _decrypt_batch(dev, sks[2], cts) == want  # the default path: host-stage hashes
    assert hash_launches(dev) == 1
