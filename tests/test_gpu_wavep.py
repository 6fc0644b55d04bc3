"""HBH_IMPL_WAVEP (k_wavep.hip: one wave per check, WV_PACK checks per workgroup, the final
exponentiation's cyclotomic-squaring runs and inversion shared on the workgroup's first wave), forced
through set_pairing_impl: bit-exact verdicts and values against the lane-pair kernel, the
construction and the oracles.  Every call size here has a partial last workgroup for at least one of
the two pack factors the kernel builds with (2 and 3)."""
import random

import numpy as np
import pytest
import torch

from oracle import bls12_381 as C
from oracle import cbls, tc
from hbbft_amd._lib import AUTO_WAVEP_MAX, AUTO_WAVEP_MIN, IMPL_AUTO, IMPL_PAIR, IMPL_WAVEP
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a

pytestmark = pytest.mark.gpu
R = C.R
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))


def forced(engine, impl, fn, *args):
    engine.set_pairing_impl(impl)
    try:
        return fn(*args)
    finally:
        engine.set_pairing_impl(IMPL_AUTO)


def dev(b, dtype=torch.uint8):
    t = torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).to("cuda:0")
    return t if dtype == torch.uint8 else t.view(dtype)


@pytest.fixture(scope="module")
def share_pool():
    """14 sign-share items over 3 documents: valid, forged (another document's share, another node's
    key) and all-zero points (pk = sig = O verifies: a pairing with O is 1), with the C oracle's
    verdict of each."""
    rng = random.Random(1010)
    hs = [cbls.g2_mul(G2, rng.randrange(1, R)) for _ in range(3)]
    sk = [rng.randrange(1, R) for _ in range(5)]
    pks = [cbls.g1_mul(G1, k) for k in sk]
    kinds = ["ok", "doc", "inf", "ok", "key", "ok", "sig_inf", "doc", "ok", "inf", "ok", "key", "ok", "ok"]
    items = []
    for i, kind in enumerate(kinds):
        d, j = i % 3, i % 5
        pk, sig = pks[j], cbls.g2_mul(hs[d], sk[j])
        if kind == "doc":
            sig = cbls.g2_mul(hs[(d + 1) % 3], sk[j])
        elif kind == "key":
            pk = pks[(j + 1) % 5]
        elif kind == "inf":
            pk, sig = bytes(96), bytes(192)
        elif kind == "sig_inf":
            sig = bytes(192)
        items.append((pk, sig, d, cbls.verify_g2(pk, sig, hs[d])))
    assert [it[3] for it in items] == [k in ("ok", "inf") for k in kinds]
    return hs, items


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7])
def test_sig_shares_every_remainder(engine, share_pool, n):
    """n = 1..7 covers every fill of the last workgroup for 2 and for 3 checks per workgroup."""
    hs, items = share_pool
    batch = [items[(n + k) % len(items)] for k in range(n)]  # n = 1 starts on a forged share
    args = ([b[0] for b in batch], [b[1] for b in batch], hs, [b[2] for b in batch])
    got = forced(engine, IMPL_WAVEP, engine.verify_sig_shares, *args)
    ref = forced(engine, IMPL_PAIR, engine.verify_sig_shares, *args)
    assert got == ref
    assert list(got) == [int(b[3]) for b in batch]


@pytest.mark.parametrize("slot", [0, 1, 2])
def test_index_out_of_range_in_every_wave(engine, share_pool, slot):
    """A Q index past its table at slot 0, 1, 2 of a 5-check call (every wave of a workgroup of
    three, both waves of one of two): that check gets verdict 0 -- it runs to the workgroup's last
    barrier as an inactive check instead of leaving early --, the other four equal PAIR's, and the
    call returns normally."""
    hs, items = share_pool
    batch = [items[k] for k in (0, 3, 5, 1, 8)]  # valid x3, forged, valid
    n = len(batch)
    d_pk, d_sg, d_h = dev(b"".join(b[0] for b in batch)), dev(b"".join(b[1] for b in batch)), dev(b"".join(hs))

    def run(impl, di):
        d_di = dev(np.array(di, dtype=np.uint32).tobytes(), torch.int32)
        d_v = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
        forced(engine, impl, engine.verify_pairing_eq_dev, None, n, d_pk.data_ptr(), d_h.data_ptr(), len(hs),
               d_di.data_ptr(), None, d_sg.data_ptr(), n, None, d_v.data_ptr())
        torch.cuda.synchronize()
        return bytes(d_v.cpu().numpy())

    di = [b[2] for b in batch]
    clean = run(IMPL_PAIR, di)
    assert list(clean) == [1, 1, 1, 0, 1]
    for bad_index in (len(hs), 1 << 30):  # == table size; far out of range
        bad = list(di)
        bad[slot] = bad_index
        got = run(IMPL_WAVEP, bad)
        want = bytearray(clean)
        want[slot] = 0
        assert got == bytes(want), (slot, bad_index)
        assert got == run(IMPL_PAIR, bad)


def f12_bytes(e):
    return b"".join(c.to_bytes(48, "little") for six in e for f2 in six for c in f2)


def test_pairing_values_match_oracle(engine):
    """hbh_dbg_pairing runs through the selected kind: four pairs (a partial second workgroup for
    either pack factor), each value the oracle's e(P, Q)^3, bit-exact."""
    rng = random.Random(44)
    ks = [(rng.randrange(1, R), rng.randrange(1, R)) for _ in range(4)]
    P = [C.g1_mul(C.G1_GEN, a) for a, _ in ks]
    Q = [C.g2_mul(C.G2_GEN, b) for _, b in ks]
    pa, qa = [g1a(C.g1_uncompressed(p)) for p in P], [g2a(C.g2_uncompressed(q)) for q in Q]
    out = forced(engine, IMPL_WAVEP, engine.dbg_pairing, pa, qa)
    for k, (p, q) in enumerate(zip(P, Q)):
        assert out[k] == f12_bytes(C.f12_pow(C.pairing(p, q), 3)), k
    assert out == forced(engine, IMPL_PAIR, engine.dbg_pairing, pa, qa)


def test_dec_shares_tabled_sides_partial_last_group(engine):
    """1,025 decryption-share checks over 5 ciphertexts: both G2 sides are shared and the call has at
    least HBH_WAVE_TT_MIN checks, so both are tabled and the TT Miller program runs; 1,025 = 3 * 341 + 2
    = 2 * 512 + 1 leaves the last workgroup partial.  Forged shares sit in the first, a middle and the
    last workgroup; verdicts equal PAIR's and the construction's."""
    n, ncts, nodes, t = 1025, 5, 16, 5
    rng = random.Random(1025)
    coeffs = [rng.randrange(1, R) for _ in range(t + 1)]
    sks = [tc.poly_eval(coeffs, i + 1) for i in range(nodes)]
    pks = engine.g1_mul([G1] * nodes, sks)
    rs = [rng.randrange(1, R) for _ in range(ncts)]
    hh = [rng.randrange(1, R) for _ in range(ncts)]
    us = engine.g1_mul([G1] * ncts, rs)
    huv = engine.g2_mul([G2] * ncts, hh)
    ws = engine.g2_mul([G2] * ncts, [h * r % R for h, r in zip(hh, rs)])
    ct = [i % ncts for i in range(n)]
    bad = {0, 1, 2, 511, 512, 513, 1022, 1023, 1024} | set(range(7, n, 97))
    shares = engine.g1_mul([us[ct[i]] for i in range(n)],
                           [rng.randrange(1, R) if i in bad else sks[i % nodes] for i in range(n)])
    want = bytes(0 if i in bad else 1 for i in range(n))
    args = (shares, [pks[i % nodes] for i in range(n)], huv, ws, ct)
    got = forced(engine, IMPL_WAVEP, engine.verify_dec_shares, *args)
    assert got == want
    assert got == forced(engine, IMPL_PAIR, engine.verify_dec_shares, *args)
    for i in (0, 3, 512, 1024):
        assert cbls.pairing_eq(shares[i], huv[ct[i]], pks[i % nodes], ws[ct[i]]) == bool(got[i]), i


if AUTO_WAVEP_MIN <= AUTO_WAVEP_MAX:  # AUTO uses the form: both sides of both ends of its range

    @pytest.mark.parametrize("n", sorted({max(AUTO_WAVEP_MIN - 1, 1), AUTO_WAVEP_MIN, AUTO_WAVEP_MAX,
                                          AUTO_WAVEP_MAX + 1}))
    def test_auto_range_boundaries(engine, n):
        nodes, ndocs = 64, (AUTO_WAVEP_MAX + 1 + 63) // 64
        rng = random.Random(AUTO_WAVEP_MAX)
        sks = [rng.randrange(1, R) for _ in range(nodes)]
        pks = engine.g1_mul([G1] * nodes, sks)
        hashes = engine.g2_mul([G2] * ndocs, [rng.randrange(1, R) for _ in range(ndocs)])
        bad = set(range(0, n, 61)) | {n - 1}
        sigs = engine.g2_mul([hashes[i // nodes] for i in range(n)],
                             [rng.randrange(1, R) if i in bad else sks[i % nodes] for i in range(n)])
        v = engine.verify_sig_shares([pks[i % nodes] for i in range(n)], sigs, hashes, [i // nodes for i in range(n)])
        assert v == bytes(0 if i in bad else 1 for i in range(n))
