"""The latency form of the point decoders (HBH_DEC_SPLIT, k_wire_split.hip: four lanes per point
split the subgroup chain's group operations): the same bytes and ok verdicts as the oracle's
r * P == O definition and as the throughput form (HBH_DEC_LANE), for subgroup / torsion / random
points, malformed and edge encodings, batch shapes on both sides of every tile, the _dev entry
points, and AUTO's thresholds."""
import functools
import random

import numpy as np
import pytest
import torch

from oracle import bls12_381 as C
from oracle import cbls
from hbbft_amd import _lib
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a
from tests import subgroup_points as S

pytestmark = pytest.mark.gpu

GROUPS = pytest.mark.parametrize("g2", [False, True], ids=["G1", "G2"])


def c_in_g1(pt):
    return cbls.g1_mul(g1a(C.g1_uncompressed(pt)), C.R) == bytes(96)


def c_in_g2(pt):
    return cbls.g2_mul(g2a(C.g2_uncompressed(pt)), C.R) == bytes(192)


def oracle_decode(g2, encs):
    dec = C.g2_decompress if g2 else C.g1_decompress
    chk = c_in_g2 if g2 else c_in_g1
    unc, abi, size = (C.g2_uncompressed, g2a, 192) if g2 else (C.g1_uncompressed, g1a, 96)
    pts, ok = [], []
    for e in encs:
        try:
            pt = dec(e, in_subgroup=chk)
            pts.append(bytes(size) if pt is None else abi(unc(pt)))
            ok.append(1)
        except C.DecodeError:
            pts.append(bytes(size))
            ok.append(0)
    return pts, ok


def decode(engine, g2, impl, encs):
    """(points, ok list) with the decoder form forced; the engine goes back to AUTO."""
    engine.set_decode_impl(impl)
    try:
        pts, ok = (engine.g2_decompress if g2 else engine.g1_decompress)(encs)
    finally:
        engine.set_decode_impl(_lib.DEC_AUTO)
    return pts, list(ok)


def flagged(b, bits):
    return bytes([b[0] | bits]) + b[1:]


def off_curve_x(g2, rng):
    """x (48 / 96 big-endian bytes, c1 first for G2) with x^3 + b not a square."""
    while True:
        if g2:
            x = (rng.randrange(C.P), rng.randrange(C.P))
            if C.f2_sqrt(C.f2_add(C.f2_mul(C.f2_sqr(x), x), C.B2)) is None:
                return x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big")
        else:
            x = rng.randrange(C.P)
            if C.fp_sqrt((x * x * x + C.B1) % C.P) is None:
                return x.to_bytes(48, "big")


@functools.lru_cache(maxsize=None)
def mixed_pool(g2):
    """40 encodings; consecutive entries cycle through valid, off-curve, on-curve outside the
    subgroup, infinity, rejected flag -- neighbouring lane quads of one wave take different paths."""
    rng = random.Random(7300 + g2)
    comp, mul, gen = (C.g2_compress, C.g2_mul, C.G2_GEN) if g2 else (C.g1_compress, C.g1_mul, C.G1_GEN)
    rand = S.random_g2_on_curve if g2 else S.random_g1_on_curve
    pool = []
    for k in range(8):
        valid = comp(mul(gen, rng.randrange(1, C.R)))
        pool.append(valid)
        pool.append(flagged(off_curve_x(g2, rng), 0x80 | (0x20 if k & 1 else 0)))
        pool.append(comp(rand(rng)))                    # order divides h r, not r (random: never in the subgroup)
        pool.append(comp(None))
        pool.append(bytes([valid[0] & 0x7F]) + valid[1:] if k & 1 else bytes([0xC0]) + valid[1:])
    return pool


def cyclic(pool, n):
    return [pool[j % len(pool)] for j in range(n)]


@GROUPS
def test_split_matches_r_mul(engine, g2):
    """SPLIT forced against the oracle's r * P definition: exactly the subgroup points decode."""
    sample = S.sample(g2, 192, seed=730 if g2 else 720)
    comp = C.g2_compress if g2 else C.g1_compress
    encs = [comp(pt) for _, pt in sample]
    labels = [lab for lab, _ in sample]
    assert sum(lab.startswith("order|") for lab in labels) >= (8 if g2 else 10)
    want_pts, want_ok = oracle_decode(g2, encs)
    got_pts, got_ok = decode(engine, g2, _lib.DEC_SPLIT, encs)
    bad = [labels[i] for i in range(len(encs)) if got_ok[i] != want_ok[i]]
    assert not bad, bad[:10]
    assert got_pts == want_pts
    assert want_ok == [int(lab == "subgroup") for lab in labels]


@GROUPS
def test_split_malformed_and_edge_encodings(engine, g2):
    """Infinity (proper and with a stray bit), no compression flag, the other root, x >= p (either
    component for G2), off-curve x and on-curve x outside the subgroup, against the oracle."""
    rng = random.Random(148 + g2)
    comp, mul, gen = (C.g2_compress, C.g2_mul, C.G2_GEN) if g2 else (C.g1_compress, C.g1_mul, C.G1_GEN)
    size = 96 if g2 else 48
    encs = [comp(mul(gen, rng.randrange(1, C.R))) for _ in range(4)]
    encs.append(comp(None))                                        # infinity
    encs.append(bytes([0xC0]) + bytes(size - 2) + b"\x01")         # infinity flag with a stray bit
    encs.append(bytes([encs[0][0] & 0x7F]) + encs[0][1:])           # no compression flag
    encs.append(bytes([encs[1][0] ^ 0x20]) + encs[1][1:])           # the other root: the negated point
    pb = (C.P + 5).to_bytes(48, "big")
    if g2:
        encs.append(encs[2][:48] + pb)                              # x.c0 >= p
        encs.append(bytes([pb[0] | 0x80]) + pb[1:] + encs[2][48:])   # x.c1 >= p
        p0 = C.P.to_bytes(48, "big")
        encs.append(encs[3][:48] + p0)                              # x.c0 == p
    else:
        encs.append(bytes([pb[0] | 0x80]) + pb[1:])                 # x >= p
        p0 = C.P.to_bytes(48, "big")
        encs.append(bytes([p0[0] | 0x80]) + p0[1:])                 # x == p
    n_edge = len(encs)
    rand = S.random_g2_on_curve if g2 else S.random_g1_on_curve
    for k in range(3):
        encs.append(flagged(off_curve_x(g2, rng), 0x80 | (0x20 if k & 1 else 0)))   # off the curve
        encs.append(comp(rand(rng)))                                               # on the curve, not in the subgroup
    want_pts, want_ok = oracle_decode(g2, encs)
    assert want_ok[:n_edge] == [1] * 5 + [0, 0, 1] + [0] * (n_edge - 8)
    assert want_ok[n_edge:] == [0] * 6
    got_pts, got_ok = decode(engine, g2, _lib.DEC_SPLIT, encs)
    assert got_ok == want_ok
    assert got_pts == want_pts


@GROUPS
@pytest.mark.parametrize("n", [1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 257])
def test_split_equals_lane_batch_shapes(engine, g2, n):
    """Both forms forced in turn on one engine: byte for byte the same, every slot of the last
    (partial) workgroup included."""
    encs = cyclic(mixed_pool(g2), n)
    lane_pts, lane_ok = decode(engine, g2, _lib.DEC_LANE, encs)
    split_pts, split_ok = decode(engine, g2, _lib.DEC_SPLIT, encs)
    assert split_ok == lane_ok
    assert split_pts == lane_pts
    assert lane_ok == [int(j % 5 == 0 or j % 5 == 3) for j in range(n)]   # valid and infinity decode


@GROUPS
@pytest.mark.parametrize("own_stream", [False, True], ids=["null-stream", "torch-stream"])
def test_split_dev_entry(engine, g2, own_stream):
    """The _dev entry points under SPLIT; a second decode on the same stream takes the other
    staging slot."""
    sample = S.sample(g2, 64, seed=710 + g2)
    comp = C.g2_compress if g2 else C.g1_compress
    encs = [comp(pt) for _, pt in sample]
    want_pts, want_ok = oracle_decode(g2, encs)
    n = 192 if g2 else 96
    stream = torch.cuda.Stream(device="cuda:0") if own_stream else None
    raw = stream.cuda_stream if own_stream else None
    d_in = torch.from_numpy(np.frombuffer(b"".join(encs), dtype=np.uint8).copy()).to("cuda:0")
    d_out = [torch.zeros(len(encs) * n, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    d_ok = [torch.zeros(len(encs), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    fn = engine.g2_decompress_dev if g2 else engine.g1_decompress_dev
    engine.set_decode_impl(_lib.DEC_SPLIT)
    try:
        for k in range(2):
            fn(raw, len(encs), d_in.data_ptr(), d_out[k].data_ptr(), d_ok[k].data_ptr())
        torch.cuda.synchronize()
    finally:
        engine.set_decode_impl(_lib.DEC_AUTO)
    for k in range(2):
        assert list(d_ok[k].cpu().numpy()) == want_ok
        got = d_out[k].cpu().numpy().tobytes()
        assert [got[i * n:(i + 1) * n] for i in range(len(encs))] == want_pts


@GROUPS
def test_auto_boundaries(engine, g2):
    """AUTO at its threshold T and at T + 1 equals the forced throughput form."""
    T = _lib.AUTO_DEC_G2_SPLIT_MAX if g2 else _lib.AUTO_DEC_G1_SPLIT_MAX
    if T == 0:
        pytest.skip("AUTO never picks SPLIT for this group (threshold 0: SPLIT won nowhere in the sweep)")
    pool = mixed_pool(g2)
    for n in (T, T + 1):
        encs = cyclic(pool, n)
        lane_pts, lane_ok = decode(engine, g2, _lib.DEC_LANE, encs)
        auto_pts, auto_ok = decode(engine, g2, _lib.DEC_AUTO, encs)
        assert auto_ok == lane_ok
        assert auto_pts == lane_pts
        assert sum(lane_ok) == sum(1 for j in range(n) if j % 5 in (0, 3))


def test_set_decode_impl_rejects_unknown(engine):
    """An unknown value is the engine's argument error (HBH_ERR_ARG = 1) and leaves the previous
    setting in force: the engine goes on decoding (both forms write the same bytes, so which one ran
    is not visible from here)."""
    encs = cyclic(mixed_pool(False), 5)
    want = decode(engine, False, _lib.DEC_LANE, encs)
    engine.set_decode_impl(_lib.DEC_SPLIT)
    try:
        for bad in (7, -1, 3):
            with pytest.raises(_lib.HbhError, match="error 1: unknown point-decoding implementation"):
                engine.set_decode_impl(bad)
        pts, ok = engine.g1_decompress(encs)
        assert (pts, list(ok)) == want
    finally:
        engine.set_decode_impl(_lib.DEC_AUTO)
