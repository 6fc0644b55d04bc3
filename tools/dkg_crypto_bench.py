"""SyncKeyGen's ciphertext batches with hash_g1_g2 on the host stage against its device Q form, call by
call in one process (the protocol of tools/hash_bench.py).

  python3 tools/dkg_crypto_bench.py --out profiles/r15
  python3 tools/dkg_crypto_bench.py --sizes 1024 --reps 3 --node-round 0

Every row compares the host-stage path of this build with the new engine call forced to DEVICE
(hbh_engine_set_hash_impl) on the same inputs: outputs compared first, one warm-up call of each form at
that size, then `reps` alternations timed host-to-host with profiling off; min / median / max.

  verify      hbh_hash_g1_g2_bp + hbh_verify_pairing_eq (P1 = G1K, Q1 = W, P2 = U, Q2 = Q_bp: what
              Engine.verify_ciphertexts_bp runs) against hbh_verify_ciphertexts_uv
  encrypt     hbh_encrypt against hbh_engine_encrypt; 100 keys, 32-byte values (a SyncKeyGen node's Acks)
  hash stage  HBH_STAGE_HASH device time of hbh_engine_hash_g1_g2_bp (Q form) against hbh_engine_hash_g1_g2
              (full form), profiling on
  node round  bench.py's dkg_node_round restated (N = 100, t = 33, the same set-up and the same three timed
              steps) with SyncKeyGen(device_hash=False / True) under HBH_HASH_AUTO

--form lane | quad | both picks the device form of the hash in the verify rows (hbh_engine_set_hash_form;
default lane, the rows of profiles/r15); both times hbh_verify_ciphertexts_uv under LANE and under QUAD in
the same alternation.

A form wins a row when the other's median exceeds its own by more than both cells' min-max spreads together."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hbbft_amd import _lib, hoststage  # noqa: E402
from hbbft_amd.engine import Engine  # noqa: E402
from hbbft_amd.sync_key_gen import (G1_GEN, R_ORDER, Ack, Ciphertext, Part, SyncKeyGen, coeff_pos,  # noqa: E402
                                    poly_eval, ser_row, ser_val)

SIZES = [1024, 4096, 10100]
STAGE_SIZES = [10100, 65536]
VP = ctypes.c_void_p
NKEYS, VALUE_BYTES = 100, 32


def cell(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "samples": samples}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def wins(a, b):
    """a beats b by more than both cells' spreads"""
    return b["median_ms"] - a["median_ms"] > (a["max_ms"] - a["min_ms"]) + (b["max_ms"] - b["min_ms"])


def cbuf(b):
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


def ptr(b):
    return ctypes.cast(b, VP)


def alternate(forms, reps):
    t = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            t[k].append(timed(fn))
    return {k: cell(v) for k, v in t.items()}


def batch(n, seed):
    """n (key, 32-byte value, nonce) items over 100 keys, as hbh_encrypt's buffers"""
    rng = random.Random(seed)
    keys = hoststage.g1_mul([G1_GEN] * NKEYS, [rng.randrange(1, R_ORDER) for _ in range(NKEYS)])
    pks = cbuf(b"".join(keys[i % NKEYS] for i in range(n)))
    data = cbuf(bytes(rng.getrandbits(8) for _ in range(VALUE_BYTES * n)))
    offs = np.arange(n + 1, dtype=np.uint64) * VALUE_BYTES
    nonces = cbuf(b"".join(rng.randrange(1, R_ORDER).to_bytes(32, "little") for _ in range(n)))
    return pks, data, offs, nonces


def encrypt_ab(eng, n, reps):
    L = eng._l
    pks, data, offs, nonces = batch(n, n)
    po = offs.ctypes.data_as(VP)
    out = {k: [(ctypes.c_uint8 * (96 * n))(), (ctypes.c_uint8 * (VALUE_BYTES * n))(), (ctypes.c_uint8 * (192 * n))()]
           for k in ("host", "device")}

    def host():
        u, v, w = out["host"]
        _lib.check_host(L.hbh_encrypt(n, ptr(pks), 1, ptr(data), po, ptr(nonces), ptr(u), ptr(v), ptr(w), 0))

    def device():
        u, v, w = out["device"]
        _lib.check(L.hbh_engine_encrypt(eng.handle, n, ptr(pks), 1, ptr(data), po, ptr(nonces), ptr(u), ptr(v), ptr(w)))

    eng.set_hash_impl(_lib.HASH_DEVICE)
    host()
    device()
    assert [bytes(x) for x in out["host"]] == [bytes(x) for x in out["device"]], "ciphertexts differ at n = %d" % n
    row = {"n": n, **alternate({"host": host, "device": device}, reps)}
    row["device_wins"] = wins(row["device"], row["host"])
    return row, out["host"], offs


def verify_ab(eng, n, reps, cts, offs, form="lane"):
    """form: the device form of the hash (hbh_engine_set_hash_form) of the "device" column -- lane or quad;
    both adds a "quad" column beside the lane form's "device" """
    L = eng._l
    u, v, w = cts
    wb = bytearray(bytes(w))
    for i in range(0, n, 53):  # tampered: W of the next ciphertext
        j = (i + 1) % n
        wb[192 * i:192 * (i + 1)] = bytes(w)[192 * j:192 * (j + 1)]
    want = bytes(0 if i % 53 == 0 and n > 1 else 1 for i in range(n))
    w = cbuf(wb)
    po = offs.ctypes.data_as(VP)
    g1k = cbuf(hoststage.hash_bp_g1() * n)
    q = (ctypes.c_uint8 * (192 * n))()
    hform = {"device": _lib.HFORM_QUAD if form == "quad" else _lib.HFORM_LANE}
    if form == "both":
        hform["quad"] = _lib.HFORM_QUAD
    verdict = {k: (ctypes.c_uint8 * n)() for k in ("host", *hform)}

    def host():
        _lib.check_host(L.hbh_hash_g1_g2_bp(n, ptr(u), ptr(v), po, ptr(q), 0))
        _lib.check(L.hbh_verify_pairing_eq(eng.handle, n, ptr(g1k), ptr(w), n, None, ptr(u), ptr(q), n, None,
                                           ptr(verdict["host"])))

    def device(k):
        eng.set_hash_form(hform[k])
        _lib.check(L.hbh_verify_ciphertexts_uv(eng.handle, n, ptr(u), ptr(v), po, ptr(w), ptr(verdict[k])))

    forms = {"host": host, **{k: (lambda k=k: device(k)) for k in hform}}
    eng.set_hash_impl(_lib.HASH_DEVICE)
    for k, fn in forms.items():
        fn()
        assert bytes(verdict[k]) == want, "verdicts differ from the construction (%s)" % k
    row = {"n": n, **alternate(forms, reps)}
    eng.set_hash_form(_lib.HFORM_AUTO)
    row["device_wins"] = wins(row["device"], row["host"])
    if form == "both":
        row["quad_beats_lane"] = wins(row["quad"], row["device"])
    return row


def hash_stage(eng, n, reps):
    L = eng._l
    rng = random.Random(n)
    us = hoststage.g1_mul([G1_GEN] * 64, [rng.randrange(1, R_ORDER) for _ in range(64)])
    u = cbuf(b"".join(us[i % 64] for i in range(n)))
    data = cbuf(bytes(rng.getrandbits(8) for _ in range(VALUE_BYTES * n)))
    offs = np.arange(n + 1, dtype=np.uint64) * VALUE_BYTES
    po = offs.ctypes.data_as(VP)
    out = (ctypes.c_uint8 * (192 * n))()
    fns = {"bp": L.hbh_engine_hash_g1_g2_bp, "full": L.hbh_engine_hash_g1_g2}
    eng.set_hash_impl(_lib.HASH_DEVICE)
    t = {k: [] for k in fns}
    for rep in range(reps + 1):  # the first pass is the warm-up
        for k, fn in fns.items():
            eng.set_profiling(True)
            _lib.check(fn(eng.handle, n, ptr(u), ptr(data), po, ptr(out)))
            ms, launches = eng.stage_time(_lib.STAGE_HASH)
            eng.set_profiling(False)
            assert launches == 1
            if rep:
                t[k].append(ms)
    row = {"n": n, "bp": cell(t["bp"]), "full": cell(t["full"])}
    row["bp_wins"] = wins(row["bp"], row["full"])
    return row


def node_round(eng, n_nodes, t, reps, seed=5):
    """bench.py dkg_node_round's set-up and timed steps, once per form and repetition"""
    rng = random.Random(seed)
    sks = [rng.randrange(1, R_ORDER) for _ in range(n_nodes)]
    pks = dict(enumerate(eng.g1_mul([G1_GEN] * n_nodes, sks)))
    our, ox = 0, 1
    npos = (t + 1) * (t + 2) // 2
    coefs = [[rng.randrange(R_ORDER) for _ in range(npos)] for _ in range(n_nodes)]
    flat = eng.g1_mul_gen([c for cs in coefs for c in cs])
    commits = [flat[p * npos:(p + 1) * npos] for p in range(n_nodes)]
    ys = list(range(1, n_nodes + 1))
    our_rows = [[poly_eval([coefs[p][coeff_pos(a, b)] for b in range(t + 1)], ox) for a in range(t + 1)]
                for p in range(n_nodes)]
    our_vals = hoststage.fr_poly_eval(our_rows, ys)
    threads = hoststage.host_threads()
    row_cts = hoststage.encrypt([pks[our]], [ser_row(r) for r in our_rows],
                                [rng.randrange(1, R_ORDER) for _ in range(n_nodes)], threads)
    val_cts = hoststage.encrypt([pks[our]], [ser_val(v) for vs in our_vals for v in vs],
                                [rng.randrange(1, R_ORDER) for _ in range(n_nodes * n_nodes)], threads)
    parts = [(p, Part(t, commits[p], [Ciphertext(*row_cts[p])] * n_nodes)) for p in range(n_nodes)]
    acks = [(y - 1, Ack(p, [Ciphertext(*val_cts[p * n_nodes + y - 1])] * n_nodes)) for p in range(n_nodes) for y in ys]
    eng.set_hash_impl(_lib.HASH_AUTO)

    def one(device_hash):
        out = {}
        t0 = time.perf_counter()
        _, own = SyncKeyGen.new(our, sks[our], pks, t, eng, rng=random.Random(seed + 1), threads=threads,
                                device_hash=device_hash)
        out["generate_part_ms"] = (time.perf_counter() - t0) * 1e3
        kg = SyncKeyGen(our, sks[our], pks, t, eng, threads=threads, device_hash=device_hash)
        t0 = time.perf_counter()
        p_out = kg.handle_parts(parts, rng=random.Random(seed + 2))
        out["handle_parts_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        a_out = kg.handle_acks(acks)
        out["handle_acks_ms"] = (time.perf_counter() - t0) * 1e3
        out["node_round_ms"] = out["generate_part_ms"] + out["handle_parts_ms"] + out["handle_acks_ms"]
        ok = (len(own.rows) == n_nodes and all(o.valid and o.ack is not None for o in p_out)
              and all(o.valid for o in a_out) and kg.is_ready())
        assert ok, "a node round with faults"
        return out, own.to_bytes() + b"".join(o.ack.to_bytes() for o in p_out)

    forms = {"host": False, "device_hash": True}
    sent = {k: one(v)[1] for k, v in forms.items()}  # warm-up of each form, and the messages it sends
    assert sent["host"] == sent["device_hash"], "the two forms send different Part / Ack bytes"
    t_ = {k: {} for k in forms}
    for _ in range(reps):
        for k, v in forms.items():
            for step, ms in one(v)[0].items():
                t_[k].setdefault(step, []).append(ms)
    row = {"n_nodes": n_nodes, "t": t, "host_threads": threads}
    for k in forms:
        row[k] = {step: cell(v) for step, v in t_[k].items()}
    row["device_hash_wins"] = {step: wins(row["device_hash"][step], row["host"][step]) for step in row["host"]}
    return row


def fmt(c):
    return "%.2f / %.2f / %.2f" % (c["min_ms"], c["median_ms"], c["max_ms"])


def tables(res):
    o = []
    for name in ("verify", "encrypt"):
        o.append("### %s\n\n| items | host ms (min / median / max) | DEVICE ms (min / median / max) | DEVICE wins |\n"
                 "|---|---|---|---|" % name)
        for r in res[name]:
            o.append("| %d | %s | %s | %s |" % (r["n"], fmt(r["host"]), fmt(r["device"]), "yes" if r["device_wins"] else "no"))
        o.append("")
        if any("quad" in r for r in res[name]):
            o.append("### %s, the device hash on lanes against lane quads\n\n| items | DEVICE-LANE ms (min / median / max) | "
                     "DEVICE-QUAD ms (min / median / max) | QUAD wins |\n|---|---|---|---|" % name)
            for r in res[name]:
                if "quad" in r:
                    o.append("| %d | %s | %s | %s |" % (r["n"], fmt(r["device"]), fmt(r["quad"]),
                                                        "yes" if r["quad_beats_lane"] else "no"))
            o.append("")
    o.append("### hash stage (HBH_STAGE_HASH device time)\n\n| seeds | Q form ms (min / median / max) | full form ms "
             "(min / median / max) | Q form wins |\n|---|---|---|---|")
    for r in res["hash_stage"]:
        o.append("| %d | %s | %s | %s |" % (r["n"], fmt(r["bp"]), fmt(r["full"]), "yes" if r["bp_wins"] else "no"))
    o.append("")
    if res.get("node_round"):
        r = res["node_round"]
        o.append("### node round (N = %d, t = %d, HBH_HASH_AUTO, %d host threads)\n\n| step | device_hash off ms (min / "
                 "median / max) | device_hash on ms (min / median / max) | on wins |\n|---|---|---|---|"
                 % (r["n_nodes"], r["t"], r["host_threads"]))
        for step in r["host"]:
            o.append("| %s | %s | %s | %s |" % (step[:-3], fmt(r["host"][step]), fmt(r["device_hash"][step]),
                                                "yes" if r["device_hash_wins"][step] else "no"))
        o.append("")
    return "\n".join(o)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--stage-sizes", default=",".join(str(s) for s in STAGE_SIZES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--node-round", type=int, default=100, help="nodes of the node-round A/B, t = (N - 1) // 3 (0: skip)")
    ap.add_argument("--form", choices=("lane", "quad", "both"), default="lane",
                    help="device form of the hash in the verify rows (hbh_engine_set_hash_form); both: LANE against QUAD")
    ap.add_argument("--out", default=None, help="directory for dkg_crypto_bench.json and dkg_crypto_bench.md")
    a = ap.parse_args()
    eng = Engine(0)
    res = {"host_threads": hoststage.host_threads(), "reps": a.reps, "keys": NKEYS, "value_bytes": VALUE_BYTES,
           "auto_hash_device_min": _lib.AUTO_HASH_DEVICE_MIN, "verify": [], "encrypt": [], "hash_stage": []}
    try:
        for n in [int(s) for s in a.sizes.split(",") if s]:
            row, cts, offs = encrypt_ab(eng, n, a.reps)
            res["encrypt"].append(row)
            print("encrypt n %6d  host %s  device %s  %s" % (n, fmt(row["host"]), fmt(row["device"]),
                                                              "DEVICE" if row["device_wins"] else "-"), flush=True)
            row = verify_ab(eng, n, a.reps, cts, offs, a.form)
            res["verify"].append(row)
            print("verify  n %6d  host %s  device %s  %s" % (n, fmt(row["host"]), fmt(row["device"]),
                                                              "DEVICE" if row["device_wins"] else "-") +
                  ("  quad %s  %s" % (fmt(row["quad"]), "QUAD" if row["quad_beats_lane"] else "-") if "quad" in row else ""),
                  flush=True)
        for n in [int(s) for s in a.stage_sizes.split(",") if s]:
            row = hash_stage(eng, n, a.reps)
            res["hash_stage"].append(row)
            print("stage   n %6d  Q form %s  full form %s  %s" % (n, fmt(row["bp"]), fmt(row["full"]),
                                                                   "Q" if row["bp_wins"] else "-"), flush=True)
        if a.node_round:
            res["node_round"] = r = node_round(eng, a.node_round, (a.node_round - 1) // 3, a.reps)
            for step in r["host"]:
                print("round %-16s off %s  on %s  %s" % (step[:-3], fmt(r["host"][step]), fmt(r["device_hash"][step]),
                                                         "ON" if r["device_hash_wins"][step] else "-"), flush=True)
    finally:
        eng.set_profiling(False)
        eng.set_hash_impl(_lib.HASH_AUTO)
        eng.close()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "dkg_crypto_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        with open(os.path.join(a.out, "dkg_crypto_bench.md"), "w") as f:
            f.write(tables(res))


if __name__ == "__main__":
    main()
