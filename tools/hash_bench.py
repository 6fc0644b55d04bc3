"""hash_g2 on the host stage against its device form, call by call in one process.

  python3 tools/hash_bench.py --out profiles/r14            the sweep + the verify_signed A/B
  python3 tools/hash_bench.py --sizes 1024,16384 --reps 9

For every size, hbh_engine_hash_g2 is forced to HOST and to DEVICE in turn (hbh_engine_set_hash_impl) on
the same seeded 28-byte messages: one warm-up call of each form at that size, then `reps` alternations
timed host-to-host (the synchronous call: SHA3 on the host workers, upload, kernels, download) with
profiling off; the two outputs must be equal bytes.  A second, shorter pass with profiling on records the
HBH_STAGE_HASH device time of the DEVICE form beside it.  The host form uses the host stage's default
worker count (hbh_host_threads).

The AUTO threshold the sweep supports is the smallest swept size from which DEVICE's median is below
HOST's by more than both cells' min-max spread, at that size and at every larger one (none: AUTO stays
HOST).  The same A/B is run for PublicKey::verify at --signed items: hbh_hash_g2 + hbh_verify_sig_shares
against hbh_verify_signatures forced to DEVICE."""
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
from hbbft_amd.sync_key_gen import G1_GEN, R_ORDER  # noqa: E402

SIZES = [64, 256, 1024, 4096, 10100, 16384, 65536]
VP = ctypes.c_void_p


def cell(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "samples": samples}


def messages(n, seed):
    rng = random.Random(seed)
    data = bytes(rng.getrandbits(8) for _ in range(28 * n))
    offs = np.arange(n + 1, dtype=np.uint64) * 28
    return data, offs


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def sweep_size(eng, n, reps):
    L = eng._l
    data, offs = messages(n, n)
    dbuf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    po = offs.ctypes.data_as(VP)
    outs = {k: (ctypes.c_uint8 * (n * 192))() for k in ("host", "device")}
    impl = {"host": _lib.HASH_HOST, "device": _lib.HASH_DEVICE}

    def call(form):
        eng.set_hash_impl(impl[form])
        _lib.check(L.hbh_engine_hash_g2(eng.handle, n, ctypes.cast(dbuf, VP), po, ctypes.cast(outs[form], VP)))

    for form in impl:
        call(form)  # warm-up at this size
    assert bytes(outs["host"]) == bytes(outs["device"]), "host and device hashes differ at n = %d" % n
    t = {"host": [], "device": []}
    for _ in range(reps):
        for form in impl:
            t[form].append(timed(lambda: call(form)))
    kern = []
    for _ in range(3):
        eng.set_profiling(True)
        call("device")
        kern.append(eng.stage_time(_lib.STAGE_HASH)[0])
        eng.set_profiling(False)
    row = {"n": n, "host": cell(t["host"]), "device": cell(t["device"]), "device_kernel_ms": cell(kern)}
    for form in impl:
        row[form]["hashes_per_s"] = n / row[form]["median_ms"] * 1e3
    return row


def wins(row):
    h, d = row["host"], row["device"]
    return h["median_ms"] - d["median_ms"] > (h["max_ms"] - h["min_ms"]) + (d["max_ms"] - d["min_ms"])


def threshold(rows):
    """smallest swept size from which DEVICE wins at every larger swept size too; None: nowhere"""
    best = None
    for row in sorted(rows, key=lambda r: -r["n"]):
        if not wins(row):
            break
        best = row["n"]
    return best


def signed_ab(eng, n, reps):
    L = eng._l
    data, offs = messages(n, 7)
    msgs = [data[28 * i:28 * (i + 1)] for i in range(n)]
    rng = random.Random(8)
    sks = [rng.randrange(1, R_ORDER) for _ in range(16)]
    keys = hoststage.g1_mul([G1_GEN] * 16, sks)
    hs = hoststage.hash_g2(msgs)
    sigs = hoststage.g2_mul(hs, [sks[i % 16] for i in range(n)])
    for i in range(0, n, 53):  # forged: another signer's signature
        sigs[i] = sigs[(i + 1) % n]
    want = bytes(0 if i % 53 == 0 else 1 for i in range(n))
    pkb = (ctypes.c_uint8 * (96 * n)).from_buffer_copy(b"".join(keys[i % 16] for i in range(n)))
    sgb = (ctypes.c_uint8 * (192 * n)).from_buffer_copy(b"".join(sigs))
    dbuf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    po = offs.ctypes.data_as(VP)
    hb = (ctypes.c_uint8 * (192 * n))()
    idx = np.arange(n, dtype=np.uint32)
    v = {k: (ctypes.c_uint8 * n)() for k in ("host", "device")}

    def host():
        _lib.check_host(L.hbh_hash_g2(n, ctypes.cast(dbuf, VP), po, ctypes.cast(hb, VP), 0))
        _lib.check(L.hbh_verify_sig_shares(eng.handle, n, ctypes.cast(pkb, VP), ctypes.cast(sgb, VP), ctypes.cast(hb, VP),
                                           n, idx.ctypes.data_as(VP), ctypes.cast(v["host"], VP)))

    def device():
        _lib.check(L.hbh_verify_signatures(eng.handle, n, ctypes.cast(pkb, VP), ctypes.cast(sgb, VP), ctypes.cast(dbuf, VP),
                                           po, ctypes.cast(v["device"], VP)))

    eng.set_hash_impl(_lib.HASH_DEVICE)
    host()
    device()
    assert bytes(v["host"]) == want and bytes(v["device"]) == want, "verdicts differ from the construction"
    t = {"host": [], "device": []}
    for _ in range(reps):
        t["host"].append(timed(host))
        t["device"].append(timed(device))
    return {"n": n, "hash_on_host_then_verify_signatures": cell(t["host"]), "verify_signed_device": cell(t["device"])}


def fmt(c):
    return "%.2f / %.2f / %.2f" % (c["min_ms"], c["median_ms"], c["max_ms"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--signed", type=int, default=10100, help="items of the verify_signed A/B (0: skip)")
    ap.add_argument("--out", default=None, help="directory for hash_bench.json and hash_bench.md")
    a = ap.parse_args()
    eng = Engine(0)
    res = {"host_threads": hoststage.host_threads(), "reps": a.reps, "message_bytes": 28, "rows": []}
    try:
        for n in [int(s) for s in a.sizes.split(",")]:
            row = sweep_size(eng, n, a.reps)
            row["device_wins"] = wins(row)
            res["rows"].append(row)
            print("n %6d  host %s  device %s  kernel %s ms  %s" % (n, fmt(row["host"]), fmt(row["device"]),
                                                                    fmt(row["device_kernel_ms"]),
                                                                    "DEVICE" if row["device_wins"] else "-"), flush=True)
        res["auto_threshold"] = threshold(res["rows"])
        print("AUTO threshold supported by this sweep:", res["auto_threshold"], flush=True)
        if a.signed:
            res["verify_signed"] = s = signed_ab(eng, a.signed, a.reps)
            print("verify_signed n %d  host hash + verify_signatures %s  device %s" %
                  (s["n"], fmt(s["hash_on_host_then_verify_signatures"]), fmt(s["verify_signed_device"])), flush=True)
    finally:
        eng.set_hash_impl(_lib.HASH_AUTO)
        eng.close()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "hash_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        with open(os.path.join(a.out, "hash_bench.md"), "w") as f:
            f.write("| messages | HOST ms (min / median / max) | DEVICE ms (min / median / max) | HASH stage ms | "
                    "HOST hashes/s | DEVICE hashes/s | DEVICE wins |\n|---|---|---|---|---|---|---|\n")
            for r in res["rows"]:
                f.write("| %d | %s | %s | %s | %.0f | %.0f | %s |\n" %
                        (r["n"], fmt(r["host"]), fmt(r["device"]), fmt(r["device_kernel_ms"]), r["host"]["hashes_per_s"],
                         r["device"]["hashes_per_s"], "yes" if r["device_wins"] else "no"))


if __name__ == "__main__":
    main()
