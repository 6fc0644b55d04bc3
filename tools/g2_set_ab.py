"""A/B of the resident G2 set against the stateless calls (hbh_verify_*_set vs hbh_verify_*): the two
calls alternate in one process on the same inputs, at the sizes of DESIGN §4's drains.  The shared
points are added to the set once, outside the timed region; the cost of that add is timed on its
own.  Two passes per workload: host-to-host wall time of the synchronous call with profiling off,
then the per-stage device time (HBH_STAGE_PREPARE, HBH_STAGE_PAIRING) with profiling on.  Verdicts
of the two calls are compared before anything is timed.

    python tools/g2_set_ab.py --reps 12 --out profiles/r12

writes g2_set_ab.json (every sample) and g2_set_ab.md (min / median / max per cell)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import bls12_381 as C  # noqa: E402
from hbbft_amd._lib import IMPL_AUTO, IMPL_WAVEP, STAGE_PAIRING, STAGE_PREPARE  # noqa: E402
from hbbft_amd.engine import Engine, g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a  # noqa: E402

R = C.R
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
WORKLOADS = [  # (kind, checks, shared points, the path AUTO takes, or the forced implementation)
    ("sign", 6144, 100, "OCT", IMPL_AUTO),
    ("sign", 16384, 256, "QUAD", IMPL_AUTO),
    ("decrypt", 256, 8, "WAVE2: TT against walk", IMPL_AUTO),
    ("decrypt", 800, 16, "WAVE: TT against walk", IMPL_AUTO),
    ("decrypt", 6144, 100, "OCT, two tables", IMPL_AUTO),
    ("decrypt", 800, 16, "WAVEP (forced): TT against walk", IMPL_WAVEP),  # AUTO never takes WAVEP below 1,025
]


def u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


def sign_inputs(eng, rng, n, ndocs, nodes=64):
    """n share checks spread over ndocs documents, 1 in 53 forged; points joined once into bytes"""
    sks = [rng.randrange(1, R) for _ in range(nodes)]
    pks = eng.g1_mul([G1] * nodes, sks)
    hashes = eng.g2_mul([G2] * ndocs, [rng.randrange(1, R) for _ in range(ndocs)])
    doc = [i % ndocs for i in range(n)]
    sigs = eng.g2_mul([hashes[d] for d in doc], [rng.randrange(1, R) if i % 53 == 7 else sks[i % nodes] for i in range(n)])
    want = bytes(0 if i % 53 == 7 else 1 for i in range(n))
    return dict(a=b"".join(pks[i % nodes] for i in range(n)), b=b"".join(sigs), points=hashes, idx=doc, want=want)


def decrypt_inputs(eng, rng, n, ncts, nodes=64):
    sks = [rng.randrange(1, R) for _ in range(nodes)]
    pks = eng.g1_mul([G1] * nodes, sks)
    rs = [rng.randrange(1, R) for _ in range(ncts)]
    hh = [rng.randrange(1, R) for _ in range(ncts)]
    us = eng.g1_mul([G1] * ncts, rs)
    huv = eng.g2_mul([G2] * ncts, hh)
    ws = eng.g2_mul([G2] * ncts, [h * r % R for h, r in zip(hh, rs)])
    ct = [i % ncts for i in range(n)]
    shares = eng.g1_mul([us[c] for c in ct], [rng.randrange(1, R) if i % 53 == 7 else sks[i % nodes] for i in range(n)])
    want = bytes(0 if i % 53 == 7 else 1 for i in range(n))
    return dict(a=b"".join(shares), b=b"".join(pks[i % nodes] for i in range(n)), points=huv + ws, idx=ct, want=want)


def calls(eng, kind, inp, gs, slots):
    """(stateless call, set call) as closures over prepared arguments"""
    idx = u32(inp["idx"])
    if kind == "sign":
        hb = b"".join(inp["points"])
        sl = u32([slots[d] for d in inp["idx"]])
        return (lambda: eng.verify_sig_shares(inp["a"], inp["b"], hb, idx),
                lambda: eng.verify_sig_shares_set(inp["a"], inp["b"], gs, sl))
    ncts = len(inp["points"]) // 2
    hb, wb = b"".join(inp["points"][:ncts]), b"".join(inp["points"][ncts:])
    hs, ws = u32([slots[c] for c in inp["idx"]]), u32([slots[ncts + c] for c in inp["idx"]])
    return (lambda: eng.verify_dec_shares(inp["a"], inp["b"], hb, wb, idx),
            lambda: eng.verify_dec_shares_set(inp["a"], inp["b"], gs, hs, ws))


def cell(samples):
    return {"min": min(samples), "median": statistics.median(samples), "max": max(samples), "samples": samples}


def measure(eng, kind, n, npts, path, impl, reps, rng):
    eng.set_pairing_impl(impl)
    inp = (sign_inputs if kind == "sign" else decrypt_inputs)(eng, rng, n, npts)
    gs = eng.g2_set(len(inp["points"]))
    # the add, timed on its own: the first fills the set, the others refill it after a release
    add_ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        slots = gs.add(inp["points"])
        add_ms.append((time.perf_counter() - t0) * 1e3)
        if len(add_ms) < reps:
            gs.release(slots)
    stateless, resident = calls(eng, kind, inp, gs, slots)
    for _ in range(2):  # warm both shapes; the verdicts must agree before a time means anything
        assert stateless() == inp["want"], "stateless verdicts differ from the construction"
        assert resident() == inp["want"], "set verdicts differ from the construction"
    wall = {"stateless": [], "set": []}
    for _ in range(reps):
        for name, fn in (("stateless", stateless), ("set", resident)):
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    stage = {name: {"prepare_ms": [], "pairing_ms": [], "prepare_launches": []} for name in wall}
    for _ in range(reps):
        for name, fn in (("stateless", stateless), ("set", resident)):
            eng.set_profiling(True)  # resets the counts
            fn()
            prep, pair = eng.stage_time(STAGE_PREPARE), eng.stage_time(STAGE_PAIRING)
            stage[name]["prepare_ms"].append(prep[0])
            stage[name]["prepare_launches"].append(prep[1])
            stage[name]["pairing_ms"].append(pair[0])
    eng.set_profiling(False)
    eng.set_pairing_impl(IMPL_AUTO)
    gs.close()
    return {"workload": kind, "checks": n, "shared_points": npts, "set_slots": len(inp["points"]), "path": path,
            "add_host_ms": cell(add_ms),
            "host_ms": {k: cell(v) for k, v in wall.items()},
            "prepare_ms": {k: cell(v["prepare_ms"]) for k, v in stage.items()},
            "pairing_ms": {k: cell(v["pairing_ms"]) for k, v in stage.items()},
            "prepare_launches": {k: sorted(set(v["prepare_launches"])) for k, v in stage.items()}}


def fmt(c):
    return "%.3f / %.3f / %.3f" % (c["min"], c["median"], c["max"])


def table(rows):
    out = ["| Workload | Checks | Shared points | Path | Call | host-to-host ms (min / median / max) | PREPARE ms | PREPARE launches | PAIRING ms | add, host ms |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for name in ("stateless", "set"):
            out.append("| %s | %d | %d | %s | %s | %s | %s | %s | %s | %s |" % (
                r["workload"], r["checks"], r["shared_points"], r["path"], name, fmt(r["host_ms"][name]),
                fmt(r["prepare_ms"][name]), r["prepare_launches"][name], fmt(r["pairing_ms"][name]),
                fmt(r["add_host_ms"]) if name == "set" else ""))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12, help="alternations per cell (>= 10)")
    ap.add_argument("--out", default=None, help="directory for g2_set_ab.json and g2_set_ab.md")
    ap.add_argument("--only", type=int, default=None, help="index of one workload (rehearsal)")
    a = ap.parse_args()
    eng = Engine(0)
    rng = random.Random(12)
    rows = []
    for k, (kind, n, npts, path, impl) in enumerate(WORKLOADS):
        if a.only is not None and k != a.only:
            continue
        rows.append(measure(eng, kind, n, npts, path, impl, a.reps, rng))
        print(json.dumps({k_: v for k_, v in rows[-1].items() if k_ in ("workload", "checks", "path")}), flush=True)
        if a.out:  # after every workload: a cut-short run keeps what it measured
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "g2_set_ab.json"), "w") as f:
                json.dump({"reps": a.reps, "rows": rows}, f, indent=1)
            with open(os.path.join(a.out, "g2_set_ab.md"), "w") as f:
                f.write(table(rows))
    print(table(rows))
    eng.close()


if __name__ == "__main__":
    main()
