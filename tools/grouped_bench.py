"""The grouped share checks against the per-share calls (hbh_verify_*_shares_grouped vs hbh_verify_*_shares):
the two calls alternate in one process on the same inputs, after a warm-up, at three drain shapes and
three validity mixes (all valid; 1 % and 10 % of the groups holding one bad share, at least one group).
Two passes per cell: host-to-host wall time of the synchronous calls with profiling off, then the stage
split of the grouped call with profiling on -- HBH_STAGE_CURVE (the group sums), HBH_STAGE_PREPARE +
HBH_STAGE_PAIRING of the whole call, and of that the fallback's share, measured as the same stages of
the per-share call on exactly the items the grouped call re-checks.  Verdicts of the two calls are
compared before anything is timed.

    python tools/grouped_bench.py --reps 7 --out profiles/r16

writes grouped_bench.json (every sample) and grouped_bench.md (min / median / max per cell)."""
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
from hbbft_amd._lib import STAGE_CURVE, STAGE_PAIRING, STAGE_PREPARE  # noqa: E402
from hbbft_amd.engine import Engine, g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a  # noqa: E402

R = C.R
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
SHAPES = [  # (kind, shares, groups)
    ("sign", 65536, 1024),   # BASELINE configs[1]: 1,024 documents of 64 shares
    ("sign", 10000, 100),    # an epoch's coins: 100 documents of 100 shares
    ("sign", 512, 8),
    ("decrypt", 65536, 1024),
]
MIXES = [("all valid", 0.0), ("1 % of groups bad", 0.01), ("10 % of groups bad", 0.10)]


def u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


def inputs(eng, rng, kind, n, ngroups, bad_groups, nodes=128):
    """n shares, item i in group i % ngroups (interleaved), from node (i // ngroups) % nodes; the first
    share of each group in bad_groups is another node's.  Points joined once into bytes."""
    sks = [rng.randrange(1, R) for _ in range(nodes)]
    pks = eng.g1_mul_gen(sks)
    grp = [i % ngroups for i in range(n)]
    node = [(i // ngroups) % nodes for i in range(n)]
    forged = {g for g in bad_groups}  # item g (< ngroups) is the first share of group g
    key = [sks[(node[i] + 1) % nodes] if i in forged else sks[node[i]] for i in range(n)]
    want = bytes(0 if i in forged else 1 for i in range(n))
    pkb = b"".join(pks[k] for k in node)
    if kind == "sign":
        hashes = eng.g2_mul([G2] * ngroups, [rng.randrange(1, R) for _ in range(ngroups)])
        sigs = eng.g2_mul([hashes[g] for g in grp], key)
        return dict(args=(pkb, b"".join(sigs), b"".join(hashes), u32(grp)), want=want, grp=grp)
    rs = [rng.randrange(1, R) for _ in range(ngroups)]
    hh = [rng.randrange(1, R) for _ in range(ngroups)]
    us = eng.g1_mul_gen(rs)
    huv = eng.g2_mul([G2] * ngroups, hh)
    ws = eng.g2_mul([G2] * ngroups, [h * r % R for h, r in zip(hh, rs)])
    shares = eng.g1_mul([us[g] for g in grp], key)
    return dict(args=(b"".join(shares), pkb, b"".join(huv), b"".join(ws), u32(grp)), want=want, grp=grp)


def subset(kind, inp, keep):
    """the per-share call's arguments for the items in keep"""
    a, b = inp["args"][0], inp["args"][1]
    sa = 96
    sb = 192 if kind == "sign" else 96
    pick = lambda raw, size: b"".join(raw[i * size:(i + 1) * size] for i in keep)  # noqa: E731
    return (pick(a, sa), pick(b, sb)) + tuple(inp["args"][2:-1]) + (u32([inp["grp"][i] for i in keep]),)


def cell(samples):
    return {"min": min(samples), "median": statistics.median(samples), "max": max(samples), "samples": samples}


def stages(eng, fn):
    """(CURVE ms, PREPARE + PAIRING ms) of one profiled call"""
    eng.set_profiling(True)
    fn()
    t = [eng.stage_time(s)[0] for s in (STAGE_CURVE, STAGE_PREPARE, STAGE_PAIRING)]
    eng.set_profiling(False)
    return t[0], t[1] + t[2]


def measure(eng, kind, n, ngroups, mix, frac, reps, rng):
    nbad = 0 if frac == 0 else max(1, round(frac * ngroups))
    bad = sorted(rng.sample(range(ngroups), nbad))
    inp = inputs(eng, rng, kind, n, ngroups, bad)
    plain = (eng.verify_sig_shares if kind == "sign" else eng.verify_dec_shares)
    grouped = (eng.verify_sig_shares_grouped if kind == "sign" else eng.verify_dec_shares_grouped)
    args = inp["args"]
    got, stats = grouped(*args)  # first calls: verdicts, and the warm-up of both paths
    assert plain(*args) == inp["want"] == got, "verdicts differ"
    assert stats.groups == ngroups and stats.groups_passed == ngroups - nbad and stats.fallback_items == nbad * (n // ngroups)
    for _ in range(2):
        plain(*args)
        grouped(*args)
    wall = {"per_share": [], "grouped": []}
    for _ in range(reps):
        for name, fn in (("per_share", plain), ("grouped", grouped)):
            t0 = time.perf_counter()
            fn(*args)
            wall[name].append((time.perf_counter() - t0) * 1e3)
    bad_set = set(bad)
    fallback = [i for i in range(n) if inp["grp"][i] in bad_set]
    fargs = subset(kind, inp, fallback) if fallback else None
    split = {"curve": [], "pairing_all": [], "pairing_fallback": [], "per_share_pairing": []}
    for _ in range(reps):
        c, p = stages(eng, lambda: grouped(*args))
        split["curve"].append(c)
        split["pairing_all"].append(p)
        split["pairing_fallback"].append(stages(eng, lambda: plain(*fargs))[1] if fargs else 0.0)
        split["per_share_pairing"].append(stages(eng, lambda: plain(*args))[1])
    row = dict(kind=kind, shares=n, groups=ngroups, mix=mix, bad_groups=nbad, fallback_items=stats.fallback_items,
               wall_ms={k: cell(v) for k, v in wall.items()}, device_ms={k: cell(v) for k, v in split.items()})
    row["ratio_median"] = row["wall_ms"]["per_share"]["median"] / row["wall_ms"]["grouped"]["median"]
    return row


def fmt(c):
    return "%.2f / %.2f / %.2f" % (c["min"], c["median"], c["max"])


def table(rows):
    out = ["| shape | mix | fallback items | per-share wall ms | grouped wall ms | per-share / grouped (medians) | "
           "grouped: CURVE ms | grouped: PREPARE + PAIRING ms | of which fallback ms | per-share: PREPARE + PAIRING ms |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        w, d = r["wall_ms"], r["device_ms"]
        out.append("| %s %d in %d | %s | %d | %s | %s | %.2f | %s | %s | %s | %s |" % (
            r["kind"], r["shares"], r["groups"], r["mix"], r["fallback_items"], fmt(w["per_share"]), fmt(w["grouped"]),
            r["ratio_median"], fmt(d["curve"]), fmt(d["pairing_all"]), fmt(d["pairing_fallback"]),
            fmt(d["per_share_pairing"])))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternations per cell (>= 5)")
    ap.add_argument("--out", default=None, help="directory for grouped_bench.json and grouped_bench.md")
    ap.add_argument("--only", type=int, default=None, help="index of one shape (rehearsal)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    eng = Engine(0)
    rng = random.Random(16)
    rows = []
    for k, (kind, n, ngroups) in enumerate(SHAPES):
        if a.only is not None and k != a.only:
            continue
        for mix, frac in MIXES:
            rows.append(measure(eng, kind, n, ngroups, mix, frac, a.reps, rng))
            print(json.dumps({k_: v for k_, v in rows[-1].items() if k_ not in ("wall_ms", "device_ms")}), flush=True)
    eng.close()
    md = "min / median / max of %d alternated runs per cell\n\n" % a.reps + table(rows)
    print(md)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "grouped_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
        with open(os.path.join(a.out, "grouped_bench.md"), "w") as f:
            f.write(md)


if __name__ == "__main__":
    main()
