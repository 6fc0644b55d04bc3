"""The grouped share checks against the per-share calls (hbh_verify_*_shares_grouped vs hbh_verify_*_shares):
the two calls alternate in one process on the same inputs, after a warm-up, at three drain shapes and
three validity mixes (all valid; 1 % and 10 % of the groups holding one bad share, at least one group).
Two passes per cell: host-to-host wall time of the synchronous calls with profiling off, then the stage
split of the grouped call with profiling on -- HBH_STAGE_CURVE (the group sums), HBH_STAGE_PREPARE +
HBH_STAGE_PAIRING of the whole call, and of that the fallback's share, measured as the same stages of
the per-share call on exactly the items the grouped call re-checks.  Verdicts of the two calls are
compared before anything is timed.

    python tools/grouped_bench.py --reps 7 --out profiles/r16

writes grouped_bench.json (every sample) and grouped_bench.md (min / median / max per cell).

--sum-impl chain|bucket forces that form of the group sums (hbh_engine_set_group_sum_impl) for the grouped
call; --sum-impl both runs the grouped call under each form in turn in this process, cell by cell (one
more column per form), and adds a sweep of the sums alone: hbh_dbg_group_sums on the G1 points and on the
G2 points of each signature shape, one side per call, under each form alternately with profiling on --
the HBH_STAGE_CURVE time per kind of sum and form that the AUTO thresholds are decided from (the rule of
include/hbbft_hip.h: the smallest swept size from which BUCKET's median is below CHAIN's by more than both
cells' min-max spread, at that and every larger swept size).  The JSON is then {"cells", "sums", "auto"}.

    python tools/grouped_bench.py --sum-impl both --reps 7 --out profiles/r17

--scalar-form digits runs the grouped call under the digit form of its scalars
(hbh_engine_set_group_scalar_form: X4 for signature shares, X2 for decryption shares; its own sum kernels);
--scalar-form both runs it under the INT128 and the digit form in turn in this process, cell by cell, one
more column per form, and judges each cell: the digit form WINS against a yardstick (the INT128 grouped
call, the per-share call) when its median wall time is below the yardstick's by more than both cells'
min-max spread, LOSES when it is above by more than both, TIES otherwise.  Not combined with --sum-impl
(which governs the INT128 form only).

    python tools/grouped_bench.py --scalar-form both --reps 7 --out profiles/r22"""
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
from hbbft_amd._lib import (GSCALAR_DIGITS, GSCALAR_INT128, GSUM_AUTO, GSUM_BUCKET, GSUM_CHAIN, STAGE_CURVE,  # noqa: E402
                            STAGE_PAIRING, STAGE_PREPARE)
from hbbft_amd.engine import Engine, g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a  # noqa: E402

R = C.R
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
SHAPES = [  # (kind, shares, groups)
    ("sign", 65536, 1024),   # BASELINE configs[1]: 1,024 documents of 64 shares
    ("sign", 10000, 100),    # an epoch's coins: 100 documents of 100 shares
    ("sign", 512, 8),
    ("decrypt", 65536, 1024),
    ("decrypt", 10000, 100),
]
# (column, (form of the group sums, form of the scalars)) of each grouped call of a cell
FORMS = {None: [("grouped", (GSUM_AUTO, GSCALAR_INT128))], "chain": [("grouped", (GSUM_CHAIN, GSCALAR_INT128))],
         "bucket": [("grouped", (GSUM_BUCKET, GSCALAR_INT128))],
         "both": [("grouped_chain", (GSUM_CHAIN, GSCALAR_INT128)), ("grouped_bucket", (GSUM_BUCKET, GSCALAR_INT128))]}
SCALAR_FORMS = {"int128": [("grouped", (GSUM_AUTO, GSCALAR_INT128))], "digits": [("grouped", (GSUM_AUTO, GSCALAR_DIGITS))],
                "both": [("grouped_int128", (GSUM_AUTO, GSCALAR_INT128)), ("grouped_digits", (GSUM_AUTO, GSCALAR_DIGITS))]}
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


def measure(eng, kind, n, ngroups, mix, frac, reps, rng, forms):
    nbad = 0 if frac == 0 else max(1, round(frac * ngroups))
    bad = sorted(rng.sample(range(ngroups), nbad))
    inp = inputs(eng, rng, kind, n, ngroups, bad)
    plain = (eng.verify_sig_shares if kind == "sign" else eng.verify_dec_shares)
    grouped_call = (eng.verify_sig_shares_grouped if kind == "sign" else eng.verify_dec_shares_grouped)
    args = inp["args"]

    def grouped(impl):
        eng.set_group_sum_impl(impl[0])
        eng.set_group_scalar_form(impl[1])
        try:
            return grouped_call(*args)
        finally:
            eng.set_group_sum_impl(GSUM_AUTO)
            eng.set_group_scalar_form(GSCALAR_INT128)

    want = plain(*args)  # first calls: verdicts, and the warm-up of every path
    assert want == inp["want"], "verdicts differ"
    for _, impl in forms:
        got, stats = grouped(impl)
        assert got == want, "verdicts differ"
        assert (stats.groups == ngroups and stats.groups_passed == ngroups - nbad
                and stats.fallback_items == nbad * (n // ngroups))
    for _ in range(2):
        plain(*args)
        for _, impl in forms:
            grouped(impl)
    wall = {name: [] for name in ["per_share"] + [f for f, _ in forms]}
    for _ in range(reps):
        for name, fn in [("per_share", lambda: plain(*args))] + [(f, lambda i=i: grouped(i)) for f, i in forms]:
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    bad_set = set(bad)
    fallback = [i for i in range(n) if inp["grp"][i] in bad_set]
    fargs = subset(kind, inp, fallback) if fallback else None
    split = {"pairing_fallback": [], "per_share_pairing": []}
    for f, _ in forms:
        split["curve" + f[len("grouped"):]] = []
        split["pairing_all" + f[len("grouped"):]] = []
    for _ in range(reps):
        for f, impl in forms:
            c, p = stages(eng, lambda: grouped(impl))
            split["curve" + f[len("grouped"):]].append(c)
            split["pairing_all" + f[len("grouped"):]].append(p)
        split["pairing_fallback"].append(stages(eng, lambda: plain(*fargs))[1] if fargs else 0.0)
        split["per_share_pairing"].append(stages(eng, lambda: plain(*args))[1])
    row = dict(kind=kind, shares=n, groups=ngroups, mix=mix, bad_groups=nbad, fallback_items=stats.fallback_items,
               wall_ms={k: cell(v) for k, v in wall.items()}, device_ms={k: cell(v) for k, v in split.items()})
    for f, _ in forms:
        row["ratio_median" + f[len("grouped"):]] = row["wall_ms"]["per_share"]["median"] / row["wall_ms"][f]["median"]
    return row, inp


def sums_alone(eng, inp, n, ngroups, reps, rng):
    """HBH_STAGE_CURVE ms of hbh_dbg_group_sums on one side (the G1 points, then the G2 points of a
    signature shape) under each form: bytes compared first, two warm-ups each, then reps alternations."""
    pks, sigs, _, grp = inp["args"]
    scalars = bytes(rng.getrandbits(8) for _ in range(16 * n))
    out = []
    for kind, pts in (("g1", (pks, None)), ("g2", (None, sigs))):
        def run(impl):
            eng.set_group_sum_impl(impl)
            try:
                return eng.dbg_group_sums(pts[0], pts[1], ngroups, grp, scalars)
            finally:
                eng.set_group_sum_impl(GSUM_AUTO)
        assert run(GSUM_CHAIN) == run(GSUM_BUCKET), "sums differ"
        for _ in range(2):
            run(GSUM_CHAIN)
            run(GSUM_BUCKET)
        t = {"chain": [], "bucket": []}
        for _ in range(reps):
            for name, impl in (("chain", GSUM_CHAIN), ("bucket", GSUM_BUCKET)):
                t[name].append(stages(eng, lambda: run(impl))[0])
        out.append(dict(kind=kind, items=n, groups=ngroups, curve_ms={k: cell(v) for k, v in t.items()}))
    return out


def auto_thresholds(sums):
    """Per kind of sum: the smallest swept size from which BUCKET's median CURVE time is below CHAIN's by
    more than both cells' min-max spread, at that and every larger swept size; 0 when no size qualifies."""
    auto = {}
    for kind in ("g1", "g2"):
        rows = sorted((r for r in sums if r["kind"] == kind), key=lambda r: r["items"])
        thr = 0
        for r in reversed(rows):
            c, b = r["curve_ms"]["chain"], r["curve_ms"]["bucket"]
            gain = c["median"] - b["median"]
            r["bucket_wins"] = bool(gain > c["max"] - c["min"] and gain > b["max"] - b["min"])
            if not r["bucket_wins"]:
                break
            thr = r["items"]
        for r in rows:  # the sizes below the break are judged too, for the record
            if "bucket_wins" not in r:
                c, b = r["curve_ms"]["chain"], r["curve_ms"]["bucket"]
                gain = c["median"] - b["median"]
                r["bucket_wins"] = bool(gain > c["max"] - c["min"] and gain > b["max"] - b["min"])
        auto[kind] = thr
    return auto


def fmt(c):
    return "%.2f / %.2f / %.2f" % (c["min"], c["median"], c["max"])


def judge(new, old):
    """'wins' / 'loses' when the medians differ by more than both cells' min-max spread, else 'ties'"""
    gain = old["median"] - new["median"]
    spread = max(new["max"] - new["min"], old["max"] - old["min"])
    return "wins" if gain > spread else "loses" if -gain > spread else "ties"


def judged_table(rows):
    """--scalar-form both: the digit form against the INT128 grouped call and the per-share call"""
    out = ["| shape | mix | INT128 / digits (medians) | digits vs INT128, beyond the spread | per-share / digits (medians) "
           "| digits vs per-share, beyond the spread | CURVE ms INT128 / digits (medians) |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        w, d = r["wall_ms"], r["device_ms"]
        r["digits_vs_int128"] = judge(w["grouped_digits"], w["grouped_int128"])
        r["digits_vs_per_share"] = judge(w["grouped_digits"], w["per_share"])
        out.append("| %s %d in %d | %s | %.2f | %s | %.2f | %s | %.2f / %.2f |" % (
            r["kind"], r["shares"], r["groups"], r["mix"], w["grouped_int128"]["median"] / w["grouped_digits"]["median"],
            r["digits_vs_int128"], w["per_share"]["median"] / w["grouped_digits"]["median"], r["digits_vs_per_share"],
            d["curve_int128"]["median"], d["curve_digits"]["median"]))
    return "\n".join(out) + "\n"


def table(rows, forms):
    tails = [f[len("grouped"):] for f, _ in forms]
    head = ["shape", "mix", "fallback items", "per-share wall ms"]
    head += ["%s wall ms" % f.replace("_", ", ") for f, _ in forms]
    head += ["per-share / %s (medians)" % f.replace("_", ", ") for f, _ in forms]
    head += ["%s: CURVE ms" % f.replace("_", ", ") for f, _ in forms]
    head += ["%s: PREPARE + PAIRING ms" % f.replace("_", ", ") for f, _ in forms]
    head += ["of which fallback ms", "per-share: PREPARE + PAIRING ms"]
    out = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in rows:
        w, d = r["wall_ms"], r["device_ms"]
        col = ["%s %d in %d" % (r["kind"], r["shares"], r["groups"]), r["mix"], "%d" % r["fallback_items"],
               fmt(w["per_share"])]
        col += [fmt(w[f]) for f, _ in forms]
        col += ["%.2f" % r["ratio_median" + t] for t in tails]
        col += [fmt(d["curve" + t]) for t in tails]
        col += [fmt(d["pairing_all" + t]) for t in tails]
        col += [fmt(d["pairing_fallback"]), fmt(d["per_share_pairing"])]
        out.append("| " + " | ".join(col) + " |")
    return "\n".join(out) + "\n"


def sums_table(sums, auto):
    out = ["| sum | items in groups | CHAIN: CURVE ms | BUCKET: CURVE ms | BUCKET wins beyond both spreads |", "|---|---|---|---|---|"]
    for r in sums:
        out.append("| %s | %d in %d | %s | %s | %s |" % (r["kind"], r["items"], r["groups"], fmt(r["curve_ms"]["chain"]),
                                                      fmt(r["curve_ms"]["bucket"]), "yes" if r["bucket_wins"] else "no"))
    out.append("")
    out.append("AUTO by the rule: HBH_AUTO_GSUM_G1_BUCKET_MIN %d, HBH_AUTO_GSUM_G2_BUCKET_MIN %d (0: never)"
               % (auto["g1"], auto["g2"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternations per cell (>= 5)")
    ap.add_argument("--out", default=None, help="directory for grouped_bench.json and grouped_bench.md")
    ap.add_argument("--only", type=int, default=None, help="index of one shape (rehearsal)")
    ap.add_argument("--sum-impl", choices=["chain", "bucket", "both"], default=None,
                    help="form of the group sums (default: the engine's AUTO)")
    ap.add_argument("--scalar-form", choices=["int128", "digits", "both"], default=None,
                    help="form of the grouped call's scalars (default: int128)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.sum_impl and a.scalar_form:
        ap.error("--sum-impl governs the INT128 form only: not combined with --scalar-form")
    forms = SCALAR_FORMS[a.scalar_form] if a.scalar_form else FORMS[a.sum_impl]
    eng = Engine(0)
    rng = random.Random(16)
    rows, sums = [], []
    for k, (kind, n, ngroups) in enumerate(SHAPES):
        if a.only is not None and k != a.only:
            continue
        for mix, frac in MIXES:
            row, inp = measure(eng, kind, n, ngroups, mix, frac, a.reps, rng, forms)
            rows.append(row)
            print(json.dumps({k_: v for k_, v in row.items() if k_ not in ("wall_ms", "device_ms")}), flush=True)
            if a.sum_impl == "both" and kind == "sign" and frac == 0.0:
                sums += sums_alone(eng, inp, n, ngroups, a.reps, rng)
                print(json.dumps([{k_: v for k_, v in r.items() if k_ != "curve_ms"} for r in sums[-2:]]), flush=True)
    eng.close()
    md = "min / median / max of %d alternated runs per cell\n\n" % a.reps + table(rows, forms)
    doc = rows
    if a.scalar_form == "both":
        md += "\nThe digit form against its yardsticks (wall time; wins / loses: beyond both cells' min-max spread)\n\n"
        md += judged_table(rows)
    if a.sum_impl == "both":
        auto = auto_thresholds(sums)
        md += "\nThe sums alone (hbh_dbg_group_sums, one side per call; device ms under HBH_STAGE_CURVE)\n\n" + sums_table(sums, auto)
        doc = {"cells": rows, "sums": sums, "auto": auto}
    print(md)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "grouped_bench.json"), "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        with open(os.path.join(a.out, "grouped_bench.md"), "w") as f:
            f.write(md)


if __name__ == "__main__":
    main()
