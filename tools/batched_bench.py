"""The batched independent checks against the unbatched calls (hbh_verify_signatures_batched vs
hbh_verify_signatures, hbh_verify_ciphertexts_uv_batched vs hbh_verify_ciphertexts_uv): the calls alternate
in one process on the same inputs, after a warm-up, at 1,024, 10,100 and 65,536 items and three validity
mixes (all valid; 1 % and 10 % of the 256-item groups holding one bad item, at least one group -- at few
groups that is more than the nominal share, so every row prints the groups it really made bad).  The
batched call runs under the forced widths PAIR, QUAD and OCT of its Miller-product kernel and under AUTO;
the unbatched call under AUTO.  A forced width is the engine's pairing implementation, so it also governs
the per-item FALLBACK of a failed group: the pair / quad / oct rows of a mix with bad groups measure the
Miller product AND a fallback forced to that kernel.  Only the all-valid rows separate the widths; the
auto rows are what a caller gets.  The unbatched calls are untouched by the batched feature, so this build's
are the parent commit's: the yardstick runs on the same box in the same process.

Two passes per cell: host-to-host wall time of the synchronous calls with profiling off, then the stage split
with profiling on -- HBH_STAGE_HASH, HBH_STAGE_CURVE (scaling and sums), HBH_STAGE_PREPARE + HBH_STAGE_PAIRING
(Miller product, closing pair, final exponentiation, fallback).  Verdicts and statistics are checked
before anything is timed.  For every all-valid cell the G2 group sum is also timed alone
(hbh_dbg_group_sums_form, X4, the same groups: HBH_STAGE_CURVE of that call), which splits the batched call's
CURVE stage into the sum and the rest (the per-item G1 scaling).  A form WINS at a cell when the other's median exceeds its own by more than both
cells' min-max spreads together, LOSES in the mirrored case, TIES otherwise.

    python tools/batched_bench.py --reps 7 --out profiles/r25

writes batched_bench.json (every sample) and batched_bench.md (min / median / max per cell)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import bls12_381 as C  # noqa: E402
from hbbft_amd import hoststage  # noqa: E402
from hbbft_amd._lib import (GFORM_X4, IMPL_AUTO, IMPL_OCT, IMPL_PAIR, IMPL_QUAD, STAGE_CURVE, STAGE_HASH, STAGE_PAIRING,  # noqa: E402
                            STAGE_PREPARE)
from hbbft_amd.engine import Engine  # noqa: E402

R = C.R
GROUP = 256
SIZES = [1024, 10100, 65536]
MIXES = [("all valid", 0.0), ("1 % of groups bad", 0.01), ("10 % of groups bad", 0.10)]
WIDTHS = [("pair", IMPL_PAIR), ("quad", IMPL_QUAD), ("oct", IMPL_OCT), ("auto", IMPL_AUTO)]


def inputs(eng, rng, kind, n, bad_groups, keys=128):
    """n items made on the engine and the host stage; the first item of each group in bad_groups carries its
    neighbour's signature / W.  (arguments of both calls, expected verdicts)"""
    msgs = [b"item %d of %d: %d" % (i, n, rng.getrandbits(64)) for i in range(n)]
    bad = {g * GROUP for g in bad_groups}
    want = bytes(0 if i in bad else 1 for i in range(n))
    if kind == "sig":
        sks = [rng.randrange(1, R) for _ in range(keys)]
        pks = eng.g1_mul_gen(sks)
        sigs = eng.g2_mul(eng.hash_g2(msgs), [sks[i % keys] for i in range(n)])
        for i in bad:
            sigs[i] = sigs[i + 1]
        return ([pks[i % keys] for i in range(n)], sigs, msgs), want
    pk = eng.g1_mul_gen([rng.randrange(1, R)])[0]
    cts = hoststage.encrypt([pk] * n, [m[:32].ljust(32, b".") for m in msgs], [rng.randrange(1, R) for _ in range(n)])
    us, vs, ws = [c[0] for c in cts], [c[1] for c in cts], [c[2] for c in cts]
    for i in bad:
        ws[i] = ws[i + 1]
    return (us, vs, ws), want


def cell(samples):
    return {"min": min(samples), "median": statistics.median(samples), "max": max(samples), "samples": samples}


def judge(new, old):
    gain = old["median"] - new["median"]
    spread = (new["max"] - new["min"]) + (old["max"] - old["min"])
    return "wins" if gain > spread else "loses" if -gain > spread else "ties"


def stages(eng, fn):
    """{stage: device ms} of one profiled call"""
    eng.set_profiling(True)
    fn()
    t = {"hash": eng.stage_time(STAGE_HASH)[0], "curve": eng.stage_time(STAGE_CURVE)[0],
         "pairing": eng.stage_time(STAGE_PREPARE)[0] + eng.stage_time(STAGE_PAIRING)[0]}
    eng.set_profiling(False)
    return t


def measure(eng, kind, n, mix, frac, reps, rng):
    ngroups = (n + GROUP - 1) // GROUP - (1 if n % GROUP == 1 else 0)
    nbad = 0 if frac == 0 else max(1, round(frac * ngroups))
    bad = sorted(rng.sample(range(n // GROUP), nbad))  # full groups only
    args, want = inputs(eng, rng, kind, n, bad)
    plain = eng.verify_signed if kind == "sig" else eng.verify_ciphertexts_uv
    batched_call = eng.verify_signed_batched if kind == "sig" else eng.verify_ciphertexts_uv_batched

    def batched(impl):
        eng.set_pairing_impl(impl)
        try:
            return batched_call(*args)
        finally:
            eng.set_pairing_impl(IMPL_AUTO)

    assert plain(*args) == want, "verdicts differ"  # first calls: verdicts, and the warm-up of every path
    for _, impl in WIDTHS:
        got, stats = batched(impl)
        assert got == want, "verdicts differ"
        assert (stats.groups, stats.groups_passed, stats.fallback_items) == (ngroups, ngroups - nbad, nbad * GROUP), stats
    for _ in range(2):
        plain(*args)
        for _, impl in WIDTHS:
            batched(impl)
    runs = [("unbatched", lambda: plain(*args))] + [(name, lambda i=impl: batched(i)) for name, impl in WIDTHS]
    wall = {name: [] for name, _ in runs}
    for _ in range(reps):
        for name, fn in runs:
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    split = {name: {"hash": [], "curve": [], "pairing": []} for name, _ in runs}
    for _ in range(reps):
        for name, fn in runs:
            for k, v in stages(eng, fn).items():
                split[name][k].append(v)
    g2_alone = []
    if nbad == 0:  # the G2 sum of the same groups on its own: what is left of CURVE is the G1 scaling
        grp = [i // GROUP for i in range(n)]
        scalars = bytes(rng.getrandbits(8) | 1 for _ in range(16 * n))
        sum_alone = lambda: eng.dbg_group_sums_form(GFORM_X4, None, args[1] if kind == "sig" else args[2],  # noqa: E731
                                                    (n + GROUP - 1) // GROUP, grp, scalars)
        sum_alone()
        g2_alone = [stages(eng, sum_alone)["curve"] for _ in range(reps)]
    mix = "%s (%d of %d)" % (mix, nbad, ngroups)
    row = dict(kind=kind, items=n, mix=mix, groups=ngroups, bad_groups=nbad, fallback_items=nbad * GROUP,
               g2_sum_alone_ms=cell(g2_alone) if g2_alone else None,
               wall_ms={k: cell(v) for k, v in wall.items()},
               device_ms={k: {s: cell(v) for s, v in d.items()} for k, d in split.items()})
    row["verdict"] = {name: judge(row["wall_ms"][name], row["wall_ms"]["unbatched"]) for name, _ in WIDTHS}
    row["pairing_verdict"] = {name: judge(row["device_ms"][name]["pairing"], row["device_ms"]["unbatched"]["pairing"])
                              for name, _ in WIDTHS}
    return row


def fmt(c):
    return "%.2f / %.2f / %.2f" % (c["min"], c["median"], c["max"])


def table(rows):
    names = [name for name, _ in WIDTHS]
    head = ["call", "items", "mix", "fallback items", "unbatched wall ms"] + ["batched %s wall ms" % w for w in names]
    head += ["batched %s vs unbatched" % w for w in names]
    out = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in rows:
        col = [r["kind"], "%d" % r["items"], r["mix"], "%d" % r["fallback_items"], fmt(r["wall_ms"]["unbatched"])]
        col += [fmt(r["wall_ms"][w]) for w in names]
        col += ["%s (x%.2f)" % (r["verdict"][w], r["wall_ms"]["unbatched"]["median"] / r["wall_ms"][w]["median"]) for w in names]
        out.append("| " + " | ".join(col) + " |")
    out += ["", "Device ms per stage (min / median / max), unbatched and batched under each width", ""]
    head = ["call", "items", "mix", "form", "HASH", "CURVE", "PREPARE + PAIRING", "pairing stage vs unbatched"]
    out += ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in rows:
        for name in ["unbatched"] + names:
            d = r["device_ms"][name]
            out.append("| %s | %d | %s | %s | %s | %s | %s | %s |" % (
                r["kind"], r["items"], r["mix"], name, fmt(d["hash"]), fmt(d["curve"]), fmt(d["pairing"]),
                "" if name == "unbatched" else "%s (x%.2f)" % (
                    r["pairing_verdict"][name], r["device_ms"]["unbatched"]["pairing"]["median"] / d["pairing"]["median"])))
    out += ["", "The batched call's CURVE stage split (all-valid cells, AUTO): the G2 group sum timed alone, and the rest", ""]
    out += ["| call | items | CURVE | G2 sum alone | rest: G1 scaling (medians) |", "|---|---|---|---|---|"]
    for r in rows:
        if r["g2_sum_alone_ms"]:
            c = r["device_ms"]["auto"]["curve"]
            out.append("| %s | %d | %s | %s | %.2f |" % (r["kind"], r["items"], fmt(c), fmt(r["g2_sum_alone_ms"]),
                                                      c["median"] - r["g2_sum_alone_ms"]["median"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternations per cell (>= 5)")
    ap.add_argument("--out", default=None, help="directory for batched_bench.json and batched_bench.md")
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES, help="items per call")
    ap.add_argument("--kinds", nargs="*", default=["sig", "ct"], choices=["sig", "ct"])
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    eng = Engine(0)
    rng = random.Random(25)
    rows = []
    for kind in a.kinds:
        for n in a.sizes:
            for mix, frac in MIXES:
                row = measure(eng, kind, n, mix, frac, a.reps, rng)
                rows.append(row)
                print(json.dumps({k: v for k, v in row.items() if k not in ("wall_ms", "device_ms")}), flush=True)
                if a.out:  # every finished cell is on disk
                    os.makedirs(a.out, exist_ok=True)
                    with open(os.path.join(a.out, "batched_bench.json"), "w") as f:
                        json.dump(rows, f, indent=1)
                        f.write("\n")
                    with open(os.path.join(a.out, "batched_bench.md"), "w") as f:
                        f.write("min / median / max of %d alternated runs per cell\n\n" % a.reps + table(rows))
    eng.close()
    print(table(rows))


if __name__ == "__main__":
    main()
