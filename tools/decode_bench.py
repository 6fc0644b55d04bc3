"""Device point decoding on n compressed subgroup points: kernel time from the engine's HIP events
(median and min-max of reps after a warm-up call of the same size) and the host-to-host call;
decoded points must equal the generated ones.

  python3 tools/decode_bench.py [n] [reps]                       one size, the engine's AUTO choice
  python3 tools/decode_bench.py --impl both --sizes 1,64,512,4096,16384,65536 --reps 7 --out sweep.json

--impl lane | split forces k_wire.hip's throughput form or k_wire_split.hip's latency form
(hbh_engine_set_decode_impl); both runs the two forms in turn in this process, cell by cell, and
adds their measured ratio beside the op model's (hbbft_amd/workcount.py) and the AUTO threshold the
sweep supports: the largest size at which SPLIT's median is below LANE's by more than the two
cells' combined min-max spread."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from hbbft_amd import _lib, workcount  # noqa: E402
from hbbft_amd._lib import STAGE_CURVE  # noqa: E402
from hbbft_amd.engine import Engine  # noqa: E402

IMPLS = {"auto": _lib.DEC_AUTO, "lane": _lib.DEC_LANE, "split": _lib.DEC_SPLIT}


def measure(eng, dec, blob, want, reps, label):
    dec(blob)   # warm-up at this size: buffers grown, code resident
    devs, hosts = [], []
    for _ in range(reps):
        eng.set_profiling(True)
        t0 = time.perf_counter()
        got, ok = dec(blob)
        hosts.append((time.perf_counter() - t0) * 1e3)
        devs.append(eng.stage_time(STAGE_CURVE)[0])
        eng.set_profiling(False)
        assert all(ok) and b"".join(got) == want, label + " decode mismatch"
    return {"kernel_ms": statistics.median(devs), "kernel_ms_min": min(devs), "kernel_ms_max": max(devs),
            "host_ms": statistics.median(hosts), "reps": reps}


def git_commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", nargs="?", type=int, default=65536)
    ap.add_argument("reps_pos", nargs="?", type=int, default=None, metavar="reps")
    ap.add_argument("--impl", choices=["auto", "lane", "split", "both"], default="auto")
    ap.add_argument("--sizes", default=None, help="comma-separated batch sizes (default: n)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default=None, help="source revision to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    reps = a.reps_pos if a.reps_pos is not None else a.reps
    sizes = [int(s) for s in a.sizes.split(",")] if a.sizes else [a.n]
    forms = ["lane", "split"] if a.impl == "both" else [a.impl]

    eng = Engine(0)
    rng = random.Random(5)
    from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a
    g1, g2 = g1a(bench.G1_UNC), g2a(bench.G2_UNC)
    m = min(max(sizes), 4096)
    p1 = eng.g1_mul([g1] * m, [rng.randrange(1, bench.R_ORDER) for _ in range(m)])
    p2 = eng.g2_mul([g2] * m, [rng.randrange(1, bench.R_ORDER) for _ in range(m)])
    e1 = [bench.g1_compress_abi(p) for p in p1]
    e2 = [bench.g2_compress_abi(p) for p in p2]
    cells = []
    try:
        for n in sizes:
            for name, encs, pts, dec in (("g1", e1, p1, eng.g1_decompress), ("g2", e2, p2, eng.g2_decompress)):
                blob = b"".join(encs[i % m] for i in range(n))
                want = b"".join(pts[i % m] for i in range(n))
                for form in forms:
                    eng.set_decode_impl(IMPLS[form])
                    cell = {"group": name, "n": n, "impl": form}
                    cell.update(measure(eng, dec, blob, want, reps, "%s %s n=%d" % (name, form, n)))
                    cells.append(cell)
                    print(json.dumps(cell), flush=True)
    finally:
        eng.set_decode_impl(_lib.DEC_AUTO)
        eng.close()

    if a.impl != "both" and len(sizes) == 1:   # the one-line form of earlier rounds
        out = {"n": sizes[0], "impl": a.impl}
        for c in cells:
            out[c["group"] + "_kernel_ms"] = c["kernel_ms"]
            out[c["group"] + "_host_ms"] = c["host_ms"]
            out[c["group"] + "_per_s_device"] = c["n"] / (c["kernel_ms"] / 1e3)
        print(json.dumps(out), flush=True)
        return

    out = {"tool": "tools/decode_bench.py", "impl": a.impl, "sizes": sizes, "reps": reps, "cells": cells,
           "git_commit": a.commit or git_commit()}
    try:
        with open(os.path.join(ROOT, "hbbft_amd", "build_info.json")) as f:
            out["lib_sha256"] = json.load(f)["lib_sha256"]
    except (OSError, ValueError, KeyError):
        out["lib_sha256"] = None
    if a.impl == "both":
        by = {(c["group"], c["n"], c["impl"]): c for c in cells}
        out["comparison"], out["threshold_supported"] = [], {}
        for g in ("g1", "g2"):
            best = 0
            for n in sizes:
                ln, sp = by[(g, n, "lane")], by[(g, n, "split")]
                spread = (ln["kernel_ms_max"] - ln["kernel_ms_min"]) + (sp["kernel_ms_max"] - sp["kernel_ms_min"])
                wins = ln["kernel_ms"] - sp["kernel_ms"] > spread
                if wins:
                    best = max(best, n)
                out["comparison"].append({"group": g, "n": n, "lane_ms": ln["kernel_ms"], "split_ms": sp["kernel_ms"],
                                          "combined_spread_ms": spread, "split_wins": wins,
                                          "measured_ratio": sp["kernel_ms"] / ln["kernel_ms"],
                                          "model_ratio_small_batch": workcount.wire_split_model_ratio(g)})
            out["threshold_supported"][g] = best
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
