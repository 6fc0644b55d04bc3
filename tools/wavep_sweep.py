"""Kernel time of a sign-share check call by size for the pairing kinds that compete for mid-size
calls -- WAVE (one wave per check), WAVEP (the same, packed: k_wavep.hip) and OCT -- forced in turn
in ONE process, cell by cell: after a warm-up call of the size, `reps` calls, kernel time from the
engine's HIP events (stage_time(HBH_STAGE_PAIRING)), median and min-max per cell.  Verdicts are
compared with the lane-pair kernel's at every size.

  python3 tools/wavep_sweep.py --out profiles/r08/wavep_sweep.json
  python3 tools/wavep_sweep.py --sizes 4096,4160 --reps 7 --forms wave,wavep

The AUTO range the sweep supports is the contiguous run of swept sizes at which WAVEP's median is
below the best of the other forms' medians by more than both cells' min-max spread (the rule the
decoder thresholds followed, tools/decode_bench.py).  HBBFT_HIP_LIB selects the build (A/B libraries
of the same sources); its sha256 is recorded."""
import argparse
import hashlib
import json
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import bls12_381 as C  # noqa: E402
from oracle import cbls  # noqa: E402
from hbbft_amd import _lib  # noqa: E402
from hbbft_amd._lib import STAGE_PAIRING  # noqa: E402
from hbbft_amd.engine import Engine, g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a  # noqa: E402

FORMS = {"wave": _lib.IMPL_WAVE, "wavep": _lib.IMPL_WAVEP, "oct": _lib.IMPL_OCT, "wave2": _lib.IMPL_WAVE2,
         "quad": _lib.IMPL_QUAD, "auto": _lib.IMPL_AUTO}
SIZES = [512, 768, 1024, 1536, 2048, 3072, 4096, 4160, 5120, 6144, 8192]


def git_commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


def base_items():
    """64 sign shares over 3 documents: valid, another document's share, pk = sig = O"""
    rng = random.Random(5)
    g1, g2 = g1a(C.g1_uncompressed(C.G1_GEN)), g2a(C.g2_uncompressed(C.G2_GEN))
    hs = [cbls.g2_mul(g2, rng.randrange(1, C.R)) for _ in range(3)]
    sk = [rng.randrange(1, C.R) for _ in range(7)]
    pks = [cbls.g1_mul(g1, k) for k in sk]
    base = []
    for i in range(64):
        d, j = i % 3, i % 7
        pk, sig = pks[j], cbls.g2_mul(hs[d], sk[j])
        if i % 11 == 3:
            sig = cbls.g2_mul(hs[(d + 1) % 3], sk[j])
        elif i % 11 == 7:
            pk, sig = bytes(96), bytes(192)
        base.append((pk, sig, d))
    return hs, base


def measure(eng, args, reps):
    eng.verify_sig_shares(*args)  # warm-up at this size
    ms = []
    for _ in range(reps):
        eng.set_profiling(True)
        eng.verify_sig_shares(*args)
        ms.append(eng.stage_time(STAGE_PAIRING)[0])
        eng.set_profiling(False)
    return {"kernel_ms": statistics.median(ms), "kernel_ms_min": min(ms), "kernel_ms_max": max(ms), "reps": reps}


def supported_range(sizes, by, forms):
    """(min, max) of the longest contiguous run of sizes where WAVEP wins by the spread rule, or None"""
    rows, best, run = [], None, []
    for n in sizes:
        wp = by[(n, "wavep")]
        others = [by[(n, f)] for f in forms if f not in ("wavep", "auto")]  # auto may be WAVEP itself
        ot = min(others, key=lambda c: c["kernel_ms"])
        spread = (wp["kernel_ms_max"] - wp["kernel_ms_min"]) + (ot["kernel_ms_max"] - ot["kernel_ms_min"])
        wins = ot["kernel_ms"] - wp["kernel_ms"] > spread
        rows.append({"n": n, "wavep_ms": wp["kernel_ms"], "best_other": ot["impl"], "best_other_ms": ot["kernel_ms"],
                     "combined_spread_ms": spread, "ratio": wp["kernel_ms"] / ot["kernel_ms"], "wavep_wins": wins})
        run = run + [n] if wins else []
        if run and (best is None or len(run) > len(best)):
            best = list(run)
    return rows, ([best[0], best[-1]] if best else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--forms", default="wave,wavep,oct")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--commit", default=None, help="source revision to record (default: git rev-parse HEAD)")
    ap.add_argument("--note", default=None, help="free text recorded with the results (the variant built)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    forms = a.forms.split(",")

    hs, base = base_items()
    eng = Engine(0)
    cells = []
    try:
        for n in sizes:
            bb = (base * ((n + 63) // 64))[:n]
            args = ([b[0] for b in bb], [b[1] for b in bb], hs, [b[2] for b in bb])
            eng.set_pairing_impl(_lib.IMPL_PAIR)
            ref = eng.verify_sig_shares(*args)
            assert sum(ref) == sum(1 for i in range(n) if i % 64 % 11 != 3), n
            for form in forms:  # the forms alternate at every size
                eng.set_pairing_impl(FORMS[form])
                assert eng.verify_sig_shares(*args) == ref, (form, n)
                cell = {"n": n, "impl": form}
                cell.update(measure(eng, args, a.reps))
                cells.append(cell)
                print(json.dumps(cell), flush=True)
    finally:
        eng.set_pairing_impl(_lib.IMPL_AUTO)
        eng.close()

    out = {"tool": "tools/wavep_sweep.py", "workload": "verify_sig_shares, 3 documents", "sizes": sizes, "forms": forms,
           "reps": a.reps, "cells": cells, "git_commit": a.commit or git_commit(), "lib": os.path.relpath(_lib.LIB_PATH, ROOT),
           "lib_sha256": sha256(_lib.LIB_PATH), "verdicts_checked_against": "pair"}
    if a.note:
        out["note"] = a.note
    if "wavep" in forms and any(f not in ("wavep", "auto") for f in forms):
        by = {(c["n"], c["impl"]): c for c in cells}
        out["comparison"], out["auto_range_supported"] = supported_range(sizes, by, forms)
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
