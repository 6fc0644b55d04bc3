"""hash_g2 on the host stage against its device form, call by call in one process.

  python3 tools/hash_bench.py --out profiles/r14            the sweep + the verify_signed A/B
  python3 tools/hash_bench.py --sizes 1024,16384 --reps 9
  python3 tools/hash_bench.py --form both --out profiles/r24   HOST, DEVICE-LANE and DEVICE-QUAD side by side

For every size, hbh_engine_hash_g2 is forced to HOST and to DEVICE in turn (hbh_engine_set_hash_impl) on
the same seeded 28-byte messages: one warm-up call of each form at that size, then `reps` alternations
timed host-to-host (the synchronous call: SHA3 on the host workers, upload, kernels, download) with
profiling off; the two outputs must be equal bytes.  A second, shorter pass with profiling on records the
HBH_STAGE_HASH device time of the DEVICE form beside it.  The host form uses the host stage's default
worker count (hbh_host_threads).

The AUTO threshold the sweep supports is the smallest swept size from which DEVICE's median is below
HOST's by more than both cells' min-max spread, at that size and at every larger one (none: AUTO stays
HOST).  The same A/B is run for PublicKey::verify at --signed items: hbh_hash_g2 + hbh_verify_sig_shares
against hbh_verify_signatures forced to DEVICE.

--form lane | quad | both picks the device form(s) (hbh_engine_set_hash_form; default lane, the sweep of
profiles/r14): with both, every alternation runs HOST, DEVICE-LANE and DEVICE-QUAD in turn, the three outputs
must be equal bytes, and the Q form (hbh_engine_hash_g1_g2_bp) is measured the same way at --bp-sizes.  The
sweep then supports two thresholds by the same rule of medians and spreads: HBH_AUTO_HASH_QUAD_MAX, the largest
swept size up to which QUAD beats LANE at every swept size from the smallest, and HBH_AUTO_HASH_DEVICE_MIN
over the better device form of each size."""
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


# a column of the sweep: (hbh_engine_set_hash_impl, hbh_engine_set_hash_form)
FORMS = {"host": (_lib.HASH_HOST, _lib.HFORM_AUTO), "device": (_lib.HASH_DEVICE, _lib.HFORM_LANE),
         "quad": (_lib.HASH_DEVICE, _lib.HFORM_QUAD)}
COLUMNS = {"lane": ("host", "device"), "quad": ("host", "quad"), "both": ("host", "device", "quad")}


def sweep_size(eng, n, reps, cols=("host", "device"), bp=False):
    """one size: `cols` in turn, warm-up, outputs compared, `reps` alternations; bp: the Q form
    (hbh_engine_hash_g1_g2_bp with one fixed U) instead of hbh_engine_hash_g2"""
    L = eng._l
    data, offs = messages(n, n)
    dbuf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    po = offs.ctypes.data_as(VP)
    outs = {k: (ctypes.c_uint8 * (n * 192))() for k in cols}
    ub = (ctypes.c_uint8 * (96 * n)).from_buffer_copy(hoststage.g1_mul([G1_GEN], [0x1234567])[0] * n) if bp else None

    def call(form):
        eng.set_hash_impl(FORMS[form][0])
        eng.set_hash_form(FORMS[form][1])
        if bp:
            _lib.check(L.hbh_engine_hash_g1_g2_bp(eng.handle, n, ctypes.cast(ub, VP), ctypes.cast(dbuf, VP), po,
                                                  ctypes.cast(outs[form], VP)))
        else:
            _lib.check(L.hbh_engine_hash_g2(eng.handle, n, ctypes.cast(dbuf, VP), po, ctypes.cast(outs[form], VP)))

    for form in cols:
        call(form)  # warm-up at this size
    for form in cols[1:]:
        assert bytes(outs[cols[0]]) == bytes(outs[form]), "%s and %s hashes differ at n = %d" % (cols[0], form, n)
    t = {form: [] for form in cols}
    for _ in range(reps):
        for form in cols:
            t[form].append(timed(lambda: call(form)))
    row = {"n": n}
    for form in cols:
        row[form] = cell(t[form])
        row[form]["hashes_per_s"] = n / row[form]["median_ms"] * 1e3
        if form == "host":
            continue
        kern = []
        for _ in range(3):
            eng.set_profiling(True)
            call(form)
            kern.append(eng.stage_time(_lib.STAGE_HASH)[0])
            eng.set_profiling(False)
        row[form + "_kernel_ms"] = cell(kern)
    return row


def beats(a, b):
    """cell a wins over cell b: b's median exceeds a's by more than the two min-max spreads together"""
    return b["median_ms"] - a["median_ms"] > (a["max_ms"] - a["min_ms"]) + (b["max_ms"] - b["min_ms"])


def best_device(row):
    return min((f for f in ("device", "quad") if f in row), key=lambda f: row[f]["median_ms"])


def wins(row):
    return beats(row[best_device(row)], row["host"])


def quad_max(rows):
    """largest swept size up to which QUAD beats LANE at every swept size from the smallest; 0: nowhere;
    "all": everywhere"""
    best = 0
    for row in sorted(rows, key=lambda r: r["n"]):
        if not beats(row["quad"], row["device"]):
            return best
        best = row["n"]
    return "all"


def threshold(rows):
    """smallest swept size from which DEVICE (its better form at each size) wins at every larger swept
    size too; None: nowhere"""
    best = None
    for row in sorted(rows, key=lambda r: -r["n"]):
        if not wins(row):
            break
        best = row["n"]
    return best


def signed_ab(eng, n, reps, cols=("host", "device")):
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
    v = {k: (ctypes.c_uint8 * n)() for k in cols}

    def host():
        _lib.check_host(L.hbh_hash_g2(n, ctypes.cast(dbuf, VP), po, ctypes.cast(hb, VP), 0))
        _lib.check(L.hbh_verify_sig_shares(eng.handle, n, ctypes.cast(pkb, VP), ctypes.cast(sgb, VP), ctypes.cast(hb, VP),
                                           n, idx.ctypes.data_as(VP), ctypes.cast(v["host"], VP)))

    def device(form):
        eng.set_hash_form(FORMS[form][1])
        _lib.check(L.hbh_verify_signatures(eng.handle, n, ctypes.cast(pkb, VP), ctypes.cast(sgb, VP), ctypes.cast(dbuf, VP),
                                           po, ctypes.cast(v[form], VP)))

    run = {form: (host if form == "host" else (lambda form=form: device(form))) for form in cols}
    eng.set_hash_impl(_lib.HASH_DEVICE)
    for form in cols:
        run[form]()
        assert bytes(v[form]) == want, "verdicts differ from the construction (%s)" % form
    t = {form: [] for form in cols}
    for _ in range(reps):
        for form in cols:
            t[form].append(timed(run[form]))
    name = {"host": "hash_on_host_then_verify_signatures", "device": "verify_signed_device", "quad": "verify_signed_quad"}
    res = {"n": n}
    for form in cols:
        res[name[form]] = cell(t[form])
    return res


def fmt(c):
    return "%.2f / %.2f / %.2f" % (c["min_ms"], c["median_ms"], c["max_ms"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--signed", type=int, default=10100, help="items of the verify_signed A/B (0: skip)")
    ap.add_argument("--form", choices=sorted(COLUMNS), default="lane", help="device form(s) beside HOST")
    ap.add_argument("--bp-sizes", default="10100,65536", help="sizes of the Q-form rows of --form both (empty: none)")
    ap.add_argument("--out", default=None, help="directory for hash_bench.json and hash_bench.md")
    a = ap.parse_args()
    cols = COLUMNS[a.form]
    dev_cols = cols[1:]
    eng = Engine(0)
    res = {"host_threads": hoststage.host_threads(), "reps": a.reps, "message_bytes": 28, "form": a.form, "rows": []}

    def show(tag, row):
        print("%s n %6d  host %s" % (tag, row["n"], fmt(row["host"])) +
              "".join("  %s %s  kernel %s ms" % (f, fmt(row[f]), fmt(row[f + "_kernel_ms"])) for f in dev_cols) +
              "  " + ("DEVICE" if row["device_wins"] else "-") +
              ("  QUAD" if row.get("quad_beats_lane") else ""), flush=True)

    def one(n, bp):
        row = sweep_size(eng, n, a.reps, cols, bp)
        row["device_wins"] = wins(row)
        if a.form == "both":
            row["quad_beats_lane"] = beats(row["quad"], row["device"])
            row["lane_beats_quad"] = beats(row["device"], row["quad"])
        return row

    try:
        for n in [int(s) for s in a.sizes.split(",")]:
            res["rows"].append(one(n, False))
            show("hash_g2", res["rows"][-1])
        res["auto_threshold"] = threshold(res["rows"])
        print("AUTO threshold supported by this sweep:", res["auto_threshold"], flush=True)
        if a.form == "both":
            res["quad_max"] = quad_max(res["rows"])
            print("HBH_AUTO_HASH_QUAD_MAX supported by this sweep:", res["quad_max"], flush=True)
            res["bp_rows"] = []
            for n in [int(s) for s in a.bp_sizes.split(",") if s]:
                res["bp_rows"].append(one(n, True))
                show("Q form ", res["bp_rows"][-1])
        if a.signed:
            res["verify_signed"] = s = signed_ab(eng, a.signed, a.reps, cols)
            print("verify_signed n %d  " % s["n"] + "  ".join("%s %s" % (k, fmt(c)) for k, c in s.items() if k != "n"),
                  flush=True)
    finally:
        eng.set_hash_impl(_lib.HASH_AUTO)
        eng.set_hash_form(_lib.HFORM_AUTO)
        eng.close()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "hash_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        label = {"device": "DEVICE-LANE" if a.form == "both" else "DEVICE", "quad": "DEVICE-QUAD"}
        with open(os.path.join(a.out, "hash_bench.md"), "w") as f:
            for title, rows in (("hash_g2", res["rows"]), ("Q form (hash_g1_g2_bp)", res.get("bp_rows", []))):
                if not rows:
                    continue
                f.write("%s, ms as min / median / max\n\n| messages | HOST |" % title +
                        "".join(" %s | %s HASH stage |" % (label[c], label[c]) for c in dev_cols) +
                        " HOST hashes/s |" + "".join(" %s hashes/s |" % label[c] for c in dev_cols) + " DEVICE wins |" +
                        (" QUAD beats LANE |" if a.form == "both" else "") + "\n")
                f.write("|---|---|" + "---|---|" * len(dev_cols) + "---|" + "---|" * len(dev_cols) + "---|" +
                        ("---|" if a.form == "both" else "") + "\n")
                for r in rows:
                    f.write("| %d | %s |" % (r["n"], fmt(r["host"])) +
                            "".join(" %s | %s |" % (fmt(r[c]), fmt(r[c + "_kernel_ms"])) for c in dev_cols) +
                            " %.0f |" % r["host"]["hashes_per_s"] +
                            "".join(" %.0f |" % r[c]["hashes_per_s"] for c in dev_cols) +
                            " %s |" % ("yes" if r["device_wins"] else "no") +
                            ((" %s |" % ("yes" if r["quad_beats_lane"] else "no")) if a.form == "both" else "") + "\n")
                f.write("\n")


if __name__ == "__main__":
    main()
