"""The engine's host arithmetic and planning (hbbft_amd/csrc/host_fr.hpp, wire_host.hpp, ack_plan.hpp)
compiled for the CPU with the address and undefined-behaviour sanitizers and run as a stand-alone
program (tests/native/engine_host_test.cpp): Lagrange coefficients and their digits against the
Python oracle, the byte-level half of point decoding, and the Ack-check plans."""
import os
import random
import shutil
import subprocess

import pytest

from oracle import tc
from oracle.tc import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XA = 0xd201000000010000  # |x| of BLS12-381
X2 = XA * XA
ERR_DUPLICATE = 5  # HBH_ERR_DUPLICATE_ENTRY
INFINITY, GREATEST, REJECT = 1, 2, 4  # hbl::WIRE_*

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = tmp_path_factory.mktemp("engine_host") / "engine_host_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "hbbft_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "engine_host_test.cpp")])

    def run(lines):
        """One process for all of a test's commands: a list of token lists (ints) per command."""
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
        rows = [[int(tok, 16) for tok in l.split()] for l in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return rows
    return run


def hexes(vals):
    return " ".join("%x" % v for v in vals)


# ---------------------------------------------------------------- Lagrange coefficients and digits
def lagrange_cases():
    rng = random.Random(1)
    top = 2**32 - 1
    cases = [(1, [top]), (2, [1, top]), (4, [1, 5, 9, 2]), (4, [top, top - 1, 7, 2**31]),
             (34, [top] + rng.sample(range(1, top), 33))]
    return [(m, [xs]) for m, xs in cases] + [
        (4, [[3, 3, 7, 8], [1, 5, 9, 2]]),  # a repeated x beside a good combine
        (4, [[1, 5, 9, 2], [6, 2, 4, 6]]),
        (2, [[9, 9], [top, 1]]),
    ]


def check_g2_digits(dg, scalar):
    assert all(d < XA for d in dg[:3]) and dg[3] < 2**64
    assert sum(d * XA**j for j, d in enumerate(dg)) == scalar


def check_g1_digits(w, scalar):
    d0, d1 = w[0] | w[1] << 64, w[2] | w[3] << 64
    assert d0 < X2 and d0 + d1 * X2 == scalar


def test_lagrange_and_digits(run):
    cases = lagrange_cases()
    rows = run(["lagrange %x %x %s" % (len(combs), m, hexes(x for xs in combs for x in xs)) for m, combs in cases])
    for (m, combs), row in zip(cases, rows):
        nc, nl = len(combs), len(combs) * m
        assert len(row) == 3 * nc + nl + 3 * 4 * nl
        st, lam = row[:nc], row[nc:nc + nl]
        pos = nc + nl
        gls = row[pos:pos + 4 * nl]
        st_g2, dg_g2 = row[pos + 4 * nl:][:nc], row[pos + 4 * nl + nc:][:4 * nl]
        st_g1, dg_g1 = row[pos + 8 * nl + nc:][:nc], row[pos + 8 * nl + 2 * nc:][:4 * nl]
        assert st_g2 == st and st_g1 == st
        assert dg_g2 == gls  # host_interp_digits(g1 = false) == host_gls_digits(host_lagrange)
        for c, xs in enumerate(combs):
            if len(set(xs)) < len(xs):
                assert st[c] == ERR_DUPLICATE
                assert lam[c * m:(c + 1) * m] == [0] * m
                assert dg_g2[4 * c * m:4 * (c + 1) * m] == [0] * (4 * m)
                assert dg_g1[4 * c * m:4 * (c + 1) * m] == [0] * (4 * m)
                continue
            assert st[c] == 0
            assert lam[c * m:(c + 1) * m] == tc.lagrange_coeffs_at_zero(xs)
            for k in range(c * m, (c + 1) * m):
                check_g2_digits(gls[4 * k:4 * k + 4], lam[k])
                check_g1_digits(dg_g1[4 * k:4 * k + 4], lam[k])


def test_digits_of_edge_scalars(run):
    scalars = [0, 1, R - 1, XA - 1, XA, X2, X2 - 1, XA**3, 2**255]
    (row,) = run(["digits %x %s" % (len(scalars), hexes(scalars))])
    assert len(row) == 9 * len(scalars)
    for k, v in enumerate(scalars):
        w = row[9 * k:9 * k + 9]
        check_g2_digits(w[:4], v)
        check_g1_digits(w[4:8], v)
        assert w[8] == 0  # the quotient by x^2 fits 128 bits


# ---------------------------------------------------------------- compressed encodings
def expected_words(enc, nfe):
    """little-endian words of each 48-byte big-endian element with the top three bits cleared,
    coefficient 0 (the last element of the encoding) first"""
    words = []
    for c in range(nfe):
        el = enc[48 * (nfe - 1 - c):48 * (nfe - c)]
        v = int.from_bytes(el, "big")
        if nfe - 1 - c == 0:
            v &= (1 << 381) - 1
        words += [(v >> (32 * w)) & 0xffffffff for w in range(12)]
    return words


@pytest.mark.parametrize("nfe", [1, 2])
def test_parse_compressed(run, nfe):
    rng = random.Random(nfe)
    body = bytearray(rng.randrange(256) for _ in range(48 * nfe))
    body[0] &= 0x1f
    inf = bytearray(48 * nfe)

    def with_flags(b, flags, **patch):
        b = bytearray(b)
        b[0] |= flags
        for pos, val in patch.items():
            b[int(pos[1:])] = val
        return bytes(b)
    cases = [(with_flags(body, 0x80), 0), (with_flags(body, 0xa0), GREATEST), (with_flags(inf, 0xc0), INFINITY),
             (with_flags(inf, 0xc1), REJECT),  # infinity with a stray low bit in byte 0
             (with_flags(inf, 0xc0, **{"b%d" % (48 * nfe - 1): 1}), REJECT),  # ... with a stray last byte
             (with_flags(inf, 0xe0), REJECT),  # infinity with the larger-y bit
             (with_flags(body, 0x00), REJECT), (with_flags(body, 0x20), REJECT)]  # compressed bit clear
    rows = run(["parse %x %s" % (nfe, enc.hex()) for enc, _ in cases])
    for (enc, flag), row in zip(cases, rows):
        assert row[0] == flag, enc.hex()
        assert row[1:] == expected_words(enc, nfe), enc.hex()


# ---------------------------------------------------------------- Ack-check plans
def test_order_by_y(run):
    rng = random.Random(3)
    cases = [[], [7], [rng.randrange(1, 40) for _ in range(1000)],
             [rng.choice([1, 5, 2**20, 2**20 + 3, 2**32 - 1]) for _ in range(200)]]  # y >= 2^20: the fallback sort
    rows = run(["order %x %s" % (len(ys), hexes(ys)) for ys in cases])
    for ys, row in zip(cases, rows):
        assert row == sorted(range(len(ys)), key=ys.__getitem__)


def test_dedup_rows(run):
    rng = random.Random(4)
    acks = [(rng.randrange(5), rng.randrange(1, 7)) for _ in range(300)] + [(4, 2**32 - 1), (0, 0), (4, 2**32 - 1)]
    bad = acks[:10] + [(5, 1)] + acks[10:20]
    line = lambda a, nparts: "dedup %x %x %s" % (len(a), nparts, hexes(v for pa in a for v in pa))
    good, refused, empty = run([line(acks, 5), line(bad, 5), line([], 5)])
    assert refused == [0]  # part 5 of 5 parts
    assert empty == [1, 0]
    first = {}
    for pa in acks:
        first.setdefault(pa, len(first))
    rows = list(first)
    n = len(rows)
    assert good[:2] == [1, n]
    assert good[2:2 + n] == [p for p, _ in rows] and good[2 + n:2 + 2 * n] == [x for _, x in rows]
    assert good[2 + 2 * n:] == [first[pa] for pa in acks]


def parse_plan(row, n=None):
    """planfd's row for n acks; plandrain's (n = None): epos with its length, and the order at the end"""
    it = iter(row)
    take = lambda k: [next(it) for _ in range(k)]
    (nfd,) = take(1)
    plan = {"slot": take(nfd), "y0": take(nfd), "off": take(nfd), "len": take(nfd), "npts": take(1)[0],
            "epos": take(take(1)[0] if n is None else n)}
    plan["fd_acks"] = take(take(1)[0])
    plan["other"] = take(take(1)[0])
    if n is None:
        plan["order"] = take(take(1)[0])
    assert not list(it)
    return plan


def fd_cases():
    rng = random.Random(5)
    fixed = [(0, y) for y in range(1, 9)] + [(1, 3), (1, 900)]
    cases = [(1, fixed), (128, [(0, y) for y in range(1, 600)])]  # t + 1 > 128: no FD row
    for t in (0, 1, 2, 5):
        acks = []
        for slot in range(12):
            y0 = rng.choice([1, 2, t + 1, t + 2, 50, 4000])
            ys = [y for y in range(y0, y0 + rng.randrange(1, 40)) if rng.random() < rng.choice([0.3, 0.6, 1.0])]
            acks += [(slot, y) for y in ys] + [(slot, y) for y in ys[:2]]  # some y twice
        rng.shuffle(acks)
        cases.append((t, acks))
    return cases


def plan_lines(cmd, cases):
    return ["%s %x %s %s" % (cmd, len(a), " ".join("%x" % v for v in head), hexes(v for sy in a for v in sy))
            for head, a in cases]


def test_plan_fd(run):
    cases = fd_cases()
    rows = run(plan_lines("planfd", [((t,), a) for t, a in cases]))
    plans = [parse_plan(row, len(a)) for (t, a), row in zip(cases, rows)]

    p = plans[0]  # slot 0: y = 1..8 from y0 = 0 (9 points); slot 1: too sparse
    assert (p["slot"], p["y0"], p["off"], p["len"], p["npts"]) == ([0], [0], [0], [9], 9)
    assert p["fd_acks"] == list(range(8)) and p["other"] == [8, 9]
    assert p["epos"][:8] == list(range(1, 9))
    assert plans[1]["slot"] == [] and plans[1]["other"] == list(range(599))

    for (t, acks), p in zip(cases, plans):
        n = len(acks)
        assert sorted(p["fd_acks"] + p["other"]) == list(range(n))
        assert p["fd_acks"] == sorted(p["fd_acks"]) and p["other"] == sorted(p["other"])
        assert len(set(p["slot"])) == len(p["slot"])
        row_of_slot = {s: f for f, s in enumerate(p["slot"])}
        assert all((acks[a][0] in row_of_slot) == (a in set(p["fd_acks"])) for a in range(n))
        for a in p["fd_acks"]:
            f = row_of_slot[acks[a][0]]
            assert p["y0"][f] <= acks[a][1] < p["y0"][f] + p["len"][f]
            assert p["epos"][a] == p["off"][f] + acks[a][1] - p["y0"][f] < p["npts"]
        assert all(l >= 2 * (t + 1) for l in p["len"])
        assert p["len"] == sorted(p["len"], reverse=True)
        assert p["off"] == [sum(p["len"][:f]) for f in range(len(p["len"]))] and p["npts"] == sum(p["len"])
    assert any(p["slot"] and p["other"] for p in plans[2:])  # the random cases take both paths


def test_plan_drain(run):
    """plan_drain on planfd's cases, on one where every ack is an FD ack and on an empty drain: with use_fd
    and at least one FD row the plan is plan_fd's and `order` the stable y order of the acks it leaves to the
    Horner kernel; without use_fd, or with no FD row, the plan is empty and `order` the stable y order of
    every ack, whatever fd and order held before."""
    cases = fd_cases() + [(1, [(0, y) for y in range(1, 9)] + [(3, y) for y in range(40, 52)]),  # no ack left over
                          (2, [])]
    rows = run(plan_lines("planfd", [((t,), a) for t, a in cases]) +
               plan_lines("plandrain", [((t, 1), a) for t, a in cases]) +
               plan_lines("plandrain", [((t, 0), a) for t, a in cases]))
    k = len(cases)
    for i, (t, acks) in enumerate(cases):
        n = len(acks)
        want, fd, plain = parse_plan(rows[i], n), parse_plan(rows[k + i]), parse_plan(rows[2 * k + i])
        by_y = lambda idx: sorted(idx, key=lambda a: acks[a][1])  # sorted() is stable
        if want["slot"]:
            assert {name: fd[name] for name in want} == want
        else:  # no row qualifies: the plan is as empty as without use_fd
            assert fd == plain
        assert sorted(fd["order"] + fd["fd_acks"]) == list(range(n)) and sorted(fd["order"]) == want["other"]
        assert fd["order"] == by_y(want["other"])
        assert plain["order"] == by_y(range(n))
        assert all(plain[name] == [] for name in ("slot", "y0", "off", "len", "epos", "fd_acks", "other"))
        assert plain["npts"] == 0
    plans = [parse_plan(row) for row in rows[k:2 * k]]
    assert plans[1]["slot"] == [] and plans[1]["order"] == list(range(599))  # no FD row: every ack in order
    assert plans[-2]["slot"] and plans[-2]["order"] == []                    # every ack an FD ack
    assert any(p["slot"] and p["order"] for p in plans)
