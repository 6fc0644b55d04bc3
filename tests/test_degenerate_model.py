"""The degenerate inputs of tests/degenerate_inputs.py, on the CPU: their integer models really reach the
exceptional additions (so the GPU tests that run the kernels on them do not quietly test nothing), and
the scalar identities the GPU tests assert hold in the independent C oracle (oracle/c/bls_cpu.c) on the
same inputs -- P + P, P - P and O operands included."""
import random

import pytest

from oracle import bls12_381 as C
from oracle import cbls
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a

from . import degenerate_inputs as D

R = D.R
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
O1, O2 = bytes(96), bytes(192)
EXCEPTIONAL = ("double", "cancel", "onto_O")


def g1(k):
    return cbls.g1_mul(G1, k % R) if k % R else O1


def reaches_all(counts):
    return all(counts[k] >= 1 for k in EXCEPTIONAL)


def test_event_kinds():
    ev = D.Events()
    assert ev.add(5, 5) == 10 and ev.add(5, R - 5) == 0 and ev.add(0, 7) == 7 and ev.add(7, 0) == 7
    assert ev.add(3, 4) == 7 and ev.add(0, 0) == 0  # O + O is not logged
    assert [k for k, _ in ev.log] == ["double", "cancel", "onto_O", "onto_O", "generic"]


def test_row_walks_reach_every_branch():
    for part in D.row_inputs():
        # beyond the first step of a walk (acc = O there on every input)
        counts = part["ev"].counts(lambda tag: tag[2] < D.T)
        assert reaches_all(counts), (part["x0"], counts)
    # one row value is O: its output bytes are the zero point
    assert sum(1 for part in D.row_inputs() for v in part["rho"] if v == 0) >= 1


def test_ack_walks_reach_every_branch():
    parts = D.ack_inputs()
    for y0 in D.ACK_Y0:
        ev = D.Events()
        for part in parts:
            if part["y0"] == y0:
                ev.merge(part["ev"])
        assert reaches_all(ev.counts(lambda tag: tag[1] < D.T)), y0
        # an infinity row value met by a finite accumulator (the quad kernel's g1q_add(acc, O))
        assert any(part["y0"] == y0 and 0 in part["taus"][:D.T] for part in parts)
        assert any(part["y0"] == y0 and part["val"] == 0 for part in parts)  # an O evaluation


def test_eval_walks_reach_every_branch():
    for x0 in D.EVAL_X0:
        ev = D.Events()
        for case in D.eval_inputs():
            if case["x0"] == x0:
                ev.merge(case["ev"])
        assert reaches_all(ev.counts(lambda tag: tag[1] < D.T)), x0


@pytest.mark.parametrize("t", D.FD_T)
def test_fd_runs_reach_every_branch(t):
    cases = D.fd_inputs(t)
    assert len(cases) == 16
    for seed in D.FD_SEEDS:
        ev = D.Events()
        for case in cases:
            if case["seed"] == seed:
                assert D.plan_fd_takes(case["ys"], t)[0]
                ev.merge(case["run"])
        assert reaches_all(ev.counts()), (t, seed)
    # E = O: val = 0 is the valid value everywhere
    assert all(v == 0 for case in cases if case["table"] == "zero" for v in case["vals"])
    first = {(c["table"], c["seed"]): c["run"].log for c in reversed(cases)}
    for seed in D.FD_SEEDS:
        assert first[("double", seed)][0] == ("double", ("fd_run", 1, 0))  # the first step's D_0 + D_1
        k = 1 if t >= 2 else 0
        assert ("cancel", ("fd_run", 1, k)) in first[("cancel", seed)]


@pytest.mark.parametrize("form", sorted(D.FORMS))
def test_combines_reach_every_branch(form):
    digits, base, nchunk, bits = D.FORMS[form]
    N = 4 if base == D.XA else 2
    level = 2 if form in ("pair", "g1q") else N
    cases = D.combine_inputs(form)
    forced = cases[:-len(D.FREE_KINDS)]
    assert len(forced) == N * nchunk * 2
    k = 0
    for j in range(N):
        for s in range(nchunk):
            for want in ("double", "cancel"):
                # the two terms (0, j, s) and (1, j, s) meet at tree level `level`
                # (Lagrange coefficients of small indices are (a + c r) / b with small a, b, c, so the
                # ratio of two digits can repeat at another j: then that pair coincides as well)
                hits = [tag for kind, tag in forced[k]["ev"].log if kind == want]
                where = (s, j & 1, level, j >> 1) if form == "pair" else (s, level, j)
                assert (form, "tree") + where in hits, (form, j, s, want, hits)
                k += 1
    free = dict(zip(D.FREE_KINDS, cases[-len(D.FREE_KINDS):]))
    assert free["root"]["want"] == 0 and free["root"]["ev"].log[-1][0] == "cancel"
    ev = D.Events()
    for case in cases:
        ev.merge(case["ev"])
    assert reaches_all(ev.counts(lambda tag: tag[1] != "term"))  # onto_O beyond acc = O + term


def test_digits_are_the_pinned_expansions():
    rng = random.Random(5)
    for lam in [0, 1, R - 1, D.XA, D.X2, D.X2 - 1] + [rng.randrange(R) for _ in range(20)]:
        d = D.g2_digits(lam)
        assert all(v < D.XA for v in d) and sum(v * D.XA ** j for j, v in enumerate(d)) == lam
        d = D.g1_digits(lam)
        assert d[0] < D.X2 and d[1] < 1 << 128 and d[0] + d[1] * D.X2 == lam


# ---------------------------------------------------------------- the C oracle on the same inputs
def test_oracle_rows():
    for part in D.row_inputs():
        commit = [g1(c) for c in part["flat"]]
        assert cbls.bivar_row(D.T, commit, part["x0"]) == [g1(v) for v in part["rho"]]
        assert cbls.bivar_row(D.T, commit, D.ROW_X_GENERIC) == [g1(v) for v in
                                                                 D.row_values(part["flat"], D.T, D.ROW_X_GENERIC)]


def test_oracle_ack_evaluations():
    for part in D.ack_inputs():
        commit = [g1(c) for c in part["flat"]]
        assert cbls.bivar_row(D.T, commit, part["x0"]) == [g1(v) for v in part["taus"]]
        assert cbls.bivar_evaluate(D.T, commit, part["x0"], part["y0"]) == g1(part["val"])  # O == O included
        assert cbls.bivar_evaluate(D.T, commit, part["x0"], 6) == g1(D.f_eval(part["flat"], D.T, part["x0"], 6))


def test_oracle_fd_evaluations():
    for case in D.fd_inputs(1) + D.fd_inputs(5)[::3]:
        commit = [g1(c) for c in case["flat"]]
        for k in (0, 1, len(case["ys"]) - 1):
            assert cbls.bivar_evaluate(case["t"], commit, case["x0"], case["ys"][k]) == g1(case["vals"][k])


@pytest.mark.parametrize("form", sorted(D.FORMS))
def test_oracle_combines(form):
    g2 = form in ("pair", "endo_g2")
    b = 0x1234567 + len(form)
    base = cbls.g2_mul(G2, b) if g2 else cbls.g1_mul(G1, b)
    mul, comb, zero = (cbls.g2_mul, cbls.combine_g2, O2) if g2 else (cbls.g1_mul, cbls.combine_g1, O1)
    for case in D.combine_inputs(form):
        pts = [mul(base, s) if s else zero for s in case["s"]]
        rc, got = comb(1, case["idx"], pts)
        assert rc == 0
        assert got == (mul(base, case["want"]) if case["want"] else zero)


def test_oracle_group_law_edges():
    a = 0xabcdef
    p = g1(a)
    assert cbls.g1_add(p, p) == g1(2 * a)
    assert cbls.g1_add(p, g1(R - a)) == O1
    assert cbls.g1_add(p, O1) == p and cbls.g1_add(O1, p) == p and cbls.g1_add(O1, O1) == O1
