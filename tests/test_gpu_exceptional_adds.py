"""The exceptional additions of every group law -- P + P, P + (-P), an operand at infinity -- reached
through the public engine calls with the inputs of tests/degenerate_inputs.py, whose points are known
multiples of one base: every expectation is an exact scalar identity computed by the C oracle
(cbls.g1_mul / g2_mul of the base), compared byte for byte or verdict for verdict.
tests/test_degenerate_model.py asserts, on the CPU, that the integer model of each kernel's addition
sequence meets a doubling, a cancellation and an O operand on these inputs.

Paths (group law in brackets):
  rows        k_bivar_row [jac_add_affine] through Engine.bivar_row and CommitSet.rows; k_bivar_row_quad
              [g1q_add_affine] keeps its rows on the device, so it is reached through the Ack verdicts on
              the same Parts (Engine.bivar_ack_check, and CommitSet.ack_check under ACK_QUAD)
  acks        k_bivar_check [jac_add_affine] and k_bivar_check_quad [g1q_add on Jacobian rows: equal
              points with different Z; g1_madd_lane on the g1 * val side]
  FD          k_bivar_fd_seed / k_bivar_fd_run [jac_add]
  evaluation  k_commit_eval [jac_add_affine]
  combines    k_interp_pair / k_interp_join [qj_add, hj/qj_add_affine], k_interp_g1q / k_interp_g1_join
              [g1q_add], k_interp_endo<Fp2> and <Fp> [jac_add, the Fp2 instantiation included]

Slot-to-term maps of the combines for m = 2 (term (k, j, s): chunk s of digit j of lambda_k, times
base_j(P_k)), as the kernels have them:
  k_interp_pair   workgroup (chunk s, half) holds term t = half + 2 g in slot g, k = t >> 2, j = t & 3: the
                  terms (0, j, s) and (1, j, s) sit in slots j >> 1 and (j >> 1) + 2 of half j & 1 and meet at
                  tree level 2
  k_interp_g1q    workgroup (chunk s) holds term t = g, k = t >> 1, j = t & 1: slots j and j + 2, level 2
  k_interp_endo   one workgroup, term t = g, k = t / N, j = t % N (N = 4 on G2, 2 on G1): slots j and j + N,
                  level N; at 128 combines and more nchunk = 1: the chunk is the whole digit
One combine per (j, s, sign) makes exactly that addition a doubling or a cancellation.

Not constructible with points of order r, so not forced here: a doubling or cancellation in g1_madd_lane
and in the quad's join of its four comb sums (k_bivar_check_quad's g1 * val: lane q adds comb windows
q, q + 4, ... of val, integers with disjoint byte positions whose partial sums stay below the next entry and
whose differences are never a multiple of r; val = 0 and val = 1 still give it O operands), and in the
mixed additions inside a multiplication by a chunk or a small scalar (n P + P with 2 <= n < 2^128).

Events of the integer model on these inputs (double / cancel / onto_O): rows 10 / 8 / 28, acks 9 / 9 / 21,
evaluation 6 / 6 / 14; FD run, seed at 0: t = 1 4 / 2 / 2, t = 5 2 / 2 / 35; seed at the first y: t = 1 4 / 2 / 2,
t = 5 2 / 2 / 33; the seed levels' own additions (not forced; no doubling or cancellation occurs in them), seed
at 0: t = 1 0 / 0 / 24, t = 5 0 / 0 / 72, seed at the first y: t = 1 0 / 0 / 18, t = 5 0 / 0 / 50; combines (trees and
joins, without acc = O + term) pair 9 / 9 / 1222, g1q 11 / 14 / 1199, endo_g2 4 / 6 / 272, endo_g1 2 / 3 / 115
(the Lagrange coefficients of small indices are (a + c r) / b with small a, b, c, so a forced pair of digits
sometimes brings a second coinciding pair with it; test_degenerate_model.py asserts the conditions, these
counts are informative)."""
import random

import pytest

from oracle import bls12_381 as C
from oracle import cbls
from hbbft_amd._lib import ACK_AUTO, ACK_LANE, ACK_LANE_HORNER, ACK_QUAD
from hbbft_amd.engine import g1_abi_from_uncompressed as g1a, g2_abi_from_uncompressed as g2a

from . import degenerate_inputs as D

pytestmark = pytest.mark.gpu
R = D.R
T = D.T
G1 = g1a(C.g1_uncompressed(C.G1_GEN))
G2 = g2a(C.g2_uncompressed(C.G2_GEN))
O1, O2 = bytes(96), bytes(192)
INTERP_PAIR_MAX, INTERP_G1Q_MAX = 384, 256  # engine_curve.hip: the latency forms run up to these many combines


def g1(k):
    """g1 * k by the C oracle; the zero bytes for k = 0."""
    return cbls.g1_mul(G1, k % R) if k % R else O1


def commit_points(engine, scalars):
    """g1 * c per coefficient from the engine's comb, the zero point where c = 0."""
    pts = engine.g1_mul_gen([c % R for c in scalars])
    return [O1 if c % R == 0 else p for c, p in zip(scalars, pts)]


def tamper(vals):
    """Every 5th val off by one: (vals, verdicts)."""
    out = [(v + 1) % R if a % 5 == 0 else v for a, v in enumerate(vals)]
    return out, bytes(0 if a % 5 == 0 else 1 for a in range(len(vals)))


def check_acks(engine, t, commits, acks, vals, want, impls=(ACK_QUAD, ACK_LANE, ACK_LANE_HORNER, ACK_AUTO)):
    args = ([a[0] for a in acks], [a[1] for a in acks], [a[2] for a in acks], vals)
    assert engine.bivar_ack_check(t, commits, *args) == want
    cs = engine.commit_set(t)
    cs.add(commits)
    try:
        for impl in impls:
            engine.set_ack_impl(impl)
            assert cs.ack_check(*args) == want, impl
    finally:
        engine.set_ack_impl(ACK_AUTO)
        cs.close()


# ---------------------------------------------------------------- rows
@pytest.fixture(scope="module")
def row_case(engine):
    parts = D.row_inputs()
    return parts, [commit_points(engine, part["flat"]) for part in parts]


def test_comb_agrees_with_oracle_on_the_coefficients(engine, row_case):
    parts, commits = row_case
    assert engine.g1_mul_gen([0, 1, R - 1]) == [O1, G1, g1(R - 1)]
    assert commits[1] == [g1(c) for c in parts[1]["flat"]]
    assert O1 in commits[0]  # an infinity coefficient


def test_rows_at_degenerate_x(engine, row_case):
    """Each Part's rows at its x0 (1: Z stays 1; 2, 3: the mixed addition meets a non-trivial Z) and at a
    generic x: byte-equal to g1 * rho_i, the zero bytes where rho_i = 0."""
    parts, commits = row_case
    rp, rx, want = [], [], []
    for p, part in enumerate(parts):
        for x in (part["x0"], D.ROW_X_GENERIC):
            rp.append(p)
            rx.append(x)
            want.append([g1(v) for v in D.row_values(part["flat"], T, x)])
    assert any(O1 in row for row in want)
    assert want == [commit_points(engine, D.row_values(parts[p]["flat"], T, x)) for p, x in zip(rp, rx)]
    assert engine.bivar_row(T, commits, rp, rx) == want
    cs = engine.commit_set(T)
    cs.add(commits)
    try:
        for impl in (ACK_QUAD, ACK_AUTO):
            engine.set_ack_impl(impl)
            assert cs.rows(rp, rx) == want, impl
    finally:
        engine.set_ack_impl(ACK_AUTO)
        cs.close()


def test_acks_on_degenerate_rows(engine, row_case):
    """The same Parts through the Ack checks: the quad forms compute their Jacobian rows at x0 with
    k_bivar_row_quad, so a wrong row shows as a wrong verdict."""
    parts, commits = row_case
    acks = [(p, x, y) for p, part in enumerate(parts) for x in (part["x0"], D.ROW_X_GENERIC) for y in (1, 2, 3, 6)]
    vals, want = tamper([D.f_eval(parts[p]["flat"], T, x, y) for p, x, y in acks])
    check_acks(engine, T, commits, acks, vals, want)


# ---------------------------------------------------------------- acks
def test_acks_at_degenerate_y(engine):
    """Parts whose row values at x0 make the Ack Horner at y0 double, cancel and meet O.  Per Part two blocks
    of five acks, so that with every 5th val off by one the forced ack (x0, y0) is checked once with its
    true val and once with val + 1; on an O evaluation these are val = 0 (valid) and val = 1 (invalid).  A
    row has at most 9 acks: below plan_fd's 2 (t + 1), so ACK_LANE takes the Horner kernel here."""
    parts = D.ack_inputs()
    commits = [commit_points(engine, part["flat"]) for part in parts]
    acks = []
    for p, part in enumerate(parts):
        x0, y0 = part["x0"], part["y0"]
        other = [y for y in range(1, 9) if y != y0]
        acks += [(p, x0, other[0]), (p, x0, y0), (p, x0, other[1]), (p, x0, other[2]), (p, x0, other[3])]
        acks += [(p, x0, y0), (p, x0 + 3, y0), (p, x0, other[4]), (p, x0, other[5]), (p, x0 + 3, other[0])]
    vals, want = tamper([D.f_eval(parts[p]["flat"], T, x, y) for p, x, y in acks])
    seen = set()
    for a, (p, x, y) in enumerate(acks):
        if (x, y) == (parts[p]["x0"], parts[p]["y0"]):
            assert vals[a] == (parts[p]["val"] + (a % 5 == 0)) % R
            seen.add((parts[p]["val"] == 0, vals[a], want[a]))
    assert {(True, 0, 1), (True, 1, 0)} <= seen
    check_acks(engine, T, commits, acks, vals, want)


# ---------------------------------------------------------------- finite differences
@pytest.mark.parametrize("t", D.FD_T)
def test_fd_runs_on_degenerate_tables(engine, t):
    """Difference tables with d_0 = d_1, d_1 = -d_2 (t = 1: d_0 = -d_1), d_k = 0 for k > 1 and all zero, at
    both of plan_fd's seeds (a run from y = 1, seeded at 0; a run from y = 50), runs of 2 (t + 1) and
    2 (t + 1) + 7 acks: ACK_LANE's finite differences, the Horner kernel and the lane quads give the
    construction's verdicts (an error in a step spoils every later y of its run)."""
    cases = D.fd_inputs(t)
    commits = [commit_points(engine, case["flat"]) for case in cases]
    acks = [(p, case["x0"], y) for p, case in enumerate(cases) for y in case["ys"]]
    vals, want = tamper([v for case in cases for v in case["vals"]])
    check_acks(engine, t, commits, acks, vals, want, impls=(ACK_LANE, ACK_LANE_HORNER, ACK_QUAD))


# ---------------------------------------------------------------- Commitment::evaluate
def test_commitment_eval_at_degenerate_x(engine):
    cases = D.eval_inputs()
    commits = [commit_points(engine, case["c"]) for case in cases]
    idx, xs, want = [], [], []
    for k, case in enumerate(cases):
        for x in (case["x0"], D.EVAL_X_GENERIC):
            idx.append(k)
            xs.append(x)
            want.append(g1(D.poly_eval(case["c"], x)))
        assert D.poly_eval(case["c"], case["x0"]) == case["val"]
    assert O1 in want
    assert engine.commitment_eval(T, commits, idx, xs) == want


# ---------------------------------------------------------------- combines
def combine_args(form, cases):
    """(base, idx, points, expected outputs) of m = 2 combines of points s_k B."""
    g2 = form in ("pair", "endo_g2")
    mul, gen, zero = (cbls.g2_mul, G2, O2) if g2 else (cbls.g1_mul, G1, O1)
    base = mul(gen, 0x5eed0 + len(form))
    pts = [[mul(base, s) if s else zero for s in case["s"]] for case in cases]
    want = [mul(base, case["want"]) if case["want"] else zero for case in cases]
    return [case["idx"] for case in cases], pts, want


@pytest.mark.parametrize("form", ["pair", "g1q"])
def test_combines_latency_forms(engine, form):
    """One combine per (digit j, 32-bit chunk s, sign): 4 x 2 x 2 on G2, 2 x 4 x 2 on G1, then f(0) = 0 (the
    output is O), both samples the same point, and either sample at infinity; one call per group."""
    cases = D.combine_inputs(form)
    assert len(cases) == 20 <= min(INTERP_PAIR_MAX, INTERP_G1Q_MAX)
    idx, pts, want = combine_args(form, cases)
    got, status = (engine.interpolate_g2 if form == "pair" else engine.interpolate_g1)(1, idx, pts)
    assert status == [0] * len(cases)
    assert got == want
    assert (O2 if form == "pair" else O1) in want


@pytest.mark.parametrize("form", ["endo_g2", "endo_g1"])
def test_combines_throughput_form(engine, form):
    """The forced combines on whole digits (nchunk = 1) and the free ones, padded with copies of one generic
    combine to one call more than the latency form takes, so that k_interp_endo runs."""
    g2 = form == "endo_g2"
    cases = D.combine_inputs(form)
    assert len(cases) == (8 if g2 else 4) + len(D.FREE_KINDS)
    rng = random.Random(77)
    s = [rng.randrange(1, R), rng.randrange(1, R)]
    generic = dict(idx=[3, 11], s=s, want=D.combine_model(form, [3, 11], s)[0])
    idx, pts, want = combine_args(form, cases + [generic])
    total = (INTERP_PAIR_MAX if g2 else INTERP_G1Q_MAX) + 1
    pad = total - len(idx)
    got, status = (engine.interpolate_g2 if g2 else engine.interpolate_g1)(
        1, idx + [idx[-1]] * pad, pts + [pts[-1]] * pad)
    assert status == [0] * total
    assert got == want + [want[-1]] * pad
