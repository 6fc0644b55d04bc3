"""Inputs that steer the curve kernels into their exceptional additions, built from known scalars.

Every point of these inputs is a known multiple of one base (g1, or s * B for the combines), so a
group addition of a kernel is an integer addition mod r here, and an exceptional addition is an
integer coincidence that the builder arranges:

  generic   neither of the below
  double    both operands nonzero and equal           (the group law's H = 0, r = 0 branch)
  cancel    both operands nonzero and opposite        (H = 0, r != 0: the sum is O)
  onto_O    exactly one operand is O                  (the early returns; O + O is not logged)

Each builder returns the scalars of its input and an Events log: the integer simulation of the
addition sequence of the kernel it targets, one entry (kind, tag) per addition.  The additions inside a
multiplication by a small or chunk scalar (double-and-add from the top bit: n P + P with 2 <= n < r)
are never exceptional for a point of prime order r and are not simulated.  Pure Python, no GPU.
"""
import random

from oracle import bls12_381 as C

R = C.R
XA = 0xd201000000010000  # |x|, the BLS parameter
X2 = XA * XA
KINDS = ("generic", "double", "cancel", "onto_O")


def inv(a):
    return pow(a % R, R - 2, R)


class Events:
    """Log of the additions of an integer model."""

    def __init__(self):
        self.log = []

    def add(self, a, b, tag=None):
        a %= R
        b %= R
        if a == 0 and b == 0:
            return 0
        if a == 0 or b == 0:
            kind = "onto_O"
        elif a == b:
            kind = "double"
        elif (a + b) % R == 0:
            kind = "cancel"
        else:
            kind = "generic"
        self.log.append((kind, tag))
        return (a + b) % R

    def counts(self, where=None):
        """{kind: count}, optionally over the entries whose tag satisfies where(tag)."""
        c = dict.fromkeys(KINDS, 0)
        for kind, tag in self.log:
            if where is None or where(tag):
                c[kind] += 1
        return c

    def merge(self, other):
        self.log += other.log
        return self


def count_line(name, counts):
    return "%s: %d double, %d cancel, %d onto_O, %d generic" % (
        name, counts["double"], counts["cancel"], counts["onto_O"], counts["generic"])


# ---------------------------------------------------------------- Horner (rows, commitment evaluation)
def cp(i, j):
    """BivarCommitment's coeff_pos of the symmetric matrix."""
    return j * (j + 1) // 2 + i if i <= j else i * (i + 1) // 2 + j


def horner_fill(x0, t, pattern, rng, fixed=None):
    """Coefficients c[0..t] of the walk h <- x0 h + c_j, j = t .. 0.  Step t - j takes pattern[t - j]
    (double: c_j = x0 h, cancel: c_j = -x0 h, onto_O: c_j = 0, generic: random) while the pattern
    lasts, then fixed[j].  A double or cancel asked for while h = 0 becomes a generic step."""
    c = [0] * (t + 1)
    h = 0
    for j in range(t, -1, -1):
        step = t - j
        xh = x0 * h % R
        if step < len(pattern):
            kind = pattern[step]
            assert kind in KINDS
            if kind == "double" and xh:
                c[j] = xh
            elif kind == "cancel" and xh:
                c[j] = R - xh
            elif kind == "onto_O":
                c[j] = 0
            else:
                c[j] = rng.randrange(1, R)
        else:
            c[j] = fixed[j] % R
        h = (xh + c[j]) % R
    return c


def horner_run(x0, c, ev, tag):
    """The kernels' Horner loop: acc = x0 acc (a small multiplication, no logged addition), then
    acc += C_j.  An infinity coefficient (c_j = 0) is logged as onto_O when acc is finite: the lane
    kernels skip it, the quad Ack kernel passes it to g1q_add."""
    h = 0
    t = len(c) - 1
    for j in range(t, -1, -1):
        h = ev.add(x0 * h, c[j], tag + (j,))
    return h


def univar(t, x0, pattern, rng):
    """A Commitment (t + 1 scalars) whose evaluation at x0 walks the pattern: (coefficients, value, events)."""
    c = horner_fill(x0, t, pattern, rng)
    ev = Events()
    return c, horner_run(x0, c, ev, ("eval",)), ev


def poly_eval(c, x):
    v = 0
    for a in reversed(c):
        v = (v * x + a) % R
    return v


def row_coeffs(flat, t, i):
    return [flat[cp(i, j)] for j in range(t + 1)]


def row_values(flat, t, x):
    """rho_i(x) = sum_j c(i, j) x^j, i = 0..t: the scalars of BivarCommitment::row(x)."""
    return [poly_eval(row_coeffs(flat, t, i), x) for i in range(t + 1)]


def f_eval(flat, t, x, y):
    return poly_eval(row_values(flat, t, x), y)


def bivar_rows(t, x0, patterns, rng):
    """A symmetric coefficient matrix (flat, by coeff_pos) whose rows at x0 walk patterns[i] on their
    free entries j = t .. i (rows are filled in order of i; the entries j < i are fixed by symmetry and
    end the walk).  Returns (flat, row values at x0, events of all t + 1 row walks, tag ("row", i, j))."""
    flat = [0] * ((t + 1) * (t + 2) // 2)
    ev = Events()
    rho = []
    for i in range(t + 1):
        fixed = [flat[cp(i, j)] if j < i else 0 for j in range(t + 1)]
        c = horner_fill(x0, t, patterns[i][:t + 1 - i], rng, fixed)
        for j in range(i, t + 1):
            flat[cp(i, j)] = c[j]
        rho.append(horner_run(x0, c, ev, ("row", i)))
    assert rho == row_values(flat, t, x0)
    return flat, rho, ev


# ---------------------------------------------------------------- Ack Horner
def solve_diagonal(t, x0, taus, rng):
    """A symmetric matrix with random off-diagonal entries whose row values at x0 are taus:
    c(i, i) = (tau_i - sum_{j != i} c(i, j) x0^j) x0^-i."""
    flat = [rng.randrange(1, R) for _ in range((t + 1) * (t + 2) // 2)]
    for i in range(t + 1):
        rest = sum(flat[cp(i, j)] * pow(x0, j, R) for j in range(t + 1) if j != i)
        flat[cp(i, i)] = (taus[i] - rest) * inv(pow(x0, i, R)) % R
    assert row_values(flat, t, x0) == [v % R for v in taus]
    return flat


def bivar_ack(t, x0, y0, pattern, rng):
    """A matrix whose row values at x0 make the Ack Horner at y0 walk the pattern:
    (flat, taus, value f(x0, y0), events with tag ("ack", j))."""
    taus = horner_fill(y0, t, pattern, rng)
    flat = solve_diagonal(t, x0, taus, rng)
    ev = Events()
    val = horner_run(y0, taus, ev, ("ack",))
    assert val == f_eval(flat, t, x0, y0)
    return flat, taus, val, ev


# ---------------------------------------------------------------- finite differences
FD_TABLES = ("double", "cancel", "linear", "zero")
FD_SEEDS = ("zero", "first")  # a run from y = 1 (seeded at y0 = 0); a run from y = 50 (seeded there)
FD_FIRST_Y = 50


def fd_table(name, t, rng):
    """Difference table d_k = Delta^k E(y0), k <= t."""
    d = [rng.randrange(1, R) for _ in range(t + 1)]
    if name == "double":      # the first step's D_0 + D_1 doubles
        d[1] = d[0]
    elif name == "cancel":    # d_1 = -d_2; at t = 1 there is no d_2: d_0 = -d_1
        if t >= 2:
            d[2] = R - d[1]
        else:
            d[1] = R - d[0]
    elif name == "linear":    # E linear: every upper entry is O
        for k in range(2, t + 1):
            d[k] = 0
    elif name == "zero":      # E = O everywhere
        d = [0] * (t + 1)
    else:
        raise ValueError(name)
    return d


def newton_to_monomial(d, y0):
    """Coefficients tau_j of E(y) = sum_k d_k binom(y - y0, k)."""
    t = len(d) - 1
    tau = [0] * (t + 1)
    basis = [1]
    for k in range(t + 1):
        for j, b in enumerate(basis):
            tau[j] = (tau[j] + d[k] * b) % R
        # basis *= (y - y0 - k) / (k + 1)
        nxt = [0] * (len(basis) + 1)
        for j, b in enumerate(basis):
            nxt[j + 1] = (nxt[j + 1] + b) % R
            nxt[j] = (nxt[j] - (y0 + k) * b) % R
        ik = inv(k + 1)
        basis = [b * ik % R for b in nxt]
    return tau


def fd_run_model(d, length, ev, tag=("fd_run",)):
    """k_bivar_fd_run: D_k += D_{k+1} for all k < t at once, length - 1 steps; E(y0 + s) = D_0."""
    D = list(d)
    t = len(D) - 1
    out = [D[0]]
    for s in range(1, length):
        D = [ev.add(D[k], D[k + 1], tag + (s, k)) for k in range(t)] + [D[t]]
        out.append(D[0])
    return out


def fd_seed_model(tau, y0, ev, tag=("fd_seed",)):
    """k_bivar_fd_seed, levels m = t .. 0: Delta^k F_m(y0) from level m + 1 by the product rule; the
    row value R_m joins entry k = 0 by a mixed addition."""
    t = len(tau) - 1
    prev = []
    for m in range(t, -1, -1):
        deg = t - m
        cur = []
        for k in range(deg + 1):
            d = 0
            if m < t:
                a = prev[k] if k < deg else 0
                b = prev[k - 1] if k > 0 else 0
                if y0 == 0:
                    d = k * ev.add(a, b, tag + (m, k)) % R
                else:
                    d = ev.add((y0 + k) * a, k * b, tag + (m, k))
            if k == 0:
                d = ev.add(d, tau[m], tag + (m, "row"))
            cur.append(d)
        prev = cur
    return prev


def plan_fd_takes(ys, t):
    """plan_fd's condition (ack_plan.hpp) for the acks of one row: (taken, y0, length)."""
    T1 = t + 1
    ymin, ymax, cnt = min(ys), max(ys), len(ys)
    if ymin <= T1:
        ymin = 0
    span = ymax - ymin + 1
    return cnt >= 2 * T1 and 2 * T1 <= span <= 2 * cnt, ymin, span


def fd_case(t, x0, table, seed, nacks, rng):
    """One Part and the dense run of acks of its row at x0 that plan_fd hands to the FD kernels.
    Returns dict(flat, ys, vals, run (events of the run), seed_ev (events of the seed levels))."""
    first = 1 if seed == "zero" else FD_FIRST_Y
    ys = list(range(first, first + nacks))
    taken, y0, length = plan_fd_takes(ys, t)
    assert taken and y0 == (0 if seed == "zero" else first)
    d = fd_table(table, t, rng)
    tau = newton_to_monomial(d, y0)
    flat = solve_diagonal(t, x0, tau, rng)
    seed_ev, run = Events(), Events()
    assert fd_seed_model(tau, y0, seed_ev) == d
    E = fd_run_model(d, length, run)
    assert E == [poly_eval(tau, y0 + s) for s in range(length)]
    vals = [E[y - y0] for y in ys]
    return dict(flat=flat, ys=ys, vals=vals, run=run, seed_ev=seed_ev, x0=x0)


# ---------------------------------------------------------------- Lagrange combines, m = 2
def lagrange2(idx):
    """lambda_k(0) for the two samples x_k = idx_k + 1."""
    x0, x1 = idx[0] + 1, idx[1] + 1
    return [x1 * inv(x1 - x0) % R, x0 * inv(x0 - x1) % R]


def g2_digits(lam):
    """lam = sum_{j<4} d_j |x|^j, d_j < |x|."""
    d = [lam % XA, lam // XA % XA, lam // XA ** 2 % XA, lam // XA ** 3]
    assert d[3] < XA
    return d


def g1_digits(lam):
    """lam = D_0 + D_1 x^2, D_0 < x^2."""
    d = [lam % X2, lam // X2]
    assert d[1] < 1 << 128
    return d


# form -> (digits, base of digit j, chunks per digit, bits per chunk)
FORMS = {
    "pair": (g2_digits, XA, 2, 32),      # k_interp_pair + k_interp_join (G2, latency)
    "g1q": (g1_digits, X2, 4, 32),       # k_interp_g1q + k_interp_g1_join (G1, latency)
    "endo_g2": (g2_digits, XA, 1, 64),   # k_interp_endo<Fp2> with nchunk = 1 (throughput)
    "endo_g1": (g1_digits, X2, 1, 128),  # k_interp_endo<Fp> with nchunk = 1
}


def term_factor(form, lam, j, s):
    """e with term (k, j, s) = e * s_k: chunk s of digit j of lam, times base^j."""
    digits, base, _, bits = FORMS[form]
    return (digits(lam)[j] >> (bits * s)) % (1 << bits) * pow(base, j, R) % R


def _tree(slots, ev, tag):
    s = len(slots) // 2
    while s:
        for g in range(s):
            slots[g] = ev.add(slots[g], slots[g + s], tag + (s, g))
        s //= 2
    return slots[0]


def combine_model(form, idx, s, ev=None):
    """The addition sequence of one m = 2 combine of points s_k B: (sum as a scalar, events).
      pair:  workgroup (chunk, half) holds term t = half + 2 g (k = t >> 2, j = t & 3) in slot g < 64, an
             LDS tree (levels 32 .. 1) sums the slots, chunk 1 is scaled by 2^32, k_interp_join adds
             (part[2] + part[3]) + (part[0] + part[1]) with part[2 chunk + half].
      g1q:   workgroup chunk holds term t = g (k = t >> 1, j = t & 1) in slot g < 64, tree, scaled by
             2^(32 chunk); the join adds (p0 + p1) + (p2 + p3).
      endo:  one workgroup, term t = g (k = t / N, j = t % N) in slot g < 64, tree; nchunk = 1, no join.
    So the terms (0, j, s) and (1, j, s) meet at tree level 2 (pair, g1q) or N (endo)."""
    ev = ev or Events()
    lam = lagrange2(idx)
    _, _, nchunk, bits = FORMS[form]
    N = 4 if form in ("pair", "endo_g2") else 2

    def term(t, chunk):
        k, j = divmod(t, N)
        return term_factor(form, lam[k], j, chunk) * s[k] % R

    if form == "pair":
        part = []
        for chunk in range(2):
            for half in range(2):
                slots = [0] * 64
                for g in range(64):
                    if half + 2 * g < 8:
                        slots[g] = ev.add(0, term(half + 2 * g, chunk), (form, "term", chunk, half, g))
                part.append(_tree(slots, ev, (form, "tree", chunk, half)) << (32 * chunk))
        s1 = ev.add(part[2], part[3], (form, "join", 1))
        s0 = ev.add(part[0], part[1], (form, "join", 0))
        total = ev.add(s1, s0, (form, "join", 2))
    else:
        part = []
        for chunk in range(nchunk):
            slots = [0] * 64
            for g in range(2 * N):
                slots[g] = ev.add(0, term(g, chunk), (form, "term", chunk, g))
            part.append(_tree(slots, ev, (form, "tree", chunk)) << (bits * chunk))
        if form == "g1q":
            total = ev.add(ev.add(part[0], part[1], (form, "join", 0)), ev.add(part[2], part[3], (form, "join", 1)),
                           (form, "join", 2))
        else:
            total = part[0]
    assert total % R == (lam[0] * s[0] + lam[1] * s[1]) % R
    return total % R, ev


def combine_forced(form, j, s, sign, rng):
    """Indices and sample scalars whose terms (0, j, s) and (1, j, s) are equal (sign = +1: the tree
    doubles) or opposite (sign = -1: it cancels): s_1 = sign e_0 s_0 / e_1.  Indices are drawn until both
    chunks are nonzero.  Returns dict(idx, s, want (the combine as a scalar), ev)."""
    while True:
        idx = rng.sample(range(0, 200), 2)
        lam = lagrange2(idx)
        e0, e1 = term_factor(form, lam[0], j, s), term_factor(form, lam[1], j, s)
        if e0 and e1:
            break
    s0 = rng.randrange(1, R)
    s1 = sign * e0 * s0 * inv(e1) % R
    want, ev = combine_model(form, idx, [s0, s1])
    return dict(idx=idx, s=[s0, s1], want=want, ev=ev)


def combine_free(form, kind, rng):
    """Combines that need no slot map: 'root' (shares of f with f(0) = 0: the last addition cancels, the
    output is O), 'same' (both samples the same point), 'inf0' / 'inf1' (one sample at infinity)."""
    idx = rng.sample(range(0, 200), 2)
    a = rng.randrange(1, R)
    if kind == "root":
        s = [a * (idx[0] + 1) % R, a * (idx[1] + 1) % R]
    elif kind == "same":
        s = [a, a]
    elif kind == "inf0":
        s = [0, a]
    elif kind == "inf1":
        s = [a, 0]
    else:
        raise ValueError(kind)
    want, ev = combine_model(form, idx, s)
    assert kind != "root" or want == 0
    assert kind != "same" or want == a
    return dict(idx=idx, s=s, want=want, ev=ev)


FREE_KINDS = ("root", "same", "inf0", "inf1")


def combine_cases(form, rng):
    """Every forced (digit j, chunk s, sign) combine of a form, then the free ones."""
    _, _, nchunk, _ = FORMS[form]
    N = 4 if form in ("pair", "endo_g2") else 2
    cases = [combine_forced(form, j, s, sign, rng) for j in range(N) for s in range(nchunk) for sign in (1, -1)]
    return cases + [combine_free(form, kind, rng) for kind in FREE_KINDS]


# ---------------------------------------------------------------- the inputs the tests share
# tests/test_degenerate_model.py checks their event logs and the C oracle on them; the GPU tests run the
# kernels on them.  Fixed seeds: the same inputs everywhere.
T = 4
_LETTER = {"G": "generic", "D": "double", "C": "cancel", "O": "onto_O"}
# per Part: the pattern of row i's free entries j = t .. i.  Row 0 of the second Part ends in a cancel:
# rho_0 = 0, the row's first point is O.
ROW_PATTERNS = [("GDCGO", "GCGD", "GDD", "GO", "G"),
                ("GODGC", "GDCG", "GCG", "GD", "G"),
                ("GCOGD", "GGDC", "GOD", "GC", "G")]
ROW_X0 = (1, 2, 3)
ROW_X_GENERIC = 7
# Horner walks j = t .. 0; the second ends in a cancel: the evaluation is O
WALKS = ("GDCGO", "GODGC", "GCOGD")
ACK_Y0 = (1, 2, 5)
EVAL_X0 = (1, 3)
EVAL_X_GENERIC = 9
FD_T = (1, 5)


def kinds(pattern):
    return [_LETTER[ch] for ch in pattern]


def row_inputs():
    rng = random.Random(2001)
    out = []
    for x0, pats in zip(ROW_X0, ROW_PATTERNS):
        flat, rho, ev = bivar_rows(T, x0, [kinds(p) for p in pats], rng)
        out.append(dict(x0=x0, flat=flat, rho=rho, ev=ev))
    return out


def ack_inputs():
    rng = random.Random(2002)
    out = []
    for a, y0 in enumerate(ACK_Y0):
        for b, walk in enumerate(WALKS):
            x0 = 1 + (a + b) % 3
            flat, taus, val, ev = bivar_ack(T, x0, y0, kinds(walk), rng)
            out.append(dict(x0=x0, y0=y0, flat=flat, taus=taus, val=val, ev=ev))
    return out


def eval_inputs():
    rng = random.Random(2003)
    out = []
    for x0 in EVAL_X0:
        for walk in WALKS:
            c, val, ev = univar(T, x0, kinds(walk), rng)
            out.append(dict(x0=x0, c=c, val=val, ev=ev))
    return out


def fd_inputs(t):
    """Every table at both seeds and both run lengths (2 (t + 1) and 2 (t + 1) + 7 acks), x0 = 1, 2, 3 in turn."""
    rng = random.Random(2004 + t)
    out = []
    for seed in FD_SEEDS:
        for table in FD_TABLES:
            for nacks in (2 * (t + 1), 2 * (t + 1) + 7):
                case = fd_case(t, 1 + len(out) % 3, table, seed, nacks, rng)
                case.update(table=table, seed=seed, t=t)
                out.append(case)
    return out


def combine_inputs(form):
    return combine_cases(form, random.Random(2010 + sorted(FORMS).index(form)))
