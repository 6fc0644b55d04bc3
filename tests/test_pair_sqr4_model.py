"""The lane-pair Fp4 squaring leaf of the cyclotomic squarings (csrc/pfp.hpp h_sqr4_l, HP_SQR4 = 1),
restated twice.  The form tested is the one shipped: column-interleaved, with the products of a^2
and (a + b)^2 accumulated straight into the two Montgomery chains (of A and of C = A + B), b^2's
chain alone carry-extracted and sent across the lane pair, and B = C - A; no 28-limb value stored.

Values, over the oracle's Fp2 arithmetic: from three squares the leaf's formulas give
(a^2 + xi b^2, 2 a b); hc_sqr (Karabina's compressed squaring) and h12_cyclo_sqr (Granger-Scott's)
rebuilt on the leaf equal the oracle's Fp12 square on random cyclotomic elements and on 1, which
compresses to four zeros.

Bounds, over Python integers in the kernel's limb form (14 signed limbs of 28 bits, Montgomery
R = 2^392, an Fp2 value as the even and the odd lane's component): every statement of h_sqr4_l in the
order pfp.hpp has them, with a check on every int32 value, on every int64 column sum and carry of
the five chains (three of products, two of digits, in three accumulators), on every digit and on both
outputs: A normalised, in (-p/20, p + p/20), inside h_sqr's (-p/8, 9p/8); B lazy, |limb| < 2^28, |B| <
1.1p.  The unreduced sums are checked to be the integers the formulas name.  The operands stand at
the contract's ends: every sign pattern of the four components at +-2p, the low limbs all ones or
all zeros on either lane.  The pair of a + b is NOT normalised in the kernel: its limbs reach 2^30
and 2^29, its products share C's accumulator with the digits' terms, and the test shows those columns
stay below 2^63 (14 x 2^59 + 14 x 2^56 + carries < 2^62.98).  The callers' fp_red_mk passes
(3 A - 2 a_k, 3 B + 2 a_k, and the one with xi on B) are then run at the ends of the leaf's output
contract, on outputs chosen by hand.
"""
import itertools
import random

from oracle import bls12_381 as C
from tests.test_pair_exp_high_model import cyclotomic
from tests.test_pair_toom_model import (MASK, NL, NP0, P_L, RBITS, RINV, extreme, f2_of, fp_red_mk, h_xi_l, i32, i64, is_norm,
                                        limbs, val)

P = C.P
add, sub, sqr, xi, mul = C.f2_add, C.f2_sub, C.f2_sqr, C.f2_mul_xi, C.f2_mul


def k2(a, n):
    return C.f2_muls(a, n % P)


# ---------------------------------------------------------------- values
def sqr4(a, b):
    """the leaf's formulas: three squares, xi on b^2, the cross term from the square of the sum"""
    sa, sb, ss = sqr(a), sqr(b), sqr(add(a, b))
    return add(sa, xi(sb)), sub(sub(ss, sa), sb)


def hc_sqr(c):
    """pfp.hpp hc_sqr on the leaf: (a1, a2, a4, a5)"""
    a1, a2, a4, a5 = c
    A, B = sqr4(a1, a4)
    r2, r5 = sub(k2(A, 3), k2(a2, 2)), add(k2(B, 3), k2(a5, 2))
    A, B = sqr4(a2, a5)
    r4, r1 = sub(k2(A, 3), k2(a4, 2)), add(k2(xi(B), 3), k2(a1, 2))
    return (r1, r2, r4, r5)


def h12_cyclo_sqr(f):
    """pfp.hpp h12_cyclo_sqr on the leaf"""
    (a0, a2, a4), (a1, a3, a5) = f
    A, B = sqr4(a0, a3)
    c00, c11 = sub(k2(A, 3), k2(a0, 2)), add(k2(B, 3), k2(a3, 2))
    A, B = sqr4(a1, a4)
    c01, c12 = sub(k2(A, 3), k2(a2, 2)), add(k2(B, 3), k2(a5, 2))
    A, B = sqr4(a2, a5)
    c02, c10 = sub(k2(A, 3), k2(a4, 2)), add(k2(xi(B), 3), k2(a1, 2))
    return ((c00, c01, c02), (c10, c11, c12))


def compress(f):
    return (f[1][0], f[0][1], f[0][2], f[1][2])


def test_leaf_formulas():
    rng = random.Random(0x73717234)
    pick = lambda: rng.choice((0, 1, P - 1, rng.randrange(P)))
    for _ in range(300):
        a, b = (pick(), pick()), (pick(), pick())
        A, B = sqr4(a, b)
        assert A == add(mul(a, a), xi(mul(b, b)))
        assert B == k2(mul(a, b), 2)


def test_squarings_on_the_leaf_are_the_fp12_square():
    rng = random.Random(0x6379636c)
    for f in [C.F12_ONE] + [cyclotomic(rng) for _ in range(8)]:
        want = C.f12_sqr(f)
        assert h12_cyclo_sqr(f) == want
        assert hc_sqr(compress(f)) == compress(want)
    zero = (0, 0)
    assert compress(C.F12_ONE) == (zero,) * 4 and hc_sqr((zero,) * 4) == (zero,) * 4
    # a chain of compressed squarings stays the compression of the chain of squares
    f = cyclotomic(rng)
    c = compress(f)
    for _ in range(5):
        f, c = C.f12_sqr(f), hc_sqr(c)
        assert c == compress(f)


# ---------------------------------------------------------------- limbs
class Stats:
    def __init__(self):
        self.col = self.red = 0  # the largest |column| of b^2's chain; of the two Montgomery chains


def mont_digit(acc):
    return ((acc & 0xFFFFFFFF) * NP0) & MASK


def h_sqr4_l(a, b, st):
    """pfp.hpp h_sqr4_l for both lanes: a = (even lane's limbs, odd lane's limbs), the same for b;
    returns ((A even, A odd), (B even, B odd)).  The two lanes run in lock step, as the wave does,
    because column k's limb of b^2 crosses the pair."""
    L = []
    for j in (0, 1):
        sm = -1 if j == 0 else 0
        own_a, pa, own_b, pb = a[j], a[1 - j], b[j], b[1 - j]
        xa = [i32(e + p) for e, p in zip(a[0], pa)]            # dpp<DPP_EVEN>(a) + dpp<DPP_SWAP>(a)
        ya = [i32(o - (p & sm)) for o, p in zip(own_a, pa)]
        xb = [i32(e + p) for e, p in zip(b[0], pb)]
        yb = [i32(o - (p & sm)) for o, p in zip(own_b, pb)]
        xs = [i32(u + v) for u, v in zip(xa, xb)]
        ys = [i32(u + v) for u, v in zip(ya, yb)]
        assert all(abs(c) < 1 << 29 for c in xa + xb) and all(abs(c) < 1 << 28 for c in ya[:-1] + yb[:-1])
        assert all(abs(c) <= (1 << 30) - 4 for c in xs) and all(abs(c) <= (1 << 29) - 2 for c in ys)
        L.append(dict(xa=xa, ya=ya, xb=xb, yb=yb, xs=xs, ys=ys, cb=0, ra=0, rc=0, mA=[], mC=[],
                      A=[None] * NL, C=[None] * NL, SB=0, W=0))
    for k in range(2 * NL - 1):
        ext = []
        for s in L:
            lo, hi = (0, k) if k < NL else (k - NL + 1, NL - 1)
            for i in range(lo, hi + 1):
                s["ra"] = i64(s["ra"] + s["xa"][i] * s["ya"][k - i])
                s["cb"] = i64(s["cb"] + s["xb"][i] * s["yb"][k - i])
                s["rc"] = i64(s["rc"] + s["xs"][i] * s["ys"][k - i])
            st.col = max(st.col, abs(s["cb"]))
            lb = s["cb"] & MASK
            s["cb"] >>= 28
            ext.append(lb)
        for j, s in enumerate(L):
            lb, plb = ext[j], ext[1 - j]             # plb: dpp<DPP_SWAP>(lb)
            sm = -1 if j == 0 else 0
            w = i32((plb ^ sm) - sm)
            assert w == (-plb if j == 0 else plb)
            s["SB"] += lb << (28 * k)
            s["W"] += w << (28 * k)
            s["ra"] = i64(s["ra"] + i32(lb + w))
            s["rc"] = i64(s["rc"] + w)
            for acc, m, out in (("ra", "mA", "A"), ("rc", "mC", "C")):
                if k < NL:
                    for i in range(k):
                        s[acc] = i64(s[acc] + s[m][i] * P_L[k - i])
                    s[m].append(mont_digit(s[acc]))
                    assert 0 <= s[m][k] <= MASK
                    s[acc] = i64(s[acc] + s[m][k] * P_L[0])
                    assert s[acc] & MASK == 0
                else:
                    for i in range(k - NL + 1, NL):
                        s[acc] = i64(s[acc] + s[m][i] * P_L[k - i])
                    s[out][k - NL] = s[acc] & MASK
                st.red = max(st.red, abs(s[acc]))
                s[acc] >>= 28
    tops = [i32(s["cb"]) for s in L]
    for s, t in zip(L, tops):
        assert t == s["cb"] and abs(t) < 1 << 16
    out = []
    for j, s in enumerate(L):
        sm = -1 if j == 0 else 0
        tb, tw = tops[j], i32((tops[1 - j] ^ sm) - sm)
        s["SB"] += tb << (28 * (2 * NL - 1))
        s["W"] += tw << (28 * (2 * NL - 1))
        assert i32(s["ra"]) == s["ra"] and i32(s["rc"]) == s["rc"]
        s["A"][NL - 1] = i32(i32(s["ra"]) + i32(tb + tw))
        s["C"][NL - 1] = i32(i32(s["rc"]) + tw)
        A, Cc = s["A"], s["C"]
        B = [i32(c - x) for c, x in zip(Cc, A)]
        # the unreduced sums are the integers the comment says, and the outputs their reductions
        va, vpa, vb, vpb = val(a[j]), val(a[1 - j]), val(b[j]), val(b[1 - j])
        sq = (lambda o, p: (o + p) * (o - p)) if j == 0 else (lambda o, p: 2 * p * o)
        sq_partner = (lambda o, p: 2 * o * p) if j == 0 else (lambda o, p: (p + o) * (p - o))
        Sa, Sb, Sbp, Ss = sq(va, vpa), sq(vb, vpb), sq_partner(vb, vpb), sq(va + vb, vpa + vpb)
        assert s["SB"] == Sb and s["W"] == (-Sbp if j == 0 else Sbp)
        TA, TC = Sa + Sb + s["W"], Ss + s["W"]
        assert abs(TA) < 48 * P * P and abs(TC) < 80 * P * P
        assert val(A) << RBITS == TA + val(s["mA"]) * P
        assert val(Cc) << RBITS == TC + val(s["mC"]) * P
        for c in (A, Cc):
            assert is_norm(c) and -P // 20 < val(c) < P + P // 20
        # B's contract: lazy
        assert all(abs(c) < 1 << 28 for c in B) and abs(B[-1]) < 1 << 19 and abs(val(B)) < 11 * P // 10
        assert (val(B) << RBITS) % P == (Ss - Sa - Sb) % P
        out.append((A, B))
    return (out[0][0], out[1][0]), (out[0][1], out[1][1])


def check_values(a, b, A, B):
    fa, fb = f2_of(a), f2_of(b)
    wa, wb = sqr4(fa, fb)
    assert f2_of(A) == k2(wa, RINV) and f2_of(B) == k2(wb, RINV)


def test_leaf_limb_model_at_the_contract_ends():
    st = Stats()
    n = 0
    for signs in itertools.product((1, -1), repeat=4):
        for lows in itertools.product((0, 1), repeat=4):
            comp = [extreme(2 * P, s, l) for s, l in zip(signs, lows)]
            a, b = (comp[0], comp[1]), (comp[2], comp[3])
            A, B = h_sqr4_l(a, b, st)
            check_values(a, b, A, B)
            n += 1
    assert n == 256
    # the unnormalised pair of a + b goes into C's Montgomery chain: its columns came near 14 x 2^59
    # + 14 x 2^56 and stayed inside int64; b^2's own chain is far below
    assert 1 << 62 < st.red < (14 << 59) + (14 << 56) + (1 << 37) < 1 << 63
    assert st.col < 14 << 57


def test_leaf_limb_model_limbs_all_ones():
    """not values the contract's |.| < 2p allows at the top limb, but every lower limb at its end on
    both operands and both lanes, the top limbs at +-2p's: the largest columns a normalised input
    can give"""
    st = Stats()
    top = (2 * P) >> (28 * (NL - 1))
    for ta, tb, tc, td in itertools.product((top - 1, -top), repeat=4):
        mk = lambda t: [MASK] * (NL - 1) + [t]
        a, b = (mk(ta), mk(tb)), (mk(tc), mk(td))
        A, B = h_sqr4_l(a, b, st)
        check_values(a, b, A, B)
    assert st.red < (14 << 59) + (14 << 56) + (1 << 37) and st.col < 14 << 57


def test_leaf_limb_model_random_and_small_operands():
    rng = random.Random(0x6c656166)
    st = Stats()
    pick = lambda: rng.choice((0, 1, -1, P - 1, P, rng.randrange(P), -rng.randrange(P), rng.randrange(2 * P)))
    for _ in range(300):
        a, b = (limbs(pick()), limbs(pick())), (limbs(pick()), limbs(pick()))
        A, B = h_sqr4_l(a, b, st)
        check_values(a, b, A, B)
    zero = limbs(0)
    A, B = h_sqr4_l((zero, zero), (zero, zero), st)
    assert all(val(c) == 0 for c in A + B)  # 1 compressed: zeros stay zeros, limb for limb


# ---------------------------------------------------------------- the callers' carry passes
def caller_passes(A, B, ak_lo, ak_hi, with_xi):
    """3 A - 2 a_k and 3 B + 2 a_k (B through xi for the block that needs it: h_add_xi_l(0, B))"""
    lo = fp_red_mk(3, -2, A, ak_lo)
    t = h_xi_l(B) if with_xi else B
    for j in (0, 1):
        assert all(abs(c) < 1 << 31 for c in t[j])
        assert abs(3 * val(A[j]) - 2 * val(ak_lo[j])) < 64 * P and abs(3 * val(t[j]) + 2 * val(ak_hi[j])) < 64 * P
    hi = fp_red_mk(3, 2, t, ak_hi)
    for c in lo + hi:
        assert is_norm(c) and -P // 1000 < val(c) < P + P // 1000  # reduced: the next squaring's input
    fA, fB, fl, fh = f2_of(A), f2_of(B), f2_of(ak_lo), f2_of(ak_hi)
    assert f2_of(lo) == sub(k2(fA, 3), k2(fl, 2))
    assert f2_of(hi) == add(k2(xi(fB) if with_xi else fB, 3), k2(fh, 2))


def lazy_end(sign, low):
    """B at an end of its contract: |limb| < 2^28 with the low limbs all +-(2^28 - 1) or all zeros, the
    value at +-1.1p"""
    top = (11 * P // 10) >> (28 * (NL - 1))
    l = [sign * MASK * low] * (NL - 1) + [sign * (top - 1)]
    assert all(abs(c) < 1 << 28 for c in l) and abs(l[-1]) < 1 << 19 and P < abs(val(l)) < 11 * P // 10
    return l


def test_callers_passes_at_the_ends_of_the_leaf_range():
    """leaf outputs chosen by hand: A at the ends of (-p/20, p + p/20), low limbs all ones or all
    zeros; B at the ends of its lazy contract; on either lane, against a_k at +-2p"""
    ends = [extreme(P + P // 20, 1, 1), extreme(P + P // 20, 1, 0), extreme(P // 20, -1, 1), extreme(P // 20, -1, 0)]
    bends = [lazy_end(1, 1), lazy_end(1, 0), lazy_end(-1, 1), lazy_end(-1, 0)]
    aks = [extreme(2 * P, 1, 1), extreme(2 * P, -1, 0), extreme(2 * P, -1, 1), extreme(2 * P, 1, 0)]
    n = 0
    for ia, ib in itertools.product(range(4), repeat=2):
        for shift in range(4):
            A = (ends[ia], ends[(ia + shift) % 4])
            B = (bends[ib], bends[(ib + shift + 1) % 4])
            for ik in range(4):
                ak_lo = (aks[ik], aks[(ik + shift) % 4])
                ak_hi = (aks[(ik + 1) % 4], aks[(ik + 2 + shift) % 4])
                for with_xi in (False, True):
                    caller_passes(A, B, ak_lo, ak_hi, with_xi)
                    n += 1
    assert n == 512


def test_squaring_chain_in_limb_form():
    """hc_sqr and h12_cyclo_sqr in limb form, fed their own outputs: a cyclotomic element's chain of
    squarings stays reduced and stays the oracle's"""
    rng = random.Random(0x636861)
    st = Stats()
    f = cyclotomic(rng)
    R = 1 << RBITS
    to_l = lambda c: (limbs(c[0] * R % P), limbs(c[1] * R % P))
    g = tuple(tuple(to_l(c) for c in six) for six in f)
    from_l = lambda c: k2(f2_of(c), RINV)

    def block(a, b, ak_lo, ak_hi, with_xi):
        A, B = h_sqr4_l(a, b, st)
        t = h_xi_l(B) if with_xi else B
        return fp_red_mk(3, -2, A, ak_lo), fp_red_mk(3, 2, t, ak_hi)

    for _ in range(3):
        (a0, a2, a4), (a1, a3, a5) = g
        c00, c11 = block(a0, a3, a0, a3, False)
        c01, c12 = block(a1, a4, a2, a5, False)
        c02, c10 = block(a2, a5, a4, a1, True)
        g = ((c00, c01, c02), (c10, c11, c12))
        f = C.f12_sqr(f)
        assert tuple(tuple(from_l(c) for c in six) for six in g) == f
        for six in g:
            for c in six:
                assert all(is_norm(c[j]) and abs(val(c[j])) < 2 * P for j in (0, 1))
