"""The lane-pair kernel's compressed exponentiation by |x| (csrc/k_pair.hip h_exp_abs_x, csrc/pfp.hpp
hc_sqr / hc_decompress) over the oracle's Fp2 arithmetic.

The kernel's formula sequence is restated here exactly as the sources state it: compressed squarings
on (a1, a2, a4, a5) from the bottom bit up to bit EXP_TOP, the compressed value saved at |x|'s set
bits on the way, one shared Fp2 inversion of the saved denominators 4 a1 (prefix products, one
inversion, back-substitution), a3 and a0 of each saved power, the highest one raised to
|x| >> EXP_TOP with Granger-Scott squarings, the product of the powers (and of the base for
|x| + 1), and the Granger-Scott square-and-multiply loop when a denominator is zero.

The kernel stops compressing at EXP_TOP = 57 (three saved powers).  The formulas are also checked
with top = 63: all 63 squarings compressed and all six powers decompressed by one inversion.

a_k is the coefficient of w^k: an Fp12 value ((c00, c01, c02), (c10, c11, c12)) has
(a0, a1, a2, a3, a4, a5) = (c00, c10, c01, c11, c02, c12).
"""
import random

import pytest

from oracle import bls12_381 as C

add, sub, mul, sqr = C.f2_add, C.f2_sub, C.f2_mul, C.f2_sqr
xi = C.f2_mul_xi
SET_BITS = [k for k in range(64) if (C.X_ABS >> k) & 1]
EXP_TOP = 57   # k_pair.hip EXP_TOP
TOPS = [EXP_TOP, 63]


def k(a, n):
    return C.f2_muls(a, n % C.P)


def coeffs(f):
    (a0, a2, a4), (a1, a3, a5) = f
    return a0, a1, a2, a3, a4, a5


def compress(f):
    _, a1, a2, _, a4, a5 = coeffs(f)
    return a1, a2, a4, a5


# ---------------------------------------------------------------- pfp.hpp
def hc_sqr(c):
    a1, a2, a4, a5 = c
    s1, s4, s14 = sqr(a1), sqr(a4), sqr(add(a1, a4))
    r2 = sub(k(add(s1, xi(s4)), 3), k(a2, 2))
    r5 = add(k(sub(sub(s14, s1), s4), 3), k(a5, 2))
    s2, s5, s25 = sqr(a2), sqr(a5), sqr(add(a2, a5))
    r4 = sub(k(add(s2, xi(s5)), 3), k(a4, 2))
    r1 = add(k(xi(sub(sub(s25, s2), s5)), 3), k(a1, 2))
    return r1, r2, r4, r5


def hc_denom(a1):
    return k(a1, 4)


def hc_decompress(c, di):
    a1, a2, a4, a5 = c
    s5, s2 = sqr(a5), sqr(a2)
    a3 = mul(sub(add(xi(s5), k(s2, 3)), k(a4, 2)), di)
    u = add(sub(k(sqr(a3), 2), k(mul(a4, a2), 3)), mul(a1, a5))
    a0 = add(C.F2_ONE, xi(u))
    return ((a0, a2, a4), (a1, a3, a5))


def cyclo_sqr(f):
    """h12_cyclo_sqr (Granger-Scott): the fallback's squaring"""
    a0, a1, a2, a3, a4, a5 = coeffs(f)
    s0, s3, s03 = sqr(a0), sqr(a3), sqr(add(a0, a3))
    r0 = sub(k(add(s0, xi(s3)), 3), k(a0, 2))
    r3 = add(k(sub(sub(s03, s0), s3), 3), k(a3, 2))
    r1, r2, r4, r5 = hc_sqr((a1, a2, a4, a5))
    return ((r0, r2, r4), (r1, r3, r5))


# ---------------------------------------------------------------- k_pair.hip
class Count:
    def __init__(self):
        self.inv = self.prod = self.fallback = 0


def exp_gs(base, plus1):
    e = C.X_ABS + (1 if plus1 else 0)
    r = base
    for b in range(62, -1, -1):
        r = cyclo_sqr(r)
        if (e >> b) & 1:
            r = C.f12_mul(r, base)
    return r


def exp_high(t, top):
    """t^(|x| >> top): the squarings above bit top run uncompressed"""
    high = C.X_ABS >> top
    r = t
    for b in range(64 - top - 2, -1, -1):
        r = cyclo_sqr(r)
        if (high >> b) & 1:
            r = C.f12_mul(r, t)
    return r


def exp_tail(parked, base, plus1, cnt, top, powers=None):
    """None if a denominator is zero"""
    pre = []
    n = len(parked)
    for j in range(n):
        d = hc_denom(parked[j][0])
        if j == 0:
            p = d
        else:
            p = mul(p, d)
            cnt.prod += 1
        pre.append(p)
    if C.f2_is_zero(p):
        return None
    inv = C.f2_inv(p)
    cnt.inv += 1
    acc = None
    for j in range(n - 1, -2 if plus1 else -1, -1):
        if j >= 0:
            c = parked[j]
            di = inv
            if j > 0:
                di = mul(inv, pre[j - 1])
                inv = mul(inv, hc_denom(c[0]))
                cnt.prod += 2
            e = hc_decompress(c, di)
            if powers is not None:
                powers[j] = e
        else:
            e = base
        acc = exp_high(e, top) if j == n - 1 else C.f12_mul(acc, e)
    return acc


def exp_abs_x(base, plus1, cnt, chain=None, powers=None, force_zero_at=None, top=None):
    top = EXP_TOP if top is None else top
    c = compress(base)
    parked = []
    for b in range(1, top + 1):
        c = hc_sqr(c)
        if chain is not None:
            chain.append(c)
        if (C.X_ABS >> b) & 1:
            parked.append((C.F2_ZERO,) + c[1:] if force_zero_at == len(parked) else c)
    assert len(parked) == sum(1 for b in SET_BITS if b <= top) and (C.X_ABS >> top) & 1
    r = exp_tail(parked, base, plus1, cnt, top, powers)
    if r is None:
        cnt.fallback += 1
        r = exp_gs(base, plus1)
    return r


# ---------------------------------------------------------------- inputs
def _rand_f12(rng):
    return tuple(tuple((rng.randrange(C.P), rng.randrange(C.P)) for _ in range(3)) for _ in range(2))


def _cyclotomic(seed):
    """a random Fp12 through the easy part of the final exponentiation"""
    f = _rand_f12(random.Random(seed))
    f1 = C.f12_mul(C.f12_conj(f), C.f12_inv(f))
    return C.f12_mul(C.f12_frob(f1, 2), f1)


@pytest.fixture(scope="module", params=[0x72313061, 0x72313062, 0x72313063])
def elem(request):
    g = _cyclotomic(request.param)
    assert g != C.F12_ONE
    return g


def test_set_bits():
    assert SET_BITS == [16, 48, 57, 60, 62, 63]
    assert C.X_ABS & 1 == 0
    assert C.X_ABS >> EXP_TOP == 105


def test_compressed_squarings_follow_the_plain_chain(elem):
    chain = []
    exp_abs_x(elem, False, Count(), chain=chain, top=63)
    assert len(chain) == 63
    f = elem
    for step, c in enumerate(chain):
        f = C.f12_sqr(f)
        assert c == compress(f), step


def test_shared_inversion_decompresses_the_six_powers(elem):
    cnt, powers = Count(), {}
    exp_abs_x(elem, False, cnt, powers=powers, top=63)
    assert sorted(powers) == list(range(6))
    for j, b in enumerate(SET_BITS):
        assert powers[j] == C.f12_pow(elem, 1 << b), b
    assert (cnt.inv, cnt.prod, cnt.fallback) == (1, 15, 0)


def test_shared_inversion_decompresses_the_kernels_powers(elem):
    cnt, powers = Count(), {}
    exp_abs_x(elem, False, cnt, powers=powers)
    assert sorted(powers) == [0, 1, 2]
    for j, b in enumerate([16, 48, 57]):
        assert powers[j] == C.f12_pow(elem, 1 << b), b
    assert exp_high(powers[2], EXP_TOP) == C.f12_pow(elem, 105 << 57)
    assert (cnt.inv, cnt.prod, cnt.fallback) == (1, 6, 0)


@pytest.mark.parametrize("top", TOPS)
def test_products(elem, top):
    cnt = Count()
    assert exp_abs_x(elem, False, cnt, top=top) == C.f12_pow(elem, C.X_ABS)
    assert exp_abs_x(elem, True, cnt, top=top) == C.f12_pow(elem, C.X_ABS + 1)
    assert (cnt.inv, cnt.fallback) == (2, 0)


def test_fallback_equals_the_plain_chain(elem):
    assert exp_gs(elem, False) == C.f12_pow(elem, C.X_ABS)
    assert exp_gs(elem, True) == C.f12_pow(elem, C.X_ABS + 1)


@pytest.mark.parametrize("top", TOPS)
@pytest.mark.parametrize("plus1", [False, True])
def test_zero_predicate_one(plus1, top):
    """g = 1 (a pair at infinity) compresses to four zeros and stays there"""
    assert compress(C.F12_ONE) == (C.F2_ZERO,) * 4
    assert hc_sqr((C.F2_ZERO,) * 4) == (C.F2_ZERO,) * 4
    cnt = Count()
    assert exp_abs_x(C.F12_ONE, plus1, cnt, top=top) == C.F12_ONE
    assert (cnt.inv, cnt.fallback) == (0, 1)


@pytest.mark.parametrize("top", TOPS)
@pytest.mark.parametrize("plus1", [False, True])
def test_zero_predicate_all_zero(plus1, top):
    """a degenerate f = 0: every later value is 0, as with the plain chain"""
    zero = (C.F6_ZERO, C.F6_ZERO)
    cnt = Count()
    assert exp_abs_x(zero, plus1, cnt, top=top) == zero
    assert (cnt.inv, cnt.fallback) == (0, 1)


@pytest.mark.parametrize("top,slot", [(EXP_TOP, s) for s in range(3)] + [(63, s) for s in range(6)])
def test_zero_predicate_one_denominator(elem, top, slot):
    """a1 = 0 at one saved bit: the shared product sees it and the plain chain's value comes back"""
    cnt = Count()
    assert exp_abs_x(elem, True, cnt, force_zero_at=slot, top=top) == C.f12_pow(elem, C.X_ABS + 1)
    assert (cnt.inv, cnt.fallback) == (0, 1)
