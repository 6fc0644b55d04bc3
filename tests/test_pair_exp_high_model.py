"""t^105 of the lane-pair kernel's exponentiation by x (csrc/k_pair.hip h_exp_high), restated over the
oracle's Fp12 arithmetic.

|x| >> 57 = 105 = 7 x 15, and in the cyclotomic subgroup an inverse is a conjugate, so
u = t^8 conj(t) and u^16 conj(u) take seven Granger-Scott squarings and two products where
square-and-multiply from the top takes six and three.  Both are restated here with h12_cyclo_sqr's
formulas (csrc/pfp.hpp) and compared on random cyclotomic elements and on 1, which is what a pair at
infinity hands the final exponentiation.  The chain's one new kind of operand, the conjugate of a
reduced element as h12_mul's second factor, is followed through h12_mul in the kernel's limb form
(the last section).
"""
import random

from oracle import bls12_381 as C
from tests.test_pair_toom_model import (RINV, Contract, extreme, f2_of, fp_add, fp_addl, fp_norm, fp_red_mk, h_xi_l, i32,
                                        is_norm, lane, val)

P = C.P
add, sub, sqr, xi = C.f2_add, C.f2_sub, C.f2_sqr, C.f2_mul_xi
EXP_HIGH = C.X_ABS >> 57


def k2(a, n):
    return C.f2_muls(a, n % P)


def cyclo_sqr(f):
    """h12_cyclo_sqr: f = (a0 + a2 v + a4 v^2) + (a1 + a3 v + a5 v^2) w"""
    (a0, a2, a4), (a1, a3, a5) = f

    def block(x, y):
        sx, sy, sxy = sqr(x), sqr(y), sqr(add(x, y))
        return add(sx, xi(sy)), sub(sub(sxy, sx), sy)

    A0, A3 = block(a0, a3)
    A2, A5 = block(a1, a4)
    A4, A1 = block(a2, a5)
    A1 = xi(A1)
    lo = lambda A, a: sub(k2(A, 3), k2(a, 2))
    hi = lambda A, a: add(k2(A, 3), k2(a, 2))
    return ((lo(A0, a0), lo(A2, a2), lo(A4, a4)), (hi(A1, a1), hi(A3, a3), hi(A5, a5)))


def exp_high_bits(t):
    """square-and-multiply from the top: 6 squarings, 3 products"""
    r, ops = t, [0, 0]
    for b in range(EXP_HIGH.bit_length() - 2, -1, -1):
        r = cyclo_sqr(r)
        ops[0] += 1
        if (EXP_HIGH >> b) & 1:
            r = C.f12_mul(r, t)
            ops[1] += 1
    return r, ops


def exp_high_chain(t):
    """h_exp_high: two passes of r <- r^(2^(3 + pass)) conj(b), b <- r"""
    r, b, ops = t, t, [0, 0]
    for n in (3, 4):
        for _ in range(n):
            r = cyclo_sqr(r)
            ops[0] += 1
        r = C.f12_mul(r, C.f12_conj(b))
        ops[1] += 1
        b = r
    return r, ops


def cyclotomic(rng):
    f = tuple(tuple((rng.randrange(P), rng.randrange(P)) for _ in range(3)) for _ in range(2))
    g = C.f12_mul(C.f12_conj(f), C.f12_inv(f))  # f^(p^6 - 1)
    return C.f12_mul(C.f12_frob(g, 2), g)       # ^(p^2 + 1)


def test_exp_high_chain_is_the_bit_loop():
    assert EXP_HIGH == 105 == 7 * 15
    rng = random.Random(0x313035)
    for t in [C.F12_ONE] + [cyclotomic(rng) for _ in range(6)]:
        assert cyclo_sqr(t) == C.f12_sqr(t)  # t is cyclotomic: Granger-Scott's formulas apply
        assert C.f12_mul(t, C.f12_conj(t)) == C.F12_ONE  # and its inverse is its conjugate
        want, ops = exp_high_bits(t)
        assert ops == [6, 3]
        got, ops = exp_high_chain(t)
        assert ops == [7, 2]
        assert got == want == C.f12_pow(t, 105)
    assert exp_high_chain(C.F12_ONE)[0] == C.F12_ONE


def test_chain_needs_the_cyclotomic_subgroup():
    """outside it the conjugate is no inverse: the chain is only for final_exp's hard part"""
    rng = random.Random(0x6e6f74)
    f = tuple(tuple((rng.randrange(P), rng.randrange(P)) for _ in range(3)) for _ in range(2))
    assert C.f12_mul(f, C.f12_conj(f)) != C.F12_ONE


# ---------------------------------------------------------------- limbs: conj(b) as h12_mul's operand
# The chain hands h12_mul the conjugate of a reduced element (csrc/pfp.hpp h12_conj: fp_neg on the
# three components of c1).  In the kernel's limb form (the helpers of test_pair_toom_model.py), with
# every component of r and b at +-2p and the low limbs all ones or all zeros: the negation is
# normalised and below 2p, every h_mul operand of h12_mul's three Karatsuba Fp6 products is inside its
# contract (a lazy with |limb| <= 2^29, b normalised, both < 16p; the sums of two components < 4p),
# every int32 / int64 holds, and the output is reduced and is the product.
fp_neg = lane(lambda a: fp_norm([i32(-x) for x in a]))
fp_sub2l = lane(lambda a, b, c: [i32(x - y - z) for x, y, z in zip(a, b, c)])


def fp_red_l(t):
    return fp_red_mk(1, 0, t, t)


def h_add_xi_l(s, t):
    return fp_addl(s, h_xi_l(t))


def h6_mul(a, b, ct):
    """pfp.hpp h6_mul, statement by statement"""
    v1 = ct.h_mul(a[1], b[1])
    v2 = ct.h_mul(a[2], b[2])
    d0 = fp_sub2l(ct.h_mul(fp_addl(a[1], a[2]), fp_add(b[1], b[2])), v1, v2)
    v0 = ct.h_mul(a[0], b[0])
    c0 = fp_red_l(h_add_xi_l(v0, d0))
    c1 = fp_red_l(h_add_xi_l(fp_sub2l(ct.h_mul(fp_addl(a[0], a[1]), fp_add(b[0], b[1])), v0, v1), v2))
    c2 = fp_red_l(fp_addl(fp_sub2l(ct.h_mul(fp_addl(a[0], a[2]), fp_add(b[0], b[2])), v0, v2), v1))
    return (c0, c1, c2)


def h12_mul(a, b, ct):
    """pfp.hpp h12_mul and h12_kcomb"""
    h6_add = lambda x, y: tuple(fp_add(p, q) for p, q in zip(x, y))
    t0, t1 = h6_mul(a[0], b[0], ct), h6_mul(a[1], b[1], ct)
    sa, sb = h6_add(a[0], a[1]), h6_add(b[0], b[1])
    for c in sa + sb:
        assert all(is_norm(c[j]) and abs(val(c[j])) < 4 * P for j in (0, 1))
    s = h6_mul(sa, sb, ct)
    return ((fp_red_l(h_add_xi_l(t0[0], t1[2])), fp_red_l(fp_addl(t0[1], t1[0])), fp_red_l(fp_addl(t0[2], t1[1]))),
            tuple(fp_red_l(fp_sub2l(s[k], t0[k], t1[k])) for k in range(3)))


def f12_of(a):
    return tuple(tuple(f2_of(c) for c in six) for six in a)


def test_conjugate_operand_in_limb_form():
    rng = random.Random(0x636f6e6a)
    ct = Contract()
    reduced = lambda: tuple(tuple((extreme(2 * P, rng.choice((1, -1)), low), extreme(2 * P, rng.choice((1, -1)), low))
                                  for low in (rng.choice((0, 1)),) * 3) for _ in range(2))
    for _ in range(40):
        r, b = reduced(), reduced()
        cb = (b[0], tuple(fp_neg(c) for c in b[1]))  # h12_conj
        for c in cb[1]:
            assert all(is_norm(c[j]) and abs(val(c[j])) < 2 * P for j in (0, 1))
        assert f12_of(cb) == C.f12_conj(f12_of(b))
        out = h12_mul(r, cb, ct)
        for six in out:
            for c in six:
                assert all(is_norm(c[j]) and abs(val(c[j])) < 2 * P for j in (0, 1))
        want = C.f12_mul(f12_of(r), f12_of(cb))
        assert f12_of(out) == tuple(tuple(k2(c, RINV) for c in six) for six in want)
    assert ct.calls == 40 * 18 and ct.max_a > 7 * P and ct.max_b > 39 * P // 10
