"""The lane-pair Miller loop's five-product Fp6 multiplication (csrc/pfp.hpp h6_mul6), restated twice.

Values, over the oracle's Fp2 arithmetic: h6_mul6 is 6 times the Karatsuba product, h12_sqr and
h12_mul_lines built from it (and from the sparse product brought to the same factor) are 6 times the
exact results, and a Miller value times a power of 6 enters the final exponentiation as the same
element: f^(p^6 - 1), its first step, removes any factor in Fp.

Bounds, over Python integers in the kernel's limb form (14 signed limbs of 28 bits, Montgomery
R = 2^392, an Fp2 value as the even and the odd lane's component): every statement of h6_mul6 and of
the scaled h6_mul_12 in the order pfp.hpp has them, with a check on every int32 value, every int64
column sum and carry, every h_mul operand (a lazy with |limb| <= 2^29, b normalised, both < 16p)
and every output (normalised, |.| < 2p).  The operands stand at the contract's extremes: values at
+-4p (b: +-16p / 7, so that |b0| + 2 |b1| + 4 |b2| < 16p) with the low limbs all ones or all zeros.
The interpolation is run again on products chosen by hand, normalised limbs all ones or all zeros on
either lane and the values at the ends of a product's range, which real operands cannot be steered
to.
"""
import itertools
import random

from oracle import bls12_381 as C

P = C.P
NL = 14
MASK = (1 << 28) - 1
RBITS = 28 * NL
P_L = [(P >> (28 * i)) & MASK for i in range(NL)]
NP0 = (-pow(P, -1, 1 << 28)) % (1 << 28)
QINV = (1 << 396) // P
assert QINV == 40323

add, sub, mul, neg, xi = C.f2_add, C.f2_sub, C.f2_mul, C.f2_neg, C.f2_mul_xi


def k2(a, n):
    return C.f2_muls(a, n % P)


def k6(a, n):
    return tuple(k2(c, n) for c in a)


def k12(a, n):
    return (k6(a[0], n), k6(a[1], n))


# ---------------------------------------------------------------- values
def toom6(a, b):
    """h6_mul6's formulas"""
    a0, a1, a2 = a
    b0, b1, b2 = b
    sa = add(a0, a2)
    p1 = mul(add(sa, a1), add(add(b0, b1), b2))
    pm = mul(sub(sa, a1), add(sub(b0, b1), b2))
    p0 = mul(a0, b0)
    pi = mul(a2, b2)
    xpi = xi(pi)
    w = sub(sub(add(p1, pm), k2(p0, 2)), k2(pi, 2))
    m = sub(k2(sub(p0, p1), 3), pm)
    e = sub(p1, pm)
    k = sub(p0, k2(xpi, 2))
    h = add(k2(pi, 2), xpi)
    c2 = k2(w, 3)
    p2 = mul(add(add(a0, k2(a1, 2)), k2(a2, 4)), add(add(b0, k2(b1, 2)), k2(b2, 4)))
    t = add(p2, m)
    c0 = add(xi(t), k2(k, 6))
    c1 = add(sub(k2(e, 3), t), k2(h, 6))
    return (c0, c1, c2)


def mul_12(x, b1, b2, s):
    """h6_mul_12<S>: x (b1 v + b2 v^2), times s"""
    u = mul(x[1], b1)
    w = mul(x[2], b2)
    c0 = xi(sub(sub(mul(add(x[1], x[2]), add(b1, b2)), u), w))
    c1 = add(mul(x[0], b1), xi(w))
    c2 = add(mul(x[0], b2), u)
    return (k2(c0, s), k2(c1, s), k2(c2, s))


def h12_sqr(a, mul6):
    t = mul6(a[0], a[1])
    s = mul6(C.f6_add(a[0], a[1]), C.f6_add(a[0], C.f6_mul_v(a[1])))
    c0 = (add(sub(s[0], t[0]), xi(neg(t[2]))), sub(sub(s[1], t[1]), t[0]), sub(sub(s[2], t[2]), t[1]))
    return (c0, C.f6_add(t, t))


def line_product(la, lb):
    a0, a1, a4 = la
    b0, b1, b4 = lb
    a0b0, a1b1, a4b4 = mul(a0, b0), mul(a1, b1), mul(a4, b4)
    c11 = sub(sub(mul(add(a0, a4), add(b0, b4)), a0b0), a4b4)
    c12 = sub(sub(mul(add(a1, a4), add(b1, b4)), a1b1), a4b4)
    C0 = (add(a0b0, xi(a4b4)), sub(sub(mul(add(a0, a1), add(b0, b1)), a0b0), a1b1), a1b1)
    return C0, c11, c12


def h12_mul_lines(f, la, lb, mul6, s):
    C0, c11, c12 = line_product(la, lb)
    t0 = mul6(f[0], C0)
    t1 = mul_12(f[1], c11, c12, s)
    sm = mul6(C.f6_add(f[0], f[1]), (C0[0], add(C0[1], c11), add(C0[2], c12)))
    return (C.f6_add(t0, C.f6_mul_v(t1)), C.f6_sub(C.f6_sub(sm, t0), t1))


def line12(l):
    """c0 + c1 w^2 + c4 w^3 with w^2 = v"""
    return ((l[0], l[1], C.F2_ZERO), (C.F2_ZERO, l[2], C.F2_ZERO))


def rnd2(rng):
    return (rng.randrange(P), rng.randrange(P))


def rnd6(rng):
    return (rnd2(rng), rnd2(rng), rnd2(rng))


def edge6(rng):
    return tuple((rng.choice((0, 1, P - 1)), rng.choice((0, 1, P - 1))) for _ in range(3))


def test_mul6_is_six_times_karatsuba():
    rng = random.Random(0x746f6f6d)
    cases = [(rnd6(rng), rnd6(rng)) for _ in range(200)]
    cases += [(edge6(rng), edge6(rng)) for _ in range(300)]
    cases += [(edge6(rng), rnd6(rng)) for _ in range(50)] + [(rnd6(rng), edge6(rng)) for _ in range(50)]
    for v in (0, 1, P - 1):
        for w in (0, 1, P - 1):
            cases.append((((v, v),) * 3, ((w, w),) * 3))
            cases.append((((v, 0), (0, v), (v, v)), ((0, w), (w, w), (w, 0))))
    for a, b in cases:
        assert toom6(a, b) == k6(C.f6_mul(a, b), 6)


def test_sqr_and_line_step_carry_the_factor():
    rng = random.Random(0x6c696e65)
    for _ in range(20):
        f = (rnd6(rng), rnd6(rng))
        assert h12_sqr(f, toom6) == k12(C.f12_sqr(f), 6)
        assert h12_sqr(f, C.f6_mul) == C.f12_sqr(f)
        la, lb = tuple(rnd2(rng) for _ in range(3)), tuple(rnd2(rng) for _ in range(3))
        want = C.f12_mul(f, C.f12_mul(line12(la), line12(lb)))
        assert h12_mul_lines(f, la, lb, toom6, 6) == k12(want, 6)
        assert h12_mul_lines(f, la, lb, C.f6_mul, 1) == want
    # the first step: the line product itself, (C0, (0, c11, c12)), is 1 times the lines
    C0, c11, c12 = line_product(la, lb)
    assert (C0, (C.F2_ZERO, c11, c12)) == C.f12_mul(line12(la), line12(lb))
    # an inactive pair's line is 1
    one = (C.F2_ONE, C.F2_ZERO, C.F2_ZERO)
    assert h12_mul_lines(f, la, one, toom6, 6) == k12(C.f12_mul(f, line12(la)), 6)


def test_scaled_miller_value_has_the_same_final_exponentiation():
    """f -> conj(f) / f is the final exponentiation's first step (f^(p^6 - 1)); everything after it
    is a function of that element"""
    rng = random.Random(0x66657870)
    f = (rnd6(rng), rnd6(rng))
    easy = lambda g: C.f12_mul(C.f12_conj(g), C.f12_inv(g))
    want = easy(f)
    # 63 doubling steps with a square and a line step each, 5 addition steps, less the first square
    for k in (1, 2, 68, 2 * 63 + 5 - 1):
        assert easy(k12(f, pow(6, k, P))) == want


# ---------------------------------------------------------------- limbs
def i32(x):
    assert -(1 << 31) <= x < (1 << 31), x
    return x


def i64(x):
    assert -(1 << 63) <= x < (1 << 63), x
    return x


def val(l):
    return sum(c << (28 * i) for i, c in enumerate(l))


def limbs(v):
    """normalised: limbs 0..12 in [0, 2^28), the top limb signed"""
    return [(v >> (28 * i)) & MASK for i in range(NL - 1)] + [v >> (28 * (NL - 1))]


def is_norm(l):
    return all(0 <= c <= MASK for c in l[:-1]) and -(1 << 31) <= l[-1] < (1 << 31)


def fp_norm(l):
    r = list(l)
    for i in range(NL - 1):
        c = r[i] >> 28
        r[i] &= MASK
        r[i + 1] = i32(r[i + 1] + c)
    return r


def lane(f):
    """an Fp function as one on a lane pair's two components"""
    return lambda *a: tuple(f(*[x[j] if isinstance(x, tuple) else x for x in a]) for j in (0, 1))


fp_addl = lane(lambda a, b: [i32(x + y) for x, y in zip(a, b)])
fp_subl = lane(lambda a, b: [i32(x - y) for x, y in zip(a, b)])
fp_add = lane(lambda a, b: fp_norm([i32(x + y) for x, y in zip(a, b)]))
fp_lin3 = lane(lambda a, k1, b, k2, c: fp_norm([i32(x + k1 * y + k2 * z) for x, y, z in zip(a, b, c)]))


def fp_red_mk_1(M, K, t, a):
    top = i64(t[NL - 1] * M + K * a[NL - 1])
    assert abs(top) < 1 << 23, "the quotient estimate's range"
    q = i32((top * QINV) >> 32)
    r, acc = [], 0
    for i in range(NL - 1):
        acc = i64(acc + i64(t[i] * M) + i64(K * a[i]) - i64(q * P_L[i]))
        r.append(acc & MASK)
        acc >>= 28
    r.append(i32(acc + top - q * P_L[NL - 1]))
    assert val(r) == M * val(t) + K * val(a) - q * P
    return r


def fp_red_mk(M, K, t, a):
    return tuple(fp_red_mk_1(M, K, t[j], a[j]) for j in (0, 1))


def fp_red_124(a, b, c):
    out = []
    for j in (0, 1):
        x, y, z = a[j], b[j], c[j]
        top = i32(x[NL - 1] + 2 * y[NL - 1] + 4 * z[NL - 1])
        assert abs(top) < 1 << 23
        q = i32((top * QINV) >> 32)
        r, acc = [], 0
        for i in range(NL - 1):
            acc = i64(acc + i32(x[i] + 2 * y[i] + 4 * z[i]) - i64(q * P_L[i]))
            r.append(acc & MASK)
            acc >>= 28
        r.append(i32(acc + top - q * P_L[NL - 1]))
        assert val(r) == val(x) + 2 * val(y) + 4 * val(z) - q * P
        out.append(r)
    return tuple(out)


def h_xi_l(t):
    ev, od = t
    return ([i32(x + i32(-y)) for x, y in zip(ev, od)], [i32(y + x) for x, y in zip(ev, od)])


def lane_product(x, Y, Z, W):
    """h_mul_l's two loops for one lane: (x Y + Z W) / R, with every column sum inside int64"""
    m, r, acc = [], [], 0
    for k in range(NL):
        for i in range(k + 1):
            acc = i64(acc + x[i] * Y[k - i])
            acc = i64(acc + Z[i] * W[k - i])
        for i in range(k):
            acc = i64(acc + m[i] * P_L[k - i])
        m.append(((acc & 0xFFFFFFFF) * NP0) & MASK)
        acc = i64(acc + m[k] * P_L[0])
        assert acc & MASK == 0
        acc >>= 28
    for k in range(NL, 2 * NL - 1):
        for i in range(k - NL + 1, NL):
            acc = i64(acc + x[i] * Y[k - i])
            acc = i64(acc + Z[i] * W[k - i])
            acc = i64(acc + m[i] * P_L[k - i])
        r.append(acc & MASK)
        acc >>= 28
    r.append(i32(acc))
    assert val(r) << RBITS == val(x) * val(Y) + val(Z) * val(W) + val(m) * P
    return r


class Contract:
    """what h_mul was handed, over one run"""
    def __init__(self):
        self.calls = 0
        self.max_a = self.max_b = 0

    def h_mul(self, a, b):
        for j in (0, 1):
            assert all(abs(c) <= 1 << 29 for c in a[j]), "a lazy, |limb| <= 2^29"
            assert is_norm(b[j]), "b normalised"
            assert abs(val(a[j])) < 16 * P and abs(val(b[j])) < 16 * P
            self.max_a = max(self.max_a, abs(val(a[j])))
            self.max_b = max(self.max_b, abs(val(b[j])))
        self.calls += 1
        ev = lane_product(a[0], b[0], [i32(-c) for c in a[1]], b[1])  # a0 b0 - a1 b1
        od = lane_product(a[1], b[0], a[0], b[1])                     # a1 b0 + a0 b1
        for r in (ev, od):
            assert is_norm(r) and -P // 4 < val(r) < 4 * P // 3  # h6_mul6's comment: (-0.2p, 1.33p)
        return (ev, od)


def interpolate(p1, pm, p0, pi, p2_of_m):
    """h6_mul6 after its fourth product; p2_of_m: the fifth, called when the kernel calls it"""
    xpi = h_xi_l(pi)
    w, m, e, k, h = [], [], [], [], []
    for j in (0, 1):
        w.append([i32(a + b - 2 * c - 2 * d) for a, b, c, d in zip(p1[j], pm[j], p0[j], pi[j])])
        m.append([i32(3 * i32(c - a) - b) for a, b, c in zip(p1[j], pm[j], p0[j])])
        e.append([i32(a - b) for a, b in zip(p1[j], pm[j])])
        k.append([i32(c - 2 * x) for c, x in zip(p0[j], xpi[j])])
        h.append([i32(2 * d + x) for d, x in zip(pi[j], xpi[j])])
    w, m, e, k, h = tuple(w), tuple(m), tuple(e), tuple(k), tuple(h)
    c2 = fp_red_mk(3, 0, w, w)
    t = fp_addl(p2_of_m(), m)
    c0 = fp_red_mk(1, 6, h_xi_l(t), k)
    g = tuple([i32(3 * a - b) for a, b in zip(e[j], t[j])] for j in (0, 1))
    c1 = fp_red_mk(1, 6, g, h)
    return (c0, c1, c2)


def h6_mul6(a, b, ct):
    sa = fp_add(a[0], a[2])
    p1 = ct.h_mul(fp_addl(sa, a[1]), fp_lin3(b[0], 1, b[1], 1, b[2]))
    pm = ct.h_mul(fp_subl(sa, a[1]), fp_lin3(b[0], -1, b[1], 1, b[2]))
    p0 = ct.h_mul(a[0], b[0])
    pi = ct.h_mul(a[2], b[2])
    return interpolate(p1, pm, p0, pi,
                       lambda: ct.h_mul(fp_red_124(a[0], a[1], a[2]), fp_lin3(b[0], 2, b[1], 4, b[2])))


def h6_mul_12(x, b1, b2, S, ct):
    u = ct.h_mul(x[1], b1)
    w = ct.h_mul(x[2], b2)
    d0 = h_xi_l(fp_subl(fp_subl(ct.h_mul(fp_addl(x[1], x[2]), fp_add(b1, b2)), u), w))
    c0 = fp_red_mk(S, 0, d0, d0)
    d1 = fp_addl(ct.h_mul(x[0], b1), h_xi_l(w))  # h_add_xi_l
    c1 = fp_red_mk(S, 0, d1, d1)
    d2 = fp_addl(ct.h_mul(x[0], b2), u)
    c2 = fp_red_mk(S, 0, d2, d2)
    return (c0, c1, c2)


def out_ok(c):
    return all(is_norm(c[j]) and abs(val(c[j])) < 2 * P for j in (0, 1))


def f2_of(x):
    return (val(x[0]) % P, val(x[1]) % P)


def f6_of(a):
    return tuple(f2_of(x) for x in a)


RINV = pow(1 << RBITS, -1, P)


def extreme(bound, sign, low):
    """a normalised component with |value| < bound, as close to it as the low limbs allow: the low
    limbs all ones (low = 1) or all zeros, the top limb at the bound's"""
    top = bound >> (28 * (NL - 1))
    lo = [MASK * low] * (NL - 1)
    l = lo + [top - 1] if sign > 0 else lo + [-top]
    assert is_norm(l) and abs(val(l)) <= bound
    return l


def extreme_operands():
    """every sign pattern of the six components of a (at 4p) against b (at 16p / 7), low limbs all
    ones or all zeros, the same pattern or the opposite on the partner lane"""
    A, B = 4 * P, 16 * P // 7
    rng = random.Random(0x65646765)
    pats = list(itertools.product((1, -1), repeat=6))
    for sa in pats:
        sb = rng.choice(pats)
        for low_a, low_b in ((1, 1), (0, 0), (1, 0), (0, 1)):
            a = tuple((extreme(A, sa[2 * i], low_a), extreme(A, sa[2 * i + 1], low_a)) for i in range(3))
            b = tuple((extreme(B, sb[2 * i], low_b), extreme(B, sb[2 * i + 1], low_b)) for i in range(3))
            yield a, b


def test_limb_model_values_and_bounds_at_the_contract_extremes():
    ct = Contract()
    n = 0
    for a, b in extreme_operands():
        c = h6_mul6(a, b, ct)
        assert all(out_ok(x) for x in c)
        want = k6(C.f6_mul(f6_of(a), f6_of(b)), 6 * RINV)
        assert f6_of(c) == want
        n += 1
    assert n == 256 and ct.calls == 5 * n
    # the operands really were near the contract's ends
    assert ct.max_a > 11 * P and ct.max_b > 15 * P


def test_limb_model_random_and_small_operands():
    rng = random.Random(0x6c696d62)
    ct = Contract()
    pick = lambda: rng.choice((0, 1, P - 1, rng.randrange(P), -rng.randrange(P), rng.randrange(2 * P)))
    for _ in range(150):
        a = tuple((limbs(pick()), limbs(pick())) for _ in range(3))
        b = tuple((limbs(pick()), limbs(pick())) for _ in range(3))
        c = h6_mul6(a, b, ct)
        assert all(out_ok(x) for x in c)
        assert f6_of(c) == k6(C.f6_mul(f6_of(a), f6_of(b)), 6 * RINV)


def product_extremes():
    """a product by hand: normalised, low limbs all ones or all zeros, the value at either end of
    (-0.2p, 1.33p)"""
    hi, lo = 4 * P // 3, P // 5
    return [extreme(hi, 1, 1), extreme(hi, 1, 0), extreme(lo, -1, 1), extreme(lo, -1, 0)]


def test_interpolation_bounds_on_extreme_products():
    """five products on two lanes, each one of four extremes: 4^10 combinations is too many, so the
    own lane takes all 4^5 and the partner lane a pattern that moves with it (same, opposite ends,
    and two rotations)"""
    ex = product_extremes()
    n = 0
    for idx, own in enumerate(itertools.product(range(4), repeat=5)):
        for shift in (0, 2, 1, 3) if idx % 5 == 0 else (0, 2):  # the rotations on a fifth of the patterns
            ps = [(ex[o], ex[(o + shift) % 4]) for o in own]
            p1, pm, p0, pi, p2 = ps
            c = interpolate(p1, pm, p0, pi, lambda: p2)
            assert all(out_ok(x) for x in c)
            # the formulas, on these values
            f = [f2_of(x) for x in ps]
            t = add(f[4], sub(k2(sub(f[2], f[0]), 3), f[1]))
            assert f2_of(c[0]) == add(k2(f[2], 6), xi(sub(t, k2(f[3], 12))))
            assert f2_of(c[2]) == k2(sub(sub(add(f[0], f[1]), k2(f[2], 2)), k2(f[3], 2)), 3)
            assert f2_of(c[1]) == add(add(sub(k2(sub(f[0], f[1]), 3), t), k2(f[3], 12)), k2(xi(f[3]), 6))
            n += 1
    assert n == 2 * 4 ** 5 + 2 * 205


def test_scaled_sparse_product_bounds():
    """h6_mul_12<6>: x reduced (|.| < 2p), b1 and b2 a line product's coefficients (< 1.26p)"""
    ct = Contract()
    rng = random.Random(0x73706172)
    X, Bd = 2 * P, 5 * P // 4
    for sx in itertools.product((1, -1), repeat=6):
        low = rng.choice((0, 1))
        x = tuple((extreme(X, sx[2 * i], low), extreme(X, sx[2 * i + 1], low)) for i in range(3))
        sb = [rng.choice((1, -1)) for _ in range(4)]
        b1 = (extreme(Bd, sb[0], 1 - low), extreme(Bd, sb[1], low))
        b2 = (extreme(Bd, sb[2], low), extreme(Bd, sb[3], 1 - low))
        for S in (1, 6):
            c = h6_mul_12(x, b1, b2, S, ct)
            assert all(out_ok(v) for v in c)
            want = k6(C.f6_mul(f6_of(x), (C.F2_ZERO, f2_of(b1), f2_of(b2))), S * RINV)
            assert f6_of(c) == want
