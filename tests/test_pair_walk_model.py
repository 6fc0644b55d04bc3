"""The lane-pair kernel's homogeneous G2 walk (csrc/pfp.hpp h_dbl_step_h / h_add_step_h) against
the Jacobian walk it replaces (csrc/qfp.hpp h_dbl_step_q / csrc/ofp.hpp h_dbl_step_o and their
addition steps, which the other widths keep), over the oracle's Fp2 arithmetic.

Both formula sets are restated here exactly as pfp.hpp and qfp.hpp state them.  All 68 steps of |x| are
walked with both; at every step the two running points must be the same affine point and the two
lines (c0, c1, c4) must differ by one nonzero Fp2 factor (which the final exponentiation removes).
"""
import random

import pytest

from oracle import bls12_381 as C

add, sub, mul, sqr, neg = C.f2_add, C.f2_sub, C.f2_mul, C.f2_sqr, C.f2_neg
xi = C.f2_mul_xi


def k(a, n):
    return C.f2_muls(a, n % C.P)


# ---------------------------------------------------------------- Jacobian (h_dbl_step_q / h_add_step_q)
def jac_dbl(T):
    X, Y, Z = T
    A = sqr(X)
    B = sqr(Y)
    Cc = sqr(B)
    D = k(sub(sub(sqr(add(X, B)), A), Cc), 2)
    E = k(A, 3)
    ZZ = sqr(Z)
    c0 = sub(mul(E, X), add(B, B))
    c1 = neg(mul(E, ZZ))
    Z3 = sub(sub(sqr(add(Y, Z)), B), ZZ)
    c4 = mul(Z3, ZZ)
    F = sqr(E)
    X3 = sub(F, add(D, D))
    Y3 = sub(mul(E, sub(D, X3)), k(Cc, 8))
    return (X3, Y3, Z3), (c0, c1, c4)


def jac_add(T, Q):
    X, Y, Z = T
    xQ, yQ = Q
    Z1Z1 = sqr(Z)
    U2 = mul(xQ, Z1Z1)
    S2 = mul(mul(yQ, Z), Z1Z1)
    H = sub(U2, X)
    r = sub(S2, Y)
    HH = sqr(H)
    HHH = mul(H, HH)
    V = mul(X, HH)
    X3 = sub(sub(sqr(r), HHH), add(V, V))
    Y3 = sub(mul(r, sub(V, X3)), mul(Y, HHH))
    Z3 = mul(Z, H)
    return (X3, Y3, Z3), (sub(mul(r, xQ), mul(yQ, Z3)), neg(r), Z3)


def jac_affine(T):
    X, Y, Z = T
    zi = C.f2_inv(Z)
    zi2 = sqr(zi)
    return mul(X, zi2), mul(Y, mul(zi2, zi))


# ---------------------------------------------------------------- homogeneous (h_dbl_step_h / h_add_step_h)
def hom_dbl(T):
    X, Y, Z = T
    A = mul(X, Y)
    B = sqr(Y)
    Cc = sqr(Z)
    E = k(xi(Cc), 12)  # 3 b' Z^2, b' = 4 xi
    H = sub(sub(sqr(add(Y, Z)), B), Cc)
    S = sqr(X)
    line = (sub(B, E), k(S, -3), H)
    Bm = sub(B, k(E, 3))
    Bp = add(B, k(E, 3))
    X3 = mul(add(A, A), Bm)
    Y3 = sub(sqr(Bp), k(sqr(E), 12))
    Z3 = k(mul(add(B, B), H), 2)
    return (X3, Y3, Z3), line


def hom_add(T, Q):
    X, Y, Z = T
    xQ, yQ = Q
    th = sub(Y, mul(yQ, Z))
    la = sub(X, mul(xQ, Z))
    line = (sub(mul(th, xQ), mul(la, yQ)), neg(th), la)
    Cc = sqr(th)
    D = sqr(la)
    E = mul(la, D)
    F = mul(Z, Cc)
    G = mul(X, D)
    H = sub(add(E, F), add(G, G))
    X3 = mul(la, H)
    Y3 = sub(mul(th, sub(G, H)), mul(E, Y))
    Z3 = mul(Z, E)
    return (X3, Y3, Z3), line


def hom_affine(T):
    X, Y, Z = T
    zi = C.f2_inv(Z)
    return mul(X, zi), mul(Y, zi)


def proportional(lj, lh):
    """lh = s * lj for one nonzero Fp2 s (cross products vanish; no line is all zero)"""
    assert not all(C.f2_is_zero(c) for c in lj)
    assert not all(C.f2_is_zero(c) for c in lh)
    for i in range(3):
        for j in range(i + 1, 3):
            if mul(lj[i], lh[j]) != mul(lj[j], lh[i]):
                return False
    return True


def _points():
    rng = random.Random(0x68626274)
    pts = [C.G2_GEN]
    for _ in range(3):
        pts.append(C.g2_mul(C.G2_GEN, rng.randrange(1, C.R)))
    return pts


@pytest.mark.parametrize("idx", range(4))
def test_homogeneous_walk_matches_jacobian(idx):
    Q = _points()[idx]
    assert C.g2_on_curve(Q)
    TJ = (Q[0], Q[1], C.F2_ONE)
    TH = (Q[0], Q[1], C.F2_ONE)
    steps = 0
    mult = 1
    for b in range(62, -1, -1):
        TJ, lj = jac_dbl(TJ)
        TH, lh = hom_dbl(TH)
        mult *= 2
        steps += 1
        assert not C.f2_is_zero(TH[2]) and not C.f2_is_zero(TJ[2]), (idx, b, "dbl")
        assert hom_affine(TH) == jac_affine(TJ), (idx, b, "dbl")
        assert proportional(lj, lh), (idx, b, "dbl")
        if (C.X_ABS >> b) & 1:
            TJ, lj = jac_add(TJ, Q)
            TH, lh = hom_add(TH, Q)
            mult += 1
            steps += 1
            assert not C.f2_is_zero(TH[2]) and not C.f2_is_zero(TJ[2]), (idx, b, "add")
            assert hom_affine(TH) == jac_affine(TJ), (idx, b, "add")
            assert proportional(lj, lh), (idx, b, "add")
    assert steps == 68
    assert mult == C.X_ABS
    # the walk ends on [|x|] Q
    assert hom_affine(TH) == C.g2_mul(Q, C.X_ABS)
