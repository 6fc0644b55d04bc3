// The G2 group law on LANE QUADS (namespace hbs): two lanes hold the c0 / c1 components of every
// Fp2 coordinate (pfp.hpp), so each Fp2 product is one lane-pair product; two lane pairs (a quad)
// hold the same point and split each group operation's independent products between them, two per
// round (qfp.hpp h_mul2 / h_sqr2: one DPP quad permute per limb trades the results): a doubling is
// 4 product rounds instead of 7 serial products, a mixed addition 6 instead of 11, a general
// addition 9 instead of 16.  Formulas: dbl-2009-l, madd-2007-bl, add-2007-bl (curve.hpp),
// exceptional cases included; every condition is quad-uniform.  Shared by the latency form of the
// G2 combine (k_interp_pair.hip) and of the G2 decoder (k_wire_split.hip).
#pragma once
#include "qfp.hpp"

namespace hbs {

HP_D bool hj_is_zero(const HJac& p) { return h_is_zero(p.z); }
HP_D HJac hj_zero() { return {h_one(), h_one(), h_zero()}; }

// dbl-2009-l in 4 rounds; inputs |.| < 2p, outputs reduced:
//   A = X^2, B = Y^2, C = B^2, D = 2 ((X + B)^2 - A - C), E = 3 A, F = E^2
//   X3 = F - 2 D, Y3 = E (D - X3) - 8 C, Z3 = 2 Y Z
HP_D HJac qj_dbl(const HJac& p) {
  Fp A, B, C, F, XB2, YZ;
  h_sqr2(p.x, p.y, A, B);
  const Fp E = fp_lin(3, A, 0, A);
  h_sqr2(B, E, C, F);
  h_mul2(fp_add(p.x, B), fp_add(p.x, B), p.y, p.z, XB2, YZ);
  const Fp D = fp_reduce(fp_lin(2, fp_sub(fp_sub(XB2, A), C), 0, C));
  HJac r;
  r.x = fp_reduce(fp_sub(F, fp_add(D, D)));
  r.y = fp_reduce(fp_sub(h_mul(E, fp_sub(D, r.x)), fp_lin(8, C, 0, C)));
  r.z = fp_reduce(fp_add(YZ, YZ));
  return r;
}

// madd-2007-bl in 6 rounds: p + (x2, y2), the affine point not infinity:
//   U2 = x2 Z1^2, S2 = y2 Z1^3, H = U2 - X1, r = 2 (S2 - Y1), I = 4 H^2, J = H I, V = X1 I
//   X3 = r^2 - J - 2 V, Y3 = r (V - X3) - 2 Y1 J, Z3 = 2 Z1 H (the same value as (Z1 + H)^2 - Z1^2 - H^2)
HP_D HJac qj_add_affine(const HJac& p, const Fp& x2, const Fp& y2) {
  if (hj_is_zero(p)) return {x2, y2, h_one()};
  Fp Z1Z1, YZ, U2, S2;
  h_mul2(p.z, p.z, y2, p.z, Z1Z1, YZ);
  h_mul2(x2, Z1Z1, YZ, Z1Z1, U2, S2);
  const Fp H = fp_reduce(fp_sub(U2, p.x));
  const Fp rr = fp_reduce(fp_lin(2, S2, -2, p.y));
  if (h_is_zero(H)) {
    if (h_is_zero(rr)) return qj_dbl(p);
    return hj_zero();
  }
  Fp HH, RR, J, V, EV, YJ;
  h_sqr2(H, rr, HH, RR);
  const Fp I = fp_lin(4, HH, 0, HH);
  h_mul2(H, I, p.x, I, J, V);
  HJac r;
  r.x = fp_reduce(fp_sub(fp_sub(RR, J), fp_add(V, V)));
  h_mul2(rr, fp_sub(V, r.x), p.y, J, EV, YJ);
  r.y = fp_reduce(fp_sub(EV, fp_add(YJ, YJ)));
  const Fp ZH = h_mul(p.z, H);
  r.z = fp_reduce(fp_add(ZH, ZH));
  return r;
}

// add-2007-bl (general) in 9 rounds, exceptional cases as curve.hpp jac_add:
//   U1 = X1 Z2^2, U2 = X2 Z1^2, S1 = Y1 Z2^3, S2 = Y2 Z1^3, H = U2 - U1, r = 2 (S2 - S1)
//   I = (2 H)^2, J = H I, V = U1 I, X3 = r^2 - J - 2 V, Y3 = r (V - X3) - 2 S1 J, Z3 = 2 Z1 Z2 H
HP_D HJac qj_add(const HJac& p, const HJac& q) {
  if (hj_is_zero(p)) return q;
  if (hj_is_zero(q)) return p;
  Fp Z1Z1, Z2Z2, U1, U2, YZ1, YZ2, S1, S2;
  h_sqr2(p.z, q.z, Z1Z1, Z2Z2);
  h_mul2(p.x, Z2Z2, q.x, Z1Z1, U1, U2);
  h_mul2(p.y, q.z, q.y, p.z, YZ1, YZ2);
  h_mul2(YZ1, Z2Z2, YZ2, Z1Z1, S1, S2);
  const Fp H = fp_reduce(fp_sub(U2, U1));
  const Fp rr = fp_reduce(fp_lin(2, S2, -2, S1));
  if (h_is_zero(H)) {
    if (h_is_zero(rr)) return qj_dbl(p);
    return hj_zero();
  }
  Fp I, RR, J, V, EV, SJ, Z12, ZH;
  h_sqr2(fp_add(H, H), rr, I, RR);
  h_mul2(H, I, U1, I, J, V);
  HJac r;
  r.x = fp_reduce(fp_sub(fp_sub(RR, J), fp_add(V, V)));
  h_mul2(rr, fp_sub(V, r.x), S1, J, EV, SJ);
  r.y = fp_reduce(fp_sub(EV, fp_add(SJ, SJ)));
  Z12 = h_mul(p.z, q.z);
  ZH = h_mul(Z12, H);
  r.z = fp_reduce(fp_add(ZH, ZH));
  return r;
}

}  // namespace hbs
