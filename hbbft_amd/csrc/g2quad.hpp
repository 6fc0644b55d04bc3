// The G2 group law on LANE PAIRS and LANE QUADS (namespace hbs): two lanes hold the c0 / c1
// components of every Fp2 coordinate (pfp.hpp), so each Fp2 product is one lane-pair product; two
// lane pairs (a quad) hold the same point and split each group operation's independent products
// between them, trading results with one DPP quad permute per limb: a doubling is 4 product rounds
// instead of 7 serial products, a mixed addition 6 instead of 11.  Formulas: dbl-2009-l,
// add-2007-bl, madd-2007-bl (curve.hpp), exceptional cases included.  Shared by the latency form of
// the G2 combine (k_interp_pair.hip) and of the G2 decoder (k_wire_split.hip).
#pragma once
#include "pfp.hpp"

namespace hbs {

constexpr int DPP_XQ = 0x4E;             // quad_perm [2,3,0,1]: the other lane pair, same component

HP_D bool hj_is_zero(const HJac& p) { return h_is_zero(p.z); }
HP_D HJac hj_zero() { return {h_one(), h_one(), h_zero()}; }
HP_D HJac hj_reduce(const HJac& p) { return {fp_reduce(p.x), fp_reduce(p.y), fp_reduce(p.z)}; }

// dbl-2009-l; inputs |.| < 2p, outputs reduced
HP_D HJac hj_dbl(const HJac& p) {
  const Fp A = h_sqr(p.x);
  const Fp B = h_sqr(p.y);
  const Fp C = h_sqr(B);
  const Fp D = fp_reduce(fp_lin(2, fp_sub(fp_sub(h_sqr(fp_add(p.x, B)), A), C), 0, C));
  const Fp E = fp_lin(3, A, 0, A);
  const Fp F = h_sqr(E);
  HJac r;
  r.x = fp_reduce(fp_sub(F, fp_add(D, D)));
  r.y = fp_reduce(fp_sub(h_mul(E, fp_sub(D, r.x)), fp_lin(8, C, 0, C)));
  const Fp yz = h_mul(p.y, p.z);
  r.z = fp_reduce(fp_add(yz, yz));
  return r;
}

// add-2007-bl (general), exceptional cases as curve.hpp jac_add; conditions are pair-uniform
HP_D HJac hj_add(const HJac& p, const HJac& q) {
  if (hj_is_zero(p)) return q;
  if (hj_is_zero(q)) return p;
  const Fp Z1Z1 = h_sqr(p.z);
  const Fp Z2Z2 = h_sqr(q.z);
  const Fp U1 = h_mul(p.x, Z2Z2);
  const Fp U2 = h_mul(q.x, Z1Z1);
  const Fp S1 = h_mul(h_mul(p.y, q.z), Z2Z2);
  const Fp S2 = h_mul(h_mul(q.y, p.z), Z1Z1);
  const Fp H = fp_reduce(fp_sub(U2, U1));
  const Fp rr = fp_reduce(fp_lin(2, S2, -2, S1));
  if (h_is_zero(H)) {
    if (h_is_zero(rr)) return hj_dbl(p);
    return hj_zero();
  }
  const Fp I = h_sqr(fp_add(H, H));
  const Fp J = h_mul(H, I);
  const Fp V = h_mul(U1, I);
  HJac r;
  r.x = fp_reduce(fp_sub(fp_sub(h_sqr(rr), J), fp_add(V, V)));
  const Fp SJ = h_mul(S1, J);
  r.y = fp_reduce(fp_sub(h_mul(rr, fp_sub(V, r.x)), fp_add(SJ, SJ)));
  r.z = fp_reduce(h_mul(fp_sub(fp_sub(h_sqr(fp_add(p.z, q.z)), Z1Z1), Z2Z2), H));
  return r;
}

// madd-2007-bl: p + (x2, y2), the affine point not infinity
HP_D HJac hj_add_affine(const HJac& p, const Fp& x2, const Fp& y2) {
  if (hj_is_zero(p)) return {x2, y2, h_one()};
  const Fp Z1Z1 = h_sqr(p.z);
  const Fp U2 = h_mul(x2, Z1Z1);
  const Fp S2 = h_mul(h_mul(y2, p.z), Z1Z1);
  const Fp H = fp_reduce(fp_sub(U2, p.x));
  const Fp rr = fp_reduce(fp_lin(2, S2, -2, p.y));
  if (h_is_zero(H)) {
    if (h_is_zero(rr)) return hj_dbl(p);
    return hj_zero();
  }
  const Fp HH = h_sqr(H);
  const Fp I = fp_lin(4, HH, 0, HH);
  const Fp J = h_mul(H, I);
  const Fp V = h_mul(p.x, I);
  HJac r;
  r.x = fp_reduce(fp_sub(fp_sub(h_sqr(rr), J), fp_add(V, V)));
  const Fp YJ = h_mul(p.y, J);
  r.y = fp_reduce(fp_sub(h_mul(rr, fp_sub(V, r.x)), fp_add(YJ, YJ)));
  r.z = fp_reduce(fp_sub(fp_sub(h_sqr(fp_add(p.z, H)), Z1Z1), HH));
  return r;
}

// ---------------------------------------------------------------- lane quads
// A quad's two lane pairs hold the same values; in a round pair 0 forms a0 * b0 and pair 1 a1 * b1
// (or squares), and both end with both products.  Conditions below are quad-uniform.
HP_D bool q_hi() { return (threadIdx.x & 2) != 0; }
HP_D void q_mul(const Fp& a0, const Fp& b0, const Fp& a1, const Fp& b1, Fp& r0, Fp& r1) {
  const bool q = q_hi();
  const Fp r = h_mul(fp_sel(q, a1, a0), fp_sel(q, b1, b0));
  const Fp o = dpp_fp<DPP_XQ>(r);
  r0 = fp_sel(q, o, r);
  r1 = fp_sel(q, r, o);
}
HP_D void q_sqr(const Fp& a0, const Fp& a1, Fp& r0, Fp& r1) {
  const bool q = q_hi();
  const Fp r = h_sqr(fp_sel(q, a1, a0));
  const Fp o = dpp_fp<DPP_XQ>(r);
  r0 = fp_sel(q, o, r);
  r1 = fp_sel(q, r, o);
}

// hj_dbl in 4 rounds
HP_D HJac qj_dbl(const HJac& p) {
  Fp A, B, C, F, XB2, YZ;
  q_sqr(p.x, p.y, A, B);
  const Fp E = fp_lin(3, A, 0, A);
  q_sqr(B, E, C, F);
  q_mul(fp_add(p.x, B), fp_add(p.x, B), p.y, p.z, XB2, YZ);
  const Fp D = fp_reduce(fp_lin(2, fp_sub(fp_sub(XB2, A), C), 0, C));
  HJac r;
  r.x = fp_reduce(fp_sub(F, fp_add(D, D)));
  r.y = fp_reduce(fp_sub(h_mul(E, fp_sub(D, r.x)), fp_lin(8, C, 0, C)));
  r.z = fp_reduce(fp_add(YZ, YZ));
  return r;
}

// hj_add_affine in 6 rounds (Z3 = 2 Z1 H, the same value as (Z1 + H)^2 - Z1Z1 - HH)
HP_D HJac qj_add_affine(const HJac& p, const Fp& x2, const Fp& y2) {
  if (hj_is_zero(p)) return {x2, y2, h_one()};
  Fp Z1Z1, YZ, U2, S2;
  q_mul(p.z, p.z, y2, p.z, Z1Z1, YZ);
  q_mul(x2, Z1Z1, YZ, Z1Z1, U2, S2);
  const Fp H = fp_reduce(fp_sub(U2, p.x));
  const Fp rr = fp_reduce(fp_lin(2, S2, -2, p.y));
  if (h_is_zero(H)) {
    if (h_is_zero(rr)) return qj_dbl(p);
    return hj_zero();
  }
  Fp HH, RR, J, V, EV, YJ;
  q_sqr(H, rr, HH, RR);
  const Fp I = fp_lin(4, HH, 0, HH);
  q_mul(H, I, p.x, I, J, V);
  HJac r;
  r.x = fp_reduce(fp_sub(fp_sub(RR, J), fp_add(V, V)));
  q_mul(rr, fp_sub(V, r.x), p.y, J, EV, YJ);
  r.y = fp_reduce(fp_sub(EV, fp_add(YJ, YJ)));
  const Fp ZH = h_mul(p.z, H);
  r.z = fp_reduce(fp_add(ZH, ZH));
  return r;
}

}  // namespace hbs
