// Lane-QUAD extension of the lane-pair tower (pfp.hpp), namespace hbs: FOUR lanes per pairing check
// for the mid-size batches (k_quad.hpp).
//
// A quad is two lane pairs (lanes 4i, 4i+1 = pair 0; 4i+2, 4i+3 = pair 1), each laid out as in
// pfp.hpp (even lane c0, odd lane c1).  Both pairs hold the whole check state (replicated); every
// operation whose Fp2 / Fp6 products are independent runs them side by side -- pair 0 the first,
// pair 1 the second -- and the results cross over with one DPP quad permutation per limb
// ([2,3,0,1], the same component of the other pair), after which both pairs hold both results
// again.  Every pfp.hpp DPP pattern is pair-local ([1,0,3,2], [0,0,2,2], [1,1,3,3]), so the
// lane-pair products run unchanged on both pairs at once.
//
// The split is made where the formulas are widest:
//   h6_mul2      two whole Fp6 products (one per pair): complex squaring's t and s, Karatsuba's t0
//                and t1 -- the sums and reductions inside are split too, not repeated;
//   h6_mul_q     one Fp6 product as three dual Fp2 rounds (Karatsuba's third product);
//   h_mul2 / h_sqr2 / fp_mul2   single dual products (line products, doubling step, cyclotomic
//                squaring's nine squares in five rounds, line evaluation at P); h_mul2 / h_sqr2 are
//                also the rounds of the lane-quad G2 group law (g2quad.hpp).
// A check's per-lane product count falls to ~0.55 of the lane pair's, so a batch of 16,384 checks
// (1,024 waves: one per SIMD) finishes in a little over half the lane-pair kernel's latency floor.
// Formulas and value contracts are pfp.hpp's (pairing 0.14's, restated in oracle/c/bls_cpu.c).
#pragma once
#include "pfp.hpp"

namespace hbs {

constexpr int DPP_QSWAP = 0x4E;  // quad_perm [2,3,0,1]: the other pair's lane with the same component

HP_D bool q_hi() { return (threadIdx.x & 2) != 0; }

HP_D Fp q_sel(bool hi, const Fp& a, const Fp& b) {  // hi ? b : a
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = hi ? b.l[i] : a.l[i];
  return r;
}
HP_D H6 q_sel6(bool hi, const H6& a, const H6& b) { return {q_sel(hi, a.c0, b.c0), q_sel(hi, a.c1, b.c1), q_sel(hi, a.c2, b.c2)}; }

// this pair computed `mine` (pair 0: value 0, pair 1: value 1); both pairs get (v0, v1)
HP_D void q_join(bool hi, const Fp& mine, Fp& v0, Fp& v1) {
  const Fp o = dpp_fp<DPP_QSWAP>(mine);
  v0 = q_sel(hi, mine, o);
  v1 = q_sel(hi, o, mine);
}
HP_D void q_join6(bool hi, const H6& mine, H6& v0, H6& v1) {
  q_join(hi, mine.c0, v0.c0, v1.c0);
  q_join(hi, mine.c1, v0.c1, v1.c1);
  q_join(hi, mine.c2, v0.c2, v1.c2);
}

// (x0 y0, x1 y1) in one product time (h_mul contracts per product)
HP_D void h_mul2(const Fp& x0, const Fp& y0, const Fp& x1, const Fp& y1, Fp& r0, Fp& r1) {
  const bool hi = q_hi();
  q_join(hi, h_mul(q_sel(hi, x0, x1), q_sel(hi, y0, y1)), r0, r1);
}
HP_D void h_sqr2(const Fp& a0, const Fp& a1, Fp& r0, Fp& r1) {
  const bool hi = q_hi();
  q_join(hi, h_sqr(q_sel(hi, a0, a1)), r0, r1);
}
HP_D void fp_mul2(const Fp& x0, const Fp& y0, const Fp& x1, const Fp& y1, Fp& r0, Fp& r1) {
  const bool hi = q_hi();
  q_join(hi, fp_mul(q_sel(hi, x0, x1), q_sel(hi, y0, y1)), r0, r1);
}
// (a0 b0, a1 b1) over Fp6: pair k runs pfp.hpp's h6_mul on its operands
HP_D void h6_mul2(const H6& a0, const H6& b0, const H6& a1, const H6& b1, H6& r0, H6& r1) {
  const bool hi = q_hi();
  q_join6(hi, h6_mul(q_sel6(hi, a0, a1), q_sel6(hi, b0, b1)), r0, r1);
}

// one Fp6 Karatsuba product (h6_mul) as three dual rounds: (v1, v2), (t12, v0), (t01, t02)
HP_D H6 h6_mul_q(const H6& a, const H6& b) {
  Fp v1, v2, t12, v0, t01, t02;
  h_mul2(a.c1, b.c1, a.c2, b.c2, v1, v2);
  h_mul2(fp_addl(a.c1, a.c2), fp_add(b.c1, b.c2), a.c0, b.c0, t12, v0);
  const Fp c0 = fp_red_l(h_add_xi_l(v0, fp_sub2l(t12, v1, v2)));
  h_mul2(fp_addl(a.c0, a.c1), fp_add(b.c0, b.c1), fp_addl(a.c0, a.c2), fp_add(b.c0, b.c2), t01, t02);
  const Fp c1 = fp_red_l(h_add_xi_l(fp_sub2l(t01, v0, v1), v2));
  const Fp c2 = fp_red_l(fp_addl(fp_sub2l(t02, v0, v2), v1));
  return {c0, c1, c2};
}

// the product (C0, (0, c11, c12)) of two sparse lines from its six Fp2 products (h12_mul_lines),
// each coefficient reduced in one carry pass
HP_D void h_line_comb(const Fp& a0b0, const Fp& a1b1, const Fp& a4b4, const Fp& t04, const Fp& t14, const Fp& t01,
                      H6& C0, Fp& c11, Fp& c12) {
  c11 = fp_red_l(fp_sub2l(t04, a0b0, a4b4));
  c12 = fp_red_l(fp_sub2l(t14, a1b1, a4b4));
  C0 = {fp_red_l(h_add_xi_l(a0b0, a4b4)), fp_red_l(fp_sub2l(t01, a0b0, a1b1)), a1b1};
}

// Granger-Scott squaring (h12_cyclo_sqr): nine Fp2 squares in five rounds
HP_D H12 h12_cyclo_sqr_q(const H12& f) {
  const Fp& a0 = f.c0.c0; const Fp& a2 = f.c0.c1; const Fp& a4 = f.c0.c2;
  const Fp& a1 = f.c1.c0; const Fp& a3 = f.c1.c1; const Fp& a5 = f.c1.c2;
  Fp s0, s3, s03, s1, s4, s14, s2, s5;
  h_sqr2(a0, a3, s0, s3);
  h_sqr2(fp_add(a0, a3), a1, s03, s1);
  h_sqr2(a4, fp_add(a1, a4), s4, s14);
  h_sqr2(a2, a5, s2, s5);
  const Fp s25 = h_sqr(fp_add(a2, a5));
  H12 r;
  r.c0.c0 = fp_red_mk<3, -2>(h_add_xi_l(s0, s3), a0);
  r.c1.c1 = fp_red_mk<3, 2>(fp_sub2l(s03, s0, s3), a3);
  r.c0.c1 = fp_red_mk<3, -2>(h_add_xi_l(s1, s4), a2);
  r.c1.c2 = fp_red_mk<3, 2>(fp_sub2l(s14, s1, s4), a5);
  r.c0.c2 = fp_red_mk<3, -2>(h_add_xi_l(s2, s5), a4);
  r.c1.c0 = fp_red_mk<3, 2>(h_add_xi_l(fp_zero(), fp_sub2l(s25, s2, s5)), a1);
  return r;
}

HP_D H12 h12_frob1_q(const H12& f) {
  H12 r;
  r.c0.c0 = h_conj(f.c0.c0);
  h_mul2(h_conj(f.c1.c0), HP_FROB1(1), h_conj(f.c0.c1), HP_FROB1(2), r.c1.c0, r.c0.c1);
  h_mul2(h_conj(f.c1.c1), HP_FROB1(3), h_conj(f.c0.c2), HP_FROB1(4), r.c1.c1, r.c0.c2);
  r.c1.c2 = h_mul(h_conj(f.c1.c2), HP_FROB1(5));
  return h12_red(r);
}
HP_D H12 h12_frob2_q(const H12& f) {
  H12 r;
  r.c0.c0 = f.c0.c0;
  fp_mul2(f.c1.c0, fp_const(hb::FROB2_1_C0), f.c0.c1, fp_const(hb::FROB2_2_C0), r.c1.c0, r.c0.c1);
  fp_mul2(f.c1.c1, fp_const(hb::FROB2_3_C0), f.c0.c2, fp_const(hb::FROB2_4_C0), r.c1.c1, r.c0.c2);
  r.c1.c2 = fp_mul(f.c1.c2, fp_const(hb::FROB2_5_C0));
  return r;
}

// doubling step, T in Jacobian coordinates; lines scaled as pairing 0.14 scales them (the Fp2 factors
// die in the final exponentiation): eleven products in six rounds
HP_D HLine h_dbl_step_q(HJac& T) {
  Fp A, B, C, ZZ, XB, YZ, EX, EZ, C4, F;
  h_sqr2(T.x, T.y, A, B);
  h_sqr2(B, T.z, C, ZZ);
  h_sqr2(fp_add(T.x, B), fp_add(T.y, T.z), XB, YZ);
  const Fp D = fp_lin(2, fp_sub(fp_sub(XB, A), C), 0, C);
  const Fp E = fp_lin(3, A, 0, A);
  h_mul2(E, T.x, E, ZZ, EX, EZ);
  HLine l;
  l.c0 = fp_sub(EX, fp_add(B, B));
  l.c1 = fp_neg(EZ);
  const Fp Z3 = fp_sub(fp_sub(YZ, B), ZZ);
  h_mul2(Z3, ZZ, E, E, C4, F);
  l.c4 = C4;
  const Fp X3 = fp_sub(F, fp_add(D, D));
  T.y = fp_sub(h_mul(E, fp_sub(D, X3)), fp_lin(8, C, 0, C));
  T.x = X3;
  T.z = Z3;
  l.c0 = fp_reduce(l.c0);
  T.x = fp_reduce(T.x);
  T.y = fp_reduce(T.y);
  T.z = fp_reduce(T.z);
  return l;
}

// addition step (mixed, Q affine): thirteen products in seven rounds
HP_D HLine h_add_step_q(HJac& T, const Fp& xQ, const Fp& yQ) {
  Fp YZ, U2, S2, Z3, HH, R2, HHH, V, RV, YH, RX, YZ3;
  const Fp Z1Z1 = h_sqr(T.z);
  h_mul2(yQ, T.z, xQ, Z1Z1, YZ, U2);
  const Fp H = fp_sub(U2, T.x);
  h_mul2(YZ, Z1Z1, T.z, H, S2, Z3);
  const Fp r = fp_sub(S2, T.y);
  h_sqr2(H, r, HH, R2);
  h_mul2(H, HH, T.x, HH, HHH, V);
  const Fp X3 = fp_sub(fp_sub(R2, HHH), fp_add(V, V));
  h_mul2(r, fp_sub(V, X3), T.y, HHH, RV, YH);
  h_mul2(r, xQ, yQ, Z3, RX, YZ3);
  HLine l;
  l.c0 = fp_reduce(fp_sub(RX, YZ3));
  l.c1 = fp_neg(r);
  l.c4 = Z3;
  T.x = fp_reduce(X3);
  T.y = fp_reduce(fp_sub(RV, YH));
  T.z = Z3;
  return l;
}

// ---------------------------------------------------------------- the lane quad as a width policy
// (pfp.hpp LanePair): two products side by side.  In the shared Fp12 operations that is t and s of
// the complex squaring, Karatsuba's t0 and t1 (for the two-line product t1 = f1 (0, c11, c12) is an
// h6_mul with a zero coefficient: the product with it is the one wasted of the 17) and the six line
// products in three rounds.
struct LaneQuad {
  static constexpr int LANES = 4;
  static HP_D bool leader() { return (threadIdx.x & 3) == 0; }
  static HP_D bool value_writer() { return !q_hi(); }  // pair 0
  using Walk = HJac;
  template <bool W1, bool W2, int GEN>
  using Park = NoPark;  // T and P stay in registers
  static HP_D HLine dbl_step(HJac& T) { return h_dbl_step_q(T); }
  static HP_D HLine add_step(HJac& T, const Fp& xQ, const Fp& yQ) { return h_add_step_q(T, xQ, yQ); }

  template <bool W1, bool W2>
  static constexpr bool first_line() { return false; }
  static HP_D H6 mul6(const H6& a, const H6& b) { return h6_mul_q(a, b); }
  template <class A1, class B1>
  static HP_D void mul6x2(const H6& a0, const H6& b0, const A1& a1, const B1& b1, H6& r0, H6& r1) {
    h6_mul2(a0, b0, h6_of(a1), h6_of(b1), r0, r1);
  }
  static HP_D void mul6x2_12(const H6& a0, const H6& b0, const H6& a1, const Fp& c1, const Fp& c2, H6& r0, H6& r1) {
    h6_mul2(a0, b0, a1, {h_zero(), c1, c2}, r0, r1);
  }
  static constexpr int MILLER_SCALE = 1;  // the Miller loop takes the exact Karatsuba products too
  static HP_D H6 miller_mul6(const H6& a, const H6& b) { return mul6(a, b); }
  template <class A1, class B1>
  static HP_D void miller_mul6x2(const H6& a0, const H6& b0, const A1& a1, const B1& b1, H6& r0, H6& r1) {
    mul6x2(a0, b0, a1, b1, r0, r1);
  }
  static HP_D void miller_mul6x2_12(const H6& a0, const H6& b0, const H6& a1, const Fp& c1, const Fp& c2, H6& r0,
                                    H6& r1) {
    mul6x2_12(a0, b0, a1, c1, c2, r0, r1);
  }
  static HP_D void line_product(const Fp& a0, const Fp& a1, const Fp& a4, const Fp& b0, const Fp& b1, const Fp& b4,
                                H6& C0, Fp& c11, Fp& c12) {
    Fp a0b0, a1b1, a4b4, t04, t14, t01;
    h_mul2(a0, b0, a1, b1, a0b0, a1b1);
    h_mul2(a4, b4, fp_addl(a0, a4), fp_add(b0, b4), a4b4, t04);
    h_mul2(fp_addl(a1, a4), fp_add(b1, b4), fp_addl(a0, a1), fp_add(b0, b1), t14, t01);
    h_line_comb(a0b0, a1b1, a4b4, t04, t14, t01, C0, c11, c12);
  }
  static HP_D H12 cyclo_sqr(const H12& f) { return h12_cyclo_sqr_q(f); }
  static HP_D H12 frob1(const H12& f) { return h12_frob1_q(f); }
  static HP_D H12 frob2(const H12& f) { return h12_frob2_q(f); }

  // LanePair::line_at_p with the two products side by side
  template <bool GEN, class ST>
  static HP_D HLine line_at_p(const HLine& l, const ST& st, bool negate) {
    HLine e;
    e.c0 = st.act ? l.c0 : h_one();
    Fp c1, c4;
    fp_mul2(l.c1, side_xP<GEN>(st), l.c4, side_yP<GEN>(st, negate), c1, c4);
    e.c1 = st.act ? c1 : fp_zero();
    e.c4 = st.act ? c4 : fp_zero();
    return e;
  }
  template <bool G1, bool G2, bool WALK_FIRST, class RA, class RB, class ST>
  static HP_D void lines_at_p(const RA& raw_a, const RB& raw_b, const ST& A, const ST& B, bool neg2, HLine& la,
                              HLine& lb, const NoPark&) {
    la = line_at_p<G1>(raw_a(), A, false);
    lb = line_at_p<G2>(raw_b(), B, neg2);
  }
};

}  // namespace hbs
