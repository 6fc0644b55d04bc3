// Fp2 = Fp[u]/(u^2+1) for BLS12-381 on gfx950, both components on one lane (unsigned limbs of
// fp.hpp): the coordinate field of G2 in curve.hpp, the square root of wire_root.hpp and the
// hash to G2 (k_hash.hip).  The rest of pairing 0.14's tower (Fp6 = Fp2[v]/(v^3-xi) with xi = 1+u,
// Fp12 = Fp6[w]/(w^2-v)) exists only lane-split, in pfp.hpp, and as the wave kernels' programs.
#pragma once
#include "fp.hpp"

namespace hb {

struct Fp2 { Fp c0, c1; };

// ------------------------------------------------------------------ Fp2
HB_HD Fp2 f2_zero() { return {fp_zero(), fp_zero()}; }
HB_HD Fp2 f2_one() { return {fp_one(), fp_zero()}; }
HB_HD Fp2 f2_add(const Fp2& a, const Fp2& b) { return {fp_add(a.c0, b.c0), fp_add(a.c1, b.c1)}; }
HB_HD Fp2 f2_sub(const Fp2& a, const Fp2& b) { return {fp_sub(a.c0, b.c0), fp_sub(a.c1, b.c1)}; }
HB_HD Fp2 f2_dbl(const Fp2& a) { return {fp_dbl(a.c0), fp_dbl(a.c1)}; }
HB_HD Fp2 f2_neg(const Fp2& a) { return {fp_neg(a.c0), fp_neg(a.c1)}; }
HB_HD Fp2 f2_conj(const Fp2& a) { return {a.c0, fp_neg(a.c1)}; }

HB_HD Fp2 f2_mul(const Fp2& a, const Fp2& b) {
  Fp t0 = fp_mul(a.c0, b.c0);
  Fp t1 = fp_mul(a.c1, b.c1);
  Fp t2 = fp_mul(fp_add_nr(a.c0, a.c1), fp_add_nr(b.c0, b.c1));
  return {fp_sub(t0, t1), fp_sub(fp_sub(t2, t0), t1)};
}

HB_HD Fp2 f2_sqr(const Fp2& a) {
  // (a0 + a1)(a0 - a1) + 2 a0 a1 u
  Fp s = fp_add_nr(a.c0, a.c1);
  Fp d = fp_sub(a.c0, a.c1);
  Fp m = fp_mul(a.c0, a.c1);
  return {fp_mul(s, d), fp_dbl(m)};
}

HB_HD Fp2 f2_inv(const Fp2& a) {
  Fp t = fp_inv(fp_add(fp_sqr(a.c0), fp_sqr(a.c1)));
  return {fp_mul(a.c0, t), fp_neg(fp_mul(a.c1, t))};
}

HB_HD bool f2_is_zero(const Fp2& a) { return fp_is_zero(a.c0) && fp_is_zero(a.c1); }

}  // namespace hb
