// The square-root half of point decoding (pairing 0.14 G1Compressed / G2Compressed::into_affine):
// recover y from rhs = x^3 + b and pick the root the encoding's sign flag names.  One lane per
// point on hb::Fp; shared by the throughput decoders (k_wire.hip) and their latency form
// (k_wire_split.hip), so both write the same bytes.
#pragma once
#include "curve.hpp"
#include "wire.hpp"
#include "sqrt_chain.inc"

namespace hb {

// canonical words a > b
__device__ __forceinline__ bool words_gt(const uint32_t* a, const uint32_t* b, int n) {
  for (int i = n - 1; i >= 0; i--)
    if (a[i] != b[i]) return a[i] > b[i];
  return false;
}

// G1: y = the root of rhs named by the flags, as canonical words (p: the modulus as words); false
// (y untouched) when rhs is not a square
__device__ __forceinline__ bool g1_root_y(const Fp& rhs, uint8_t f, const uint32_t* p, uint32_t* y) {
  Fp ym = fp_mul(rhs, fp_pow_pm3d4(rhs));  // rhs^((p+1)/4)
  if (!fp_eq(fp_sqr(ym), rhs)) return false;
  // "greatest" = y > p - y, i.e. y > (p - 1) / 2
  fp_to_words(ym, y);
  uint32_t half[12];
  for (int k = 0; k < 12; k++) half[k] = (p[k] >> 1) | (k < 11 ? (p[k + 1] << 31) : 0u);
  const bool greatest = words_gt(y, half, 12);
  if (greatest != ((f & hbl::WIRE_GREATEST) != 0)) {
    ym = fp_neg(ym);
    fp_to_words(ym, y);
  }
  return true;
}

// pairing 0.14 Ord for Fq2: c1 first, then c0 (canonical integers)
__device__ __forceinline__ bool f2_gt_canon(const Fp2& a, const Fp2& b) {
  uint32_t a0[12], a1[12], b0[12], b1[12];
  fp_to_words(a.c0, a0);
  fp_to_words(a.c1, a1);
  fp_to_words(b.c0, b0);
  fp_to_words(b.c1, b1);
  bool eq1 = true;
  for (int k = 0; k < 12; k++) eq1 = eq1 && a1[k] == b1[k];
  return eq1 ? words_gt(a0, b0, 12) : words_gt(a1, b1, 12);
}

// Square root in Fp2 by the norm (two Fp exponentiations by (p-3)/4 instead of two Fp2 ones):
// a = a0 + a1 u is a square iff N = a0^2 + a1^2 is a square in Fp; with s = sqrt(N) and
// t = (a0 + s) / 2 (or (a0 - s) / 2 when that is 0), w = t^((p-3)/4):
//   t w^2 ==  1 (t a square):      y = t w + (a1 w / 2) u
//   t w^2 == -1 (-t a square; p = 3 mod 8 makes (-1)^((p-3)/4) = 1, so w serves -t too):
//                                  y = a1 w / 2 - (t w) u
// (t (a0 - s)/2 = -a1^2 / 4 is a non-square for a1 != 0, so exactly one case holds.)  Any root:
// the caller picks the sign.  false when a is not a square.
// The two chains apart (k_hash.hip rejects a sampled x after the first): f2_sqrt_norm_first decides
// whether a != 0 is a square and leaves s = sqrt(N); f2_sqrt_norm_second takes the root from s.
__device__ __forceinline__ bool f2_sqrt_norm_first(const Fp2& a, Fp& s) {
  const Fp nrm = fp_add(fp_sqr(a.c0), fp_sqr(a.c1));
  s = fp_mul(nrm, fp_pow_pm3d4(nrm));
  return fp_eq(fp_sqr(s), nrm);
}
__device__ __forceinline__ bool f2_sqrt_norm_second(const Fp2& a, const Fp& s, Fp2& out) {
  const Fp half = fp_const(INV2_M);
  Fp t = fp_mul(fp_add(a.c0, s), half);
  if (fp_is_zero(t)) t = fp_mul(fp_sub(a.c0, s), half);
  const Fp w = fp_pow_pm3d4(t);
  const Fp tw = fp_mul(t, w);
  const Fp aw = fp_mul(fp_mul(a.c1, half), w);
  const bool qr = fp_eq(fp_mul(tw, w), fp_one());
  const Fp2 y = qr ? Fp2{tw, aw} : Fp2{aw, fp_neg(tw)};
  out = y;
  return f2_is_zero(f2_sub(f2_sqr(y), a));
}
__device__ __forceinline__ bool f2_sqrt_norm(const Fp2& a, Fp2& out) {
  out = f2_zero();
  if (f2_is_zero(a)) return true;
  Fp s;
  if (!f2_sqrt_norm_first(a, s)) return false;
  return f2_sqrt_norm_second(a, s, out);
}

// G2: ym = the root of rhs named by the flags; false when rhs is not a square
__device__ __forceinline__ bool g2_root_y(const Fp2& rhs, uint8_t f, Fp2& ym) {
  if (!f2_sqrt_norm(rhs, ym)) return false;
  const Fp2 ny = f2_neg(ym);
  if (f2_gt_canon(ym, ny) != ((f & hbl::WIRE_GREATEST) != 0)) ym = ny;
  return true;
}

}  // namespace hb
