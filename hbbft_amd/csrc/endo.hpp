// The curve endomorphisms and scalar splits shared by the curve kernels (k_curve.hip: interpolate();
// k_rlc.hip: the grouped random-combination sums), with the ABI point loads both use.
#pragma once
#include "curve.hpp"

namespace hb {

HB_HD void load_g1(const uint32_t* w, Fp& x, Fp& y, bool& inf) {
  G1Aff a = g1_from_words(w);
  x = a.x;
  y = a.y;
  inf = a.inf;
}
HB_HD void load_g2(const uint32_t* w, Fp2& x, Fp2& y, bool& inf) {
  G2Aff a = g2_from_words(w);
  x = a.x;
  y = a.y;
  inf = a.inf;
}

// Endomorphism split of a canonical scalar k < r (r < |x|^4, x the BLS parameter):
//   G2: k = d0 + d1|x| + d2|x|^2 + d3|x|^3 (digits < |x| < 2^64); psi = [x] on G2, so
//       |x|^j P = (-1)^j psi^j(P) and k P = sum_j d_j (-1)^j psi^j(P).
//   G1: k = d0 + d1 x^2 (digits < x^2 < 2^128); phi(x, y) = (beta x, y) = [-x^2] on G1, so
//       x^2 P = (beta x, -y) and k P = d0 P + d1 (beta x, -y).
// Digits by bit-serial long division (wave-uniform loops, no 128-bit types on the device).
// Valid for points of the prime-order subgroups, which the ABI requires of every sample.
HB_HD void k_to_u64(const uint32_t* k, uint64_t q[4]) {
  for (int w = 0; w < 4; w++) q[w] = (uint64_t)k[2 * w] | ((uint64_t)k[2 * w + 1] << 32);
}

// q <- q / D, returns q mod D; D = X_ABS (top bit set, so a shifted-out bit always means >= D)
HB_HD uint64_t div_x_abs(uint64_t q[4]) {
  uint64_t rem = 0;
  for (int w = 3; w >= 0; w--) {
    uint64_t qw = 0;
    for (int b = 63; b >= 0; b--) {
      const bool top = (rem >> 63) != 0;
      rem = (rem << 1) | ((q[w] >> b) & 1);
      const bool ge = top || rem >= X_ABS;
      if (ge) rem -= X_ABS;
      qw |= (uint64_t)ge << b;
    }
    q[w] = qw;
  }
  return rem;
}

// q <- q / x^2, rem <- q mod x^2 (128-bit divisor with its top bit set)
HB_HD void div_x2(uint64_t q[4], uint64_t rem[2]) {
  uint64_t r0 = 0, r1 = 0;
  for (int w = 3; w >= 0; w--) {
    uint64_t qw = 0;
    for (int b = 63; b >= 0; b--) {
      const bool top = (r1 >> 63) != 0;
      r1 = (r1 << 1) | (r0 >> 63);
      r0 = (r0 << 1) | ((q[w] >> b) & 1);
      const bool ge = top || r1 > X2_ABS[1] || (r1 == X2_ABS[1] && r0 >= X2_ABS[0]);
      if (ge) {
        const uint64_t nr0 = r0 - X2_ABS[0];
        r1 = r1 - X2_ABS[1] - (r0 < X2_ABS[0] ? 1 : 0);
        r0 = nr0;
      }
      qw |= (uint64_t)ge << b;
    }
    q[w] = qw;
  }
  rem[0] = r0;
  rem[1] = r1;
}

HB_HD Fp2 psi_x(const Fp2& x) {  // conj(x) * (0 + c u) = (x1 c) + (x0 c) u
  const Fp c = fp_const(PSI_C1_C1);
  return {fp_mul(x.c1, c), fp_mul(x.c0, c)};
}
HB_HD Fp2 psi_y(const Fp2& y) {
  const Fp2 c2 = {fp_const(PSI_C2_C0), fp_const(PSI_C2_C1)};
  return f2_mul(f2_conj(y), c2);
}

}  // namespace hb
