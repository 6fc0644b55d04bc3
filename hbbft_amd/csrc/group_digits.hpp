// The digit forms of a grouped call's scalars (hbh_engine_set_group_scalar_form, k_rlc_digits.hip): how the
// 16 bytes of an item's scalar are read as short digits in the endomorphism basis, and the recoding that
// turns two digits into ONE joint double-and-add chain whose every table entry is a free affine point.
// Plain integer code, no HIP types: the kernel and a CPU checker (tests/csrc/group_digits_check.cpp,
// compiled with g++) share it.
//
// lambda = |x|^2 acts on both groups as a map that costs one Fp product: lambda (X, Y) = (k X, -Y) with
// k a primitive cube root of unity (G1: beta; G2: psi^2, k = beta^2).  lambda^2 - lambda + 1 = 0 mod r,
// so  B - lambda B = -lambda^2 B = (k^2 X, -Y)  is affine and free too.
//
//   X4 (a call with a G2 sum): four LE u32 digits, r = a0 + a1 |x| + a2 |x|^2 + a3 |x|^3 as an integer
//       (at most (2^32 - 1)(1 + |x| + |x|^2 + |x|^3) < 2^224 < r).
//       G2: chain t in {0, 1} is (u, v) = (a_t, a_{t+2}) on the base B_t = |x|^t Q = (-psi)^t (Q), 32 steps.
//       G1: one chain (u, v) = (a0 + a1 |x|, a2 + a3 |x|) on P, both < 2^96, 96 steps.
//   X2 (a call whose sums are both in G1): two LE u64 digits, r = b0 + b1 |x|^2 (at most
//       (2^64 - 1)(1 + |x|^2) < 2^192 < r); one chain (u, v) = (b0, b1) on P, 64 steps.
//
// A chain computes u B + v lambda B in K steps (K = 32, 64 or 96 >= the bit length of u and v).  For
// v != 0 write v = 2^K - w with w = 2^K - v in [1, 2^K): the term 2^K lambda B is the chain's START value
// (K doublings follow), and step i adds bit_i(u) B - bit_i(w) lambda B, one of
//     entry 1: +B = (X, Y)      entry 2: -lambda B = (k X, Y)      entry 3: B - lambda B = (k^2 X, -Y)
// (entry 0: nothing).  For v = 0 the chain starts from O and w = 0.  So a step is one doubling and at
// most one mixed addition, and no table entry needs an inversion or a Jacobian addition.
#pragma once
#include <stdint.h>

#include "constants.hpp"

#ifndef HB_HD
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define HB_HD __host__ __device__ __forceinline__
#else
#define HB_HD inline
#endif
#endif

namespace gd {

constexpr int FORM_INT128 = 0, FORM_X4 = 1, FORM_X2 = 2;  // == HBH_GFORM_*
constexpr int WORDS = 3;                                  // a chain's digits: at most 96 bits

struct Chain {
  uint32_t pos[WORDS];  // u, the digit of B (added)
  uint32_t neg[WORDS];  // w = 2^K - v mod 2^K, the recoded digit of lambda B (subtracted)
  uint32_t lead;        // v != 0: the chain starts from lambda B instead of O
};

HB_HD constexpr int steps_g2() { return 32; }
HB_HD constexpr int steps_g1(int form) { return form == FORM_X4 ? 96 : 64; }

// a + b |x| < 2^96 as three LE words
HB_HD void mul_add_x(uint32_t a, uint32_t b, uint32_t out[WORDS]) {
  const uint64_t xl = hb::X_ABS & 0xffffffffull, xh = hb::X_ABS >> 32;
  const uint64_t t0 = (uint64_t)b * xl + a;           // <= (2^32 - 1)^2 + 2^32 - 1 < 2^64
  const uint64_t t1 = (uint64_t)b * xh + (t0 >> 32);  // the same bound
  out[0] = (uint32_t)t0;
  out[1] = (uint32_t)t1;
  out[2] = (uint32_t)(t1 >> 32);
}

// The chain of the digits (u, v), `nw` words each (the words above are zero): neg = -v mod 2^(32 nw)
HB_HD Chain recode(const uint32_t u[WORDS], const uint32_t v[WORDS], int nw) {
  Chain c;
  uint32_t any = 0, borrow = 0;
  for (int j = 0; j < WORDS; j++) {
    c.pos[j] = j < nw ? u[j] : 0;
    const uint32_t vj = j < nw ? v[j] : 0;
    any |= vj;
    const uint64_t d = (uint64_t)0 - vj - borrow;  // two's complement, word by word
    c.neg[j] = j < nw ? (uint32_t)d : 0;
    borrow = (vj | borrow) ? 1 : 0;
  }
  c.lead = any ? 1 : 0;
  return c;
}

// X4, the G2 sum: chain t (0 or 1) of the tuple a
HB_HD Chain chain_x4_g2(const uint32_t a[4], int t) {
  const uint32_t u[WORDS] = {a[t], 0, 0}, v[WORDS] = {a[t + 2], 0, 0};
  return recode(u, v, 1);
}
// X4, the G1 sum
HB_HD Chain chain_x4_g1(const uint32_t a[4]) {
  uint32_t u[WORDS], v[WORDS];
  mul_add_x(a[0], a[1], u);
  mul_add_x(a[2], a[3], v);
  return recode(u, v, 3);
}
// X2 (G1 only): b0 = a[0..1], b1 = a[2..3]
HB_HD Chain chain_x2_g1(const uint32_t a[4]) {
  const uint32_t u[WORDS] = {a[0], a[1], 0}, v[WORDS] = {a[2], a[3], 0};
  return recode(u, v, 2);
}
HB_HD Chain chain_g1(int form, const uint32_t a[4]) { return form == FORM_X4 ? chain_x4_g1(a) : chain_x2_g1(a); }

// Table entry (0..3, see the top) of step i, i from steps - 1 down to 0
HB_HD int entry(const Chain& c, int i) {
  return (int)((c.pos[i >> 5] >> (i & 31)) & 1u) | (int)(((c.neg[i >> 5] >> (i & 31)) & 1u) << 1);
}

}  // namespace gd
