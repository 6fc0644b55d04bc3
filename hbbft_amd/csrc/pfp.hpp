// Lane-pair BLS12-381 tower for the fused pairing kernel (k_pair.hip), namespace hbs.
//
// Every Fp2 value a = a0 + a1 u is split over two adjacent lanes of a wave: the even lane holds a0,
// the odd lane a1 (signed 14 x 28-bit limbs of sfp.hpp).  An Fp6 / Fp12 value is then 3 / 6 such
// components per lane, so one check's whole Miller-loop and final-exponentiation state fits half a
// register file, and a 65,536-check batch runs two waves per SIMD -- the occupancy at which the MAD
// pipe is saturated (tools/ubench_v2.hip: 50 G Fp-mul/s at one wave per SIMD, 74 G at two).
//
// Fp2 arithmetic in this split does no redundant work:
//   a * b : the even lane forms a0 b0 - a1 b1, the odd lane a1 b0 + a0 b1 -- both are x y + z w with
//           x = own a, y = b0, z = -+partner a, w = b1; one lazily reduced product of 588 MADs per
//           lane (2 x 196 product + 196 reduction), exactly half of a 3 x 392-MAD Karatsuba product.
//   a^2   : even (a0 + a1)(a0 - a1), odd 2 a0 a1: one 392-MAD product per lane.
//   a * s (s in Fp), a + b, a - b: each lane on its own component.
// Partner operands travel through DPP quad permutations (one full-rate v_mov_dpp per limb): swap
// [1,0,3,2], broadcast-even [0,0,2,2], broadcast-odd [1,1,3,3].  Both lanes of a pair always take
// the same control flow (every branch below depends only on the check, never on the lane parity),
// so a DPP source lane is always active.
//
// Value contracts (per Fp component, signed, normalised = limbs 0..12 in [0, 2^28)):
//   h_mul(a, b): a normalised or lazy (|limb| <= 2^29), b normalised, |a|, |b| < 16p -> normalised,
//                |out| < 1.25p + |a||b| 2^-392 bound (column sums < 2^62.1).
//   h_sqr(a)   : a normalised, |a| < 16p -> normalised (fp_mul_l contract (M) on (a0+-a1, a0-a1)).
//   Fp12 values between operations are reduced (|.| < 2p).  The tower formulas are pairing 0.14's
//   (restated in oracle/c/bls_cpu.c: Karatsuba Fp6, complex Fp12 squaring, Granger-Scott squaring).
#pragma once
#include "sfp.hpp"
#include "words.hpp"

// words.hpp's inversion mode for the final exponentiation's inversions (h6_inv, and k_pair.hip's
// decompression), chosen per translation unit: k_pair.hip, where every lane pair of a wave inverts a
// different norm, takes the branch-free INV_UNIFORM; the other includers keep the per-divstep form.
#ifndef HP_INV_MODE
#define HP_INV_MODE 0
#endif

#define HP_D __device__ __forceinline__

namespace hbs {

// ---------------------------------------------------------------- lane pair
constexpr int DPP_SWAP = 0xB1;  // quad_perm [1,0,3,2]
constexpr int DPP_EVEN = 0xA0;  // quad_perm [0,0,2,2]
constexpr int DPP_ODD = 0xF5;   // quad_perm [1,1,3,3]

HP_D bool lp_even() { return (threadIdx.x & 1) == 0; }
template <int CTRL>
HP_D int32_t dpp(int32_t v) {
  return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
HP_D Fp dpp_fp(const Fp& a) {
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = dpp<CTRL>(a.l[i]);
  return r;
}

// own component of a * b (Fp2)
HS_MULFN Fp h_mul_l(HS_P14(x), HS_P14(y)) {
  const Fp a = {{HS_L14(x)}};
  const Fp b = {{HS_L14(y)}};
  const int32_t sm = lp_even() ? -1 : 0;  // the even lane subtracts a1 b1
  int32_t Y[NL], W[NL], Z[NL];
#pragma unroll
  for (int i = 0; i < NL; i++) {
    Y[i] = dpp<DPP_EVEN>(b.l[i]);
    W[i] = dpp<DPP_ODD>(b.l[i]);
    Z[i] = (dpp<DPP_SWAP>(a.l[i]) ^ sm) - sm;
  }
  int32_t m[NL];
  int64_t acc = 0;
  Fp r;
#pragma unroll
  for (int k = 0; k < NL; k++) {
#pragma unroll
    for (int i = 0; i <= k; i++) {
      acc += (int64_t)a.l[i] * Y[k - i];
      acc += (int64_t)Z[i] * W[k - i];
    }
#pragma unroll
    for (int i = 0; i < k; i++) acc += (int64_t)m[i] * (int32_t)P_L[k - i];
    m[k] = mont_digit(acc);
    acc += (int64_t)m[k] * (int32_t)P_L[0];
    acc >>= 28;
  }
#pragma unroll
  for (int k = NL; k < 2 * NL - 1; k++) {
#pragma unroll
    for (int i = k - NL + 1; i < NL; i++) {
      acc += (int64_t)a.l[i] * Y[k - i];
      acc += (int64_t)Z[i] * W[k - i];
      acc += (int64_t)m[i] * (int32_t)P_L[k - i];
    }
    r.l[k - NL] = (int32_t)acc & MASK28;
    acc >>= 28;
  }
  r.l[NL - 1] = (int32_t)acc;
  return r;
}

HP_D Fp h_mul(const Fp& a, const Fp& b) { return h_mul_l(HS_E14(a), HS_E14(b)); }

// own component of a^2: even (a0 + a1)(a0 - a1), odd (a1 + a1) a0... written as x * y with
// x = pa + (even ? a : pa), y = a - (even ? pa : 0)  (odd lane: x = 2 a0, y = a1)
HP_D Fp h_sqr(const Fp& a) {
  const bool ev = lp_even();
  const Fp pa = dpp_fp<DPP_SWAP>(a);
  Fp x, y;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    x.l[i] = pa.l[i] + (ev ? a.l[i] : pa.l[i]);
    y.l[i] = a.l[i] - (ev ? pa.l[i] : 0);
  }
  return fp_mul(x, y);
}

// The squaring of a + b s in Fp4 = Fp2[s] / (s^2 - xi), the block of the cyclotomic squarings
// (h12_cyclo_sqr, hc_sqr): A = a^2 + xi b^2, B = 2 a b = (a + b)^2 - a^2 - b^2.  HP_SQR4 = 1 takes
// it in one leaf (h_sqr4_l) with two Montgomery reductions, one per output, on the unreduced sums;
// 0 keeps three h_sqr, each with a reduction of its own (A/B: profiles/r23).
#ifndef HP_SQR4
#define HP_SQR4 1
#endif
#if HP_SQR4
typedef int32_t V28 __attribute__((ext_vector_type(2 * NL)));  // returns in v0..v27

// own components of (A, B): limbs 0..13 of the result are A's, 14..27 B's.
// Contract: a, b normalised, |.| < 2p -> A normalised, in (-p/20, p + p/20); B lazy, |limb| < 2^28
// (the top one < 2^19), |B| < 1.1p: an operand of fp_red_mk and h_add_xi_l, as the callers use it.
//
// The three squares are h_sqr's products x y with (x, y) = (a0 + a1, a0 - a1) on the even lane and
// (2 a0, a1) on the odd one: |x_i| < 2^29, |y_i| < 2^28 for a and for b, and the pair of a + b is the
// limb-wise sum of the two, |x_i| <= 2^30 - 4, |y_i| <= 2^29 - 2, not normalised.  They are product
// scans without Montgomery digits of their own.  With S(.) the unreduced squares and S'(b) the
// partner's component of S(b), xi (g + h u) = (g - h) + (g + h) u gives
//   A = S(a) + S(b) -/+ S'(b),  C = A + B = S(a + b) -/+ S'(b)     (even lane - , odd lane +)
// so only S(b) has to cross the lane pair.  Its chain alone is carry-extracted, column by column, to
// 28-bit limbs, which travel as one v_mov_dpp each; S(a)'s and S(a + b)'s products go straight into
// the Montgomery accumulators of A and C (fp_mul_l's digits and columns) together with those limbs.
// Montgomery reduction is linear, so B = C - A limb by limb.  Three MAD chains of products, two of
// digits; no 28-limb value is stored.
// int64: a column of A is < 14 x 2^57 + 14 x 2^56 + 2^30 and one of C < 14 x 2^59 + 14 x 2^56 + 2^29,
// with carries < 2^36: < 2^62.98, inside int64 because the product chain of a + b is the only one
// at 2^59 per term and the digits' terms are 2^56.  The unreduced sums are |A| < 48 p^2 and |C| < 80
// p^2, so the outputs (T + m P) / R with 0 <= m < R lie in (-80 p^2 / R, p + 80 p^2 / R), and p / R <
// 2^-11.  The headroom in C's accumulator is 1.6 %, and it rests on the operand pair of a + b staying
// within 2^30 - 4 and 2^29 - 2: a and b MUST be normalised (limbs 0..12 in [0, 2^28)), not merely
// |.| < 2p -- a lazy operand, which h_mul takes, overflows the int64 here without a sign of it.
// (tests/test_pair_sqr4_model.py restates this function statement by statement.)
HS_MULFN V28 h_sqr4_l(HS_P14(x), HS_P14(y)) {
  const Fp a = {{HS_L14(x)}};
  const Fp b = {{HS_L14(y)}};
  const int32_t sm = lp_even() ? -1 : 0;  // the even lane subtracts the partner's component
  int32_t xa[NL], ya[NL], xb[NL], yb[NL], xs[NL], ys[NL];
#pragma unroll
  for (int i = 0; i < NL; i++) {
    // x = a0 + partner's: a0 + a1 on the even lane, a0 + a0 on the odd; y = a - (even ? a1 : 0)
    const int32_t pa = dpp<DPP_SWAP>(a.l[i]), pb = dpp<DPP_SWAP>(b.l[i]);
    xa[i] = dpp<DPP_EVEN>(a.l[i]) + pa;
    ya[i] = a.l[i] - (pa & sm);
    xb[i] = dpp<DPP_EVEN>(b.l[i]) + pb;
    yb[i] = b.l[i] - (pb & sm);
    xs[i] = xa[i] + xb[i];
    ys[i] = ya[i] + yb[i];
  }
  int32_t mA[NL], mC[NL], A[NL], C[NL];
  int64_t cb = 0, ra = 0, rc = 0;
#pragma unroll
  for (int k = 0; k < 2 * NL - 1; k++) {
#pragma unroll
    for (int i = (k < NL ? 0 : k - NL + 1); i <= (k < NL ? k : NL - 1); i++) {
      ra += (int64_t)xa[i] * ya[k - i];
      cb += (int64_t)xb[i] * yb[k - i];
      rc += (int64_t)xs[i] * ys[k - i];
    }
    const int32_t lb = (int32_t)cb & MASK28;
    cb >>= 28;
    const int32_t w = (dpp<DPP_SWAP>(lb) ^ sm) - sm;
    ra += lb + w;
    rc += w;
    if (k < NL) {
#pragma unroll
      for (int i = 0; i < k; i++) {
        ra += (int64_t)mA[i] * (int32_t)P_L[k - i];
        rc += (int64_t)mC[i] * (int32_t)P_L[k - i];
      }
      mA[k] = mont_digit(ra);
      mC[k] = mont_digit(rc);
      ra += (int64_t)mA[k] * (int32_t)P_L[0];
      rc += (int64_t)mC[k] * (int32_t)P_L[0];
    } else {
#pragma unroll
      for (int i = k - NL + 1; i < NL; i++) {
        ra += (int64_t)mA[i] * (int32_t)P_L[k - i];
        rc += (int64_t)mC[i] * (int32_t)P_L[k - i];
      }
      A[k - NL] = (int32_t)ra & MASK28;
      C[k - NL] = (int32_t)rc & MASK28;
    }
    ra >>= 28;
    rc >>= 28;
  }
  // limb 27: the chains' last carries
  const int32_t tb = (int32_t)cb;
  const int32_t tw = (dpp<DPP_SWAP>(tb) ^ sm) - sm;
  A[NL - 1] = (int32_t)ra + tb + tw;
  C[NL - 1] = (int32_t)rc + tw;
  V28 r;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    r[i] = A[i];
    r[NL + i] = C[i] - A[i];
  }
  return r;
}

// B is lazy (signed limbs, not normalised): it must go through a carry pass (fp_red_mk, fp_norm)
// before it is the operand of any product
struct Sq4 { Fp A, B; };
HP_D Sq4 h_sqr4(const Fp& a, const Fp& b) {
  const V28 v = h_sqr4_l(HS_E14(a), HS_E14(b));
  Sq4 r;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    r.A.l[i] = v[i];
    r.B.l[i] = v[NL + i];
  }
  return r;
}
#endif

// a * (1 + u): even a0 - a1, odd a1 + a0
HP_D Fp h_mul_xi(const Fp& a) {
  const int32_t sm = lp_even() ? -1 : 0;
  const Fp pa = dpp_fp<DPP_SWAP>(a);
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = a.l[i] + ((pa.l[i] ^ sm) - sm);
  fp_norm(r);
  return r;
}
// conjugate: the odd lane negates
HP_D Fp h_conj(const Fp& a) {
  const Fp n = fp_neg(a);
  return lp_even() ? a : n;
}
HP_D Fp h_zero() { return fp_zero(); }
HP_D Fp h_one() { return lp_even() ? fp_one() : fp_zero(); }
// Fp2 constant (c0, c1): each lane takes its own component
HP_D Fp h_const(const uint32_t (&c0)[NL], const uint32_t (&c1)[NL]) {
  Fp r;
  const bool ev = lp_even();
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = (int32_t)(ev ? c0[i] : c1[i]);
  return r;
}
// pair-wide AND of a per-lane flag
HP_D bool lp_both(bool v) { return (v ? 1 : 0) & dpp<DPP_SWAP>(v ? 1 : 0); }
HP_D bool h_is_zero(const Fp& a) { return lp_both(fp_is_zero(a)); }
// hb::words_inv_uniform (words.hpp INV_UNIFORM) with its work split over the lane pair, which inverts
// one value: mode bit INV_PAIR beside INV_UNIFORM.  Both lanes run the 31 divsteps of a round on
// the approximations, but each follows one column of the update matrix only (even: f0, f1; odd: g0,
// g1) and holds one of (a, b) and one of (u, v) as its own: even a and u, odd b and v.  A lane
// multiplies its own values by its two factors, keeps the term of its own row and sends the other to
// its partner (one DPP swap per word), so each of the four rows is computed once per pair; the new a
// or b travels back for the next round's approximation.  Same rounds, divsteps and value as
// words_inv_uniform.
constexpr int INV_PAIR = 8;
template <int N>
HP_D void lp_inv_uniform(const uint32_t* y, const uint32_t* mod, uint32_t* out) {
  static_assert(N <= 15, "words_reduce_32m");
  const bool ev = lp_even();
  uint32_t mine[N], other[N], co[N + 1];  // even: a, b, u; odd: b, a, v
#pragma unroll
  for (int i = 0; i < N; i++) {
    mine[i] = ev ? y[i] : mod[i];
    other[i] = ev ? mod[i] : y[i];
    co[i] = 0;
  }
  co[N] = 0;
  co[0] = ev ? 1u : 0u;
  uint32_t inv = mod[0];
  for (int k = 0; k < 5; k++) inv *= 2u - mod[0] * inv;
  const uint32_t minv = 0u - inv;
  const int rounds = (2 * hb::words_bitlen<N>(mod) - 1 + 30) / 31;
#pragma unroll 1
  for (int r = 0; r < rounds; r++) {
    const uint64_t am = hb::words_approx<N>(mine, hb::words_len2<N>(mine, other));
    const uint64_t ao = (uint64_t)(uint32_t)dpp<DPP_SWAP>((int32_t)(uint32_t)am) |
                        ((uint64_t)(uint32_t)dpp<DPP_SWAP>((int32_t)(uint32_t)(am >> 32)) << 32);
    uint64_t ab = ev ? am : ao, bb = ev ? ao : am;
    uint32_t c0 = ev ? 1u : 0u, c1 = ev ? 0u : 1u;  // own column: row a's and row b's factor
#pragma unroll 1
    for (int j = 0; j < 31; j++) {
      uint32_t odd;
      bool sw;
      hb::words_divstep_ab(ab, bb, odd, sw);
      hb::words_divstep_col(c0, c1, odd, sw);
    }
    // k: the factor of the own row (even a', u'; odd b', v'); s: the one of the partner's row
    uint32_t km, ks, sm, ss;
    hb::words_fac_split(ev ? c0 : c1, km, ks);
    hb::words_fac_split(ev ? c1 : c0, sm, ss);
    {
      uint32_t t[N + 2], k[N + 2], row[N + 1];
      hb::words_mul_sm<N, false>(mine, sm, ss, t);
#pragma unroll
      for (int i = 0; i < N + 2; i++) t[i] = (uint32_t)dpp<DPP_SWAP>((int32_t)t[i]);
      hb::words_mul_sm<N, false>(mine, km, ks, k);
      uint64_t c = 0;
#pragma unroll
      for (int i = 0; i < N + 2; i++) {
        c += (uint64_t)k[i] + t[i];
        t[i] = (uint32_t)c;
        c >>= 32;
      }
#pragma unroll
      for (int i = 0; i <= N; i++) row[i] = (t[i] >> 31) | (t[i + 1] << 1);
      // a negated row negates its two factors: the own k, and the partner's s
      const uint32_t fl = hb::words_abs<N + 1>(row);
      ks ^= fl;
      ss ^= (uint32_t)dpp<DPP_SWAP>((int32_t)fl);
#pragma unroll
      for (int i = 0; i < N; i++) {
        mine[i] = row[i];
        other[i] = (uint32_t)dpp<DPP_SWAP>((int32_t)row[i]);
      }
    }
    {
      // own coefficient <- (own k + partner's s-term + q m) / 2^31 (words_lin_sm31's sum; a word's
      // two products, the partner's word and the carry stay below 2^64)
      uint32_t t[N + 2], w[N + 2];
      hb::words_mul_sm<N, true>(co, sm, ss, t);
#pragma unroll
      for (int i = 0; i < N + 2; i++) t[i] = (uint32_t)dpp<DPP_SWAP>((int32_t)t[i]);
      const uint32_t xe = 0u - (co[N] >> 31);
      const uint32_t k0 = km & ks;
      const uint64_t q = (uint64_t)(((k0 + (co[0] ^ ks) * km + t[0]) * minv) & 0x7fffffffu);
      uint64_t c = k0;
#pragma unroll
      for (int i = 0; i < N + 2; i++) {
        const uint32_t xi = (i <= N ? co[i] : xe) ^ ks;
        c += (uint64_t)xi * km;
        if (i < N) c += q * mod[i];
        c += t[i];
        w[i] = (uint32_t)c;
        c >>= 32;
      }
#pragma unroll
      for (int i = 0; i <= N; i++) co[i] = (w[i] >> 31) | (w[i + 1] << 1);
    }
  }
  // b is the odd lane's own value, v its coefficient
  const uint32_t mine_one = hb::words_is_one<N>(mine) ? 1u : 0u;
  const uint32_t part_one = (uint32_t)dpp<DPP_SWAP>((int32_t)mine_one);
  const bool one = (ev ? part_one : mine_one) != 0;
  uint32_t v[N + 1];
#pragma unroll
  for (int i = 0; i <= N; i++) {
    const uint32_t pv = (uint32_t)dpp<DPP_SWAP>((int32_t)co[i]);
    v[i] = ev ? pv : co[i];
  }
  hb::words_reduce_32m<N>(v, mod);
#pragma unroll
  for (int i = 0; i < N; i++) out[i] = one ? v[i] : 0u;
}

// 1 / a in Fp2 with a variable-time inverse of the (public) norm: both lanes invert the same norm.
// a = 0 gives 0 (the binary Euclid loop would not terminate on a zero norm).
template <int MODE = 0>
HP_D Fp h_inv_vartime(const Fp& a) {
  const Fp s = fp_sqr(a);
  const Fp n = fp_add(s, dpp_fp<DPP_SWAP>(s));
  uint32_t w[12], p[12], r[12];
  fp_to_words(n, w);
  uint32_t nz = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) nz |= w[i];
  if (nz == 0) return fp_zero();
#pragma unroll
  for (int i = 0; i < 12; i++) p[i] = hb::PM2_W[i];
  p[0] += 2;  // p - 2 + 2
  if ((MODE & INV_PAIR) != 0)
    lp_inv_uniform<12>(w, p, r);
  else
    hb::words_inv_vartime<12, MODE>(w, p, r);
  return h_conj(fp_mul(a, fp_from_words(r)));
}

// ---------------------------------------------------------------- one-pass reductions
// reduce(M t + K a) in one carry pass: t unnormalised limbs (|t_i| < 2^31), a normalised, |M|, |K|
// <= 3.  The quotient comes from the top limb alone (as in fp_reduce); the lower limbs' excess moves
// the value by < 2^368 < 2^-12 p, so the output is normalised and in (-p/1000, p + p/1000) --
// inside (R).  Replaces a normalisation pass per sum plus fp_reduce's pass.
// h6_mul6 and the scaled h6_mul_12 widen the contract as h_dbl_step_h's <12, 0> does: <3, 0>, <6, 0>
// and <1, 6> with |t_i| < 2^31, |a_i| < 2^31 and |M t + K a| < 64p.  The int64 terms stay below
// 7 x 2^31, the top limb of the sum below 64 x 1.7 x 2^16 < 2^23 (the quotient estimate's range), and
// the lower limbs' excess below 2^34 x 2^336 < p / 1000: the output bound is the same.
template <int M, int K>
HP_D Fp fp_red_mk(const Fp& t, const Fp& a) {
  const int64_t top = (int64_t)t.l[NL - 1] * M + (int64_t)K * a.l[NL - 1];
  const int32_t q = (int32_t)((top * QINV) >> 32);
  Fp r;
  int64_t acc = 0;
#pragma unroll
  for (int i = 0; i < NL - 1; i++) {
    acc += (int64_t)t.l[i] * M + (int64_t)K * a.l[i] - (int64_t)q * (int32_t)P_L[i];
    r.l[i] = (int32_t)acc & MASK28;
    acc >>= 28;
  }
  r.l[NL - 1] = (int32_t)(acc + top - (int64_t)q * (int32_t)P_L[NL - 1]);
  return r;
}
HP_D Fp fp_red_l(const Fp& t) { return fp_red_mk<1, 0>(t, t); }
// reduce(a + 2 b + 4 c) in one carry pass, a, b, c normalised with |.| < 4p: the sum is < 28p with
// limbs < 7 x 2^28, so the top limb is < 2^22 and the lower limbs' excess < 2^368, as in fp_red_mk;
// output normalised in (-p/1000, p + p/1000)
HP_D Fp fp_red_124(const Fp& a, const Fp& b, const Fp& c) {
  const int32_t top = a.l[NL - 1] + 2 * b.l[NL - 1] + 4 * c.l[NL - 1];
  const int32_t q = (int32_t)(((int64_t)top * QINV) >> 32);
  Fp r;
  int64_t acc = 0;
#pragma unroll
  for (int i = 0; i < NL - 1; i++) {
    acc += (int64_t)(a.l[i] + 2 * b.l[i] + 4 * c.l[i]) - (int64_t)q * (int32_t)P_L[i];
    r.l[i] = (int32_t)acc & MASK28;
    acc >>= 28;
  }
  r.l[NL - 1] = (int32_t)(acc + top - (int64_t)q * (int32_t)P_L[NL - 1]);
  return r;
}
// a + k1 b + k2 c for small signed k (1 + |k1| + |k2| <= 7), normalised
HP_D Fp fp_lin3(const Fp& a, int k1, const Fp& b, int k2, const Fp& c) {
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = a.l[i] + k1 * b.l[i] + k2 * c.l[i];
  fp_norm(r);
  return r;
}
// own component of s + xi t without normalising (|s_i| + 2 |t_i| < 2^31)
HP_D Fp h_add_xi_l(const Fp& s, const Fp& t) {
  const int32_t sm = lp_even() ? -1 : 0;
  const Fp pt = dpp_fp<DPP_SWAP>(t);
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = s.l[i] + t.l[i] + ((pt.l[i] ^ sm) - sm);
  return r;
}
// a - b - c without normalising
HP_D Fp fp_sub2l(const Fp& a, const Fp& b, const Fp& c) {
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = a.l[i] - b.l[i] - c.l[i];
  return r;
}

// own component of xi t without normalising
HP_D Fp h_xi_l(const Fp& t) {
  const int32_t sm = lp_even() ? -1 : 0;
  const Fp pt = dpp_fp<DPP_SWAP>(t);
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = t.l[i] + ((pt.l[i] ^ sm) - sm);
  return r;
}

// ---------------------------------------------------------------- Fp6 / Fp12 (own components)
struct H6 { Fp c0, c1, c2; };
struct H12 { H6 c0, c1; };

HP_D H6 h6_zero() { return {h_zero(), h_zero(), h_zero()}; }
HP_D H6 h6_one() { return {h_one(), h_zero(), h_zero()}; }
HP_D H6 h6_add(const H6& a, const H6& b) { return {fp_add(a.c0, b.c0), fp_add(a.c1, b.c1), fp_add(a.c2, b.c2)}; }
HP_D H6 h6_sub(const H6& a, const H6& b) { return {fp_sub(a.c0, b.c0), fp_sub(a.c1, b.c1), fp_sub(a.c2, b.c2)}; }
HP_D H6 h6_neg(const H6& a) { return {fp_neg(a.c0), fp_neg(a.c1), fp_neg(a.c2)}; }
HP_D H6 h6_red(const H6& a) { return {fp_reduce(a.c0), fp_reduce(a.c1), fp_reduce(a.c2)}; }
HP_D H6 h6_mul_v(const H6& a) { return {h_mul_xi(a.c2), a.c0, a.c1}; }

// Karatsuba, inputs < 4p; outputs reduced (one carry pass each, fp_red_l).  Register-frugal order:
// each output is formed as soon as its products exist (c0 before t1, t2 are computed), so at most
// five Fp2 values are live beside the operands across the product calls.
HP_D H6 h6_mul(const H6& a, const H6& b) {
  const Fp v1 = h_mul(a.c1, b.c1);
  const Fp v2 = h_mul(a.c2, b.c2);
  const Fp d0 = fp_sub2l(h_mul(fp_addl(a.c1, a.c2), fp_add(b.c1, b.c2)), v1, v2);
  const Fp v0 = h_mul(a.c0, b.c0);
  const Fp c0 = fp_red_l(h_add_xi_l(v0, d0));  // v0 + xi (t0 - v1 - v2)
  const Fp c1 = fp_red_l(h_add_xi_l(fp_sub2l(h_mul(fp_addl(a.c0, a.c1), fp_add(b.c0, b.c1)), v0, v1), v2));
  const Fp c2 = fp_red_l(fp_addl(fp_sub2l(h_mul(fp_addl(a.c0, a.c2), fp_add(b.c0, b.c2)), v0, v2), v1));
  return {c0, c1, c2};
}
// 6 a b by Toom-Cook-3: five Fp2 products, on the evaluations at 0, 1, -1, 2 and infinity, instead
// of Karatsuba's six.  The interpolation has integer coefficients only because it stops at 6 a b:
//   P0 = a0 b0, Pi = a2 b2, P1 = a(1) b(1), Pm = a(-1) b(-1), P2 = a(2) b(2)
//   t = P2 + 3 (P0 - P1) - Pm                      (6 a b's v^3 coefficient is t - 12 Pi)
//   c0 = 6 P0 + xi (t - 12 Pi)            = xi t + 6 (P0 - 2 xi Pi)
//   c1 = 3 (P1 - Pm) - t + 12 Pi + 6 xi Pi = 3 (P1 - Pm) - t + 6 (2 Pi + xi Pi)
//   c2 = 3 (P1 + Pm - 2 P0 - 2 Pi)
// The factor 6 is in Fp, so a Miller-loop value that carries it (any power of it) has the same
// final exponentiation: c^(p^6 - 1) = 1.  Only h12_sqr and h12_mul_lines use this product.
//
// Contract: a normalised, |a_i| < 4p; b normalised, |b0| + 2 |b1| + 4 |b2| < 16p (|b_i| < 2.28p);
// outputs reduced.  Operands of the products: a(1) = (a0 + a2) + a1 lazy, limbs < 2^29, < 12p;
// a(-1) lazy, |limb| < 2^28, < 12p; a(2) reduced in its own pass (28p before it); b(1), b(-1) < 7p
// and b(2) < 16p normalised.  So every product is normalised (limbs 0..12 in [0, 2^28)) and in
// (-0.2p, 1.4p): 1.25p + 2 x 12p x 7p x 2^-392 < 1.33p.
// int32: P1 + Pm - 2 P0 - 2 Pi in (-2^30, 2^29); m = 3 (P0 - P1) - Pm and t = P2 + m in (-2^30, 2^30),
// xi t in (-2^31, 2^31); 3 (P1 - Pm) - t in +-7 x 2^28; P0 - 2 xi Pi in +-5 x 2^28; 2 Pi + xi Pi in
// (-2^28, 2^30).  Values into the passes, with |P| < 1.33p: |c0| < 2 x 8 x 1.33p + 6 x 5 x 1.33p =
// 61.2p, |c1| < 14 x 1.33p + 6 x 4 x 1.33p = 50.6p, |c2| < 18 x 1.33p: inside fp_red_mk's 64p.
// Register order: P1, Pm, P0, Pi, then c2 and the four sums that the last two outputs need, then
// P2: five values are live beside the operands across the last product, as in h6_mul.
HP_D H6 h6_mul6(const H6& a, const H6& b) {
  Fp c2, m, e, k, h;
  {
    const Fp sa = fp_add(a.c0, a.c2);
    const Fp p1 = h_mul(fp_addl(sa, a.c1), fp_lin3(b.c0, 1, b.c1, 1, b.c2));
    const Fp pm = h_mul(fp_subl(sa, a.c1), fp_lin3(b.c0, -1, b.c1, 1, b.c2));
    const Fp p0 = h_mul(a.c0, b.c0);
    const Fp pi = h_mul(a.c2, b.c2);
    const Fp xpi = h_xi_l(pi);
    Fp w;
#pragma unroll
    for (int i = 0; i < NL; i++) {
      w.l[i] = p1.l[i] + pm.l[i] - 2 * p0.l[i] - 2 * pi.l[i];
      m.l[i] = 3 * (p0.l[i] - p1.l[i]) - pm.l[i];
      e.l[i] = p1.l[i] - pm.l[i];
      k.l[i] = p0.l[i] - 2 * xpi.l[i];
      h.l[i] = 2 * pi.l[i] + xpi.l[i];
    }
    c2 = fp_red_mk<3, 0>(w, w);
  }
  const Fp t = fp_addl(h_mul(fp_red_124(a.c0, a.c1, a.c2), fp_lin3(b.c0, 2, b.c1, 4, b.c2)), m);
  const Fp c0 = fp_red_mk<1, 6>(h_xi_l(t), k);
  Fp g;
#pragma unroll
  for (int i = 0; i < NL; i++) g.l[i] = 3 * e.l[i] - t.l[i];
  const Fp c1 = fp_red_mk<1, 6>(g, h);
  return {c0, c1, c2};
}
HP_D H6 h6_inv(const H6& a) {
  const Fp c0 = fp_reduce(fp_sub(h_sqr(a.c0), h_mul_xi(h_mul(a.c1, a.c2))));
  const Fp c1 = fp_reduce(fp_sub(h_mul_xi(h_sqr(a.c2)), h_mul(a.c0, a.c1)));
  const Fp c2 = fp_reduce(fp_sub(h_sqr(a.c1), h_mul(a.c0, a.c2)));
  const Fp t = fp_reduce(fp_add(h_mul(a.c0, c0), h_mul_xi(fp_add(h_mul(a.c2, c1), h_mul(a.c1, c2)))));
  // the final exponentiation's one inversion: values are public (share checks), so the binary-GCD
  // inverse (25 rounds of 31 divsteps) replaces Fermat's 380 squarings + ~190 products (A/B on one
  // box: sign 23.4 -> 22.7 ms, decrypt 21.6 -> 20.8 ms per 65,536 checks, profiles/r03/ab_inv.txt)
  const Fp ti = fp_reduce(h_inv_vartime<HP_INV_MODE>(t));
  return {h_mul(c0, ti), h_mul(c1, ti), h_mul(c2, ti)};
}

HP_D H12 h12_one() { return {h6_one(), h6_zero()}; }
HP_D H12 h12_conj(const H12& a) { return {a.c0, h6_neg(a.c1)}; }
HP_D H12 h12_red(const H12& a) { return {h6_red(a.c0), h6_red(a.c1)}; }
// Karatsuba recombination (t0 + v t1, s - t0 - t1) of normalised Fp6 products, reduced in one pass
// per component
HP_D H12 h12_kcomb(const H6& t0, const H6& t1, const H6& s) {
  return {{fp_red_l(h_add_xi_l(t0.c0, t1.c2)), fp_red_l(fp_addl(t0.c1, t1.c0)), fp_red_l(fp_addl(t0.c2, t1.c1))},
          {fp_red_l(fp_sub2l(s.c0, t0.c0, t1.c0)), fp_red_l(fp_sub2l(s.c1, t0.c1, t1.c1)),
           fp_red_l(fp_sub2l(s.c2, t0.c2, t1.c2))}};
}

// x (b1 v + b2 v^2): c0 = xi (a1 b2 + a2 b1), c1 = a0 b1 + xi a2 b2, c2 = a0 b2 + a1 b1 (5 products);
// outputs reduced.  S: the product comes out times S (1, or 6 beside h6_mul6), multiplied inside the
// carry passes: the sums are < 3 x 2^28 per limb and < 7.8p (xi of three products of < 1.3p), so
// 6 times them is < 47p, inside fp_red_mk's widened contract.
template <int S = 1>
HP_D H6 h6_mul_12(const H6& x, const Fp& b1, const Fp& b2) {
  const Fp u = h_mul(x.c1, b1);
  const Fp w = h_mul(x.c2, b2);
  const Fp d0 = h_xi_l(fp_sub2l(h_mul(fp_addl(x.c1, x.c2), fp_add(b1, b2)), u, w));
  const Fp c0 = fp_red_mk<S, 0>(d0, d0);
  const Fp d1 = h_add_xi_l(h_mul(x.c0, b1), w);
  const Fp c1 = fp_red_mk<S, 0>(d1, d1);
  const Fp d2 = fp_addl(h_mul(x.c0, b2), u);
  const Fp c2 = fp_red_mk<S, 0>(d2, d2);
  return {c0, c1, c2};
}

// ---------------------------------------------------------------- Fp12 over a lane group
// The Fp12 operations of the pairing check, written once for the lane pair, the lane quad (qfp.hpp)
// and the lane octo (ofp.hpp).  G is the width's policy (LanePair below, LaneQuad, LaneOcto): a
// struct of static functions that says how many independent Fp2 products run side by side.  These
// use
//   G::mul6x2(a0, b0, a1, b1, r0, r1)         the dual Fp6 product (a0 b0, a1 b1)
//   G::mul6x2_12(a0, b0, a1, c1, c2, r0, r1)  the same with b1 = (0, c1, c2)
//   G::mul6(a, b)                             one Fp6 product
//   G::line_product(a0 .. b4, C0, c11, c12)   the product (C0, (0, c11, c12)) of two sparse lines
//   G::miller_mul6x2 / miller_mul6x2_12 / miller_mul6   the same three products as the Miller loop
//                                             takes them: times G::MILLER_SCALE, a factor in Fp
// An operand of a dual product may be a callable that returns it (h6_of): a width that runs the two
// products one after the other forms the second one's operands after the first product, so that
// they are not live across its calls.
HP_D const H6& h6_of(const H6& a) { return a; }
template <class F>
HP_D auto h6_of(const F& f) -> decltype(f()) { return f(); }

// inputs reduced; output reduced
template <class G>
HP_D H12 h12_mul(const H12& a, const H12& b) {
  H6 t0, t1;
  G::mul6x2(a.c0, b.c0, a.c1, b.c1, t0, t1);
  const H6 s = G::mul6(h6_add(a.c0, a.c1), h6_add(b.c0, b.c1));
  return h12_kcomb(t0, t1, s);
}
// complex squaring: t = a0 a1, s = (a0 + a1)(a0 + v a1); c0 = s - t - v t, c1 = 2 t (one pass each)
// Miller loop only: it takes the width's Miller-loop products (miller_mul6x2 here, miller_mul6x2_12
// and miller_mul6 in h12_mul_lines), which come out times G::MILLER_SCALE, so the value is that
// factor times the square; every formula here and in h12_mul_lines is linear in its Fp6 products,
// so the factor carries through.
template <class G>
HP_D H12 h12_sqr(const H12& a) {
  H6 t, s;
  const auto a1 = [&]() HS_LAMBDA { return h6_add(a.c0, a.c1); };
  const auto b1 = [&]() HS_LAMBDA { return h6_red(h6_add(a.c0, h6_mul_v(a.c1))); };
  G::miller_mul6x2(a.c0, a.c1, a1, b1, t, s);
  return {{fp_red_l(h_add_xi_l(fp_subl(s.c0, t.c0), fp_subl(fp_zero(), t.c2))), fp_red_l(fp_sub2l(s.c1, t.c1, t.c0)),
           fp_red_l(fp_sub2l(s.c2, t.c2, t.c1))},
          {fp_red_l(fp_addl(t.c0, t.c0)), fp_red_l(fp_addl(t.c1, t.c1)), fp_red_l(fp_addl(t.c2, t.c2))}};
}
// f * (la * lb) for two sparse lines (c0 + c1 w^2 + c4 w^3 each, normalised, < 2p): the line
// product L = (C0, C1) has C1.c0 = 0 (6 products), then one Karatsuba step over Fp6 with the sparse
// C1 -- on the lane pair 6 + 5 + 6 products, 23 in all instead of 2 x 13 for one line at a time.
// Miller loop only: G::MILLER_SCALE times the product (see h12_sqr).  first: f is the 1 that the
// Miller loop starts from (lane_verify, where G::first_line says so): the line product itself is
// the new f, whatever f holds.
template <class G>
HP_D H12 h12_mul_lines(const H12& f, const Fp& a0, const Fp& a1, const Fp& a4, const Fp& b0, const Fp& b1,
                       const Fp& b4, bool first = false) {
  H6 C0, t0, t1;
  Fp c11, c12;
  G::line_product(a0, a1, a4, b0, b1, b4, C0, c11, c12);
  if (first) return {C0, {h_zero(), c11, c12}};
  G::miller_mul6x2_12(f.c0, C0, f.c1, c11, c12, t0, t1);
  const H6 s = G::miller_mul6(h6_add(f.c0, f.c1), {C0.c0, fp_add(C0.c1, c11), fp_add(C0.c2, c12)});
  return h12_kcomb(t0, t1, s);
}
template <class G>
HP_D H12 h12_inv(const H12& a) {
  H6 s0, s1, r0, r1;
  G::mul6x2(a.c0, a.c0, a.c1, a.c1, s0, s1);
  const H6 t = h6_red(h6_sub(h6_red(s0), h6_red(h6_mul_v(h6_red(s1)))));
  const H6 ti = h6_red(h6_inv(t));
  G::mul6x2(a.c0, ti, a.c1, ti, r0, r1);
  return h12_red({r0, h6_neg(r1)});
}

#define HP_FROB1(K) h_const(hb::FROB1_##K##_C0, hb::FROB1_##K##_C1)
HP_D H12 h12_frob1(const H12& f) {
  H12 r;
  r.c0.c0 = h_conj(f.c0.c0);
  r.c1.c0 = h_mul(h_conj(f.c1.c0), HP_FROB1(1));
  r.c0.c1 = h_mul(h_conj(f.c0.c1), HP_FROB1(2));
  r.c1.c1 = h_mul(h_conj(f.c1.c1), HP_FROB1(3));
  r.c0.c2 = h_mul(h_conj(f.c0.c2), HP_FROB1(4));
  r.c1.c2 = h_mul(h_conj(f.c1.c2), HP_FROB1(5));
  return h12_red(r);
}
HP_D H12 h12_frob2(const H12& f) {
  H12 r;
  r.c0.c0 = f.c0.c0;
  r.c1.c0 = fp_mul(f.c1.c0, fp_const(hb::FROB2_1_C0));
  r.c0.c1 = fp_mul(f.c0.c1, fp_const(hb::FROB2_2_C0));
  r.c1.c1 = fp_mul(f.c1.c1, fp_const(hb::FROB2_3_C0));
  r.c0.c2 = fp_mul(f.c0.c2, fp_const(hb::FROB2_4_C0));
  r.c1.c2 = fp_mul(f.c1.c2, fp_const(hb::FROB2_5_C0));
  return r;
}

// Granger-Scott cyclotomic squaring, input reduced, output reduced.
// Each output 3 A -/+ 2 a is formed from the unnormalised squares and reduced in one carry pass
// (fp_red_mk) instead of normalising A, the linear combination and the reduction separately.
HP_D H12 h12_cyclo_sqr(const H12& f) {
  const Fp& a0 = f.c0.c0; const Fp& a2 = f.c0.c1; const Fp& a4 = f.c0.c2;
  const Fp& a1 = f.c1.c0; const Fp& a3 = f.c1.c1; const Fp& a5 = f.c1.c2;
  H12 r;
#if HP_SQR4
  // h_sqr4: A normalised, in (-p/20, 21p/20), inside h_sqr's (-p/8, 9p/8); B lazy, |limb| < 2^28, |B| <
  // 1.1p.  Into the passes: |3 A - 2 a| < 3.15p + 4p, |3 B + 2 a| < 3.3p + 4p, and with xi on B (|limb|
  // < 2^29, |.| < 2.2p) < 6.6p + 4p: under fp_red_mk's 64p with |t_i| < 2^31; outputs in (-p/1000, p +
  // p/1000), reduced
  {
    const Sq4 s = h_sqr4(a0, a3);
    r.c0.c0 = fp_red_mk<3, -2>(s.A, a0);
    r.c1.c1 = fp_red_mk<3, 2>(s.B, a3);
  }
  {
    const Sq4 s = h_sqr4(a1, a4);
    r.c0.c1 = fp_red_mk<3, -2>(s.A, a2);
    r.c1.c2 = fp_red_mk<3, 2>(s.B, a5);
  }
  {
    const Sq4 s = h_sqr4(a2, a5);
    r.c0.c2 = fp_red_mk<3, -2>(s.A, a4);
    r.c1.c0 = fp_red_mk<3, 2>(h_add_xi_l(fp_zero(), s.B), a1);
  }
#else
  {
    const Fp s0 = h_sqr(a0), s3 = h_sqr(a3), s03 = h_sqr(fp_add(a0, a3));
    r.c0.c0 = fp_red_mk<3, -2>(h_add_xi_l(s0, s3), a0);
    r.c1.c1 = fp_red_mk<3, 2>(fp_sub2l(s03, s0, s3), a3);
  }
  {
    const Fp s1 = h_sqr(a1), s4 = h_sqr(a4), s14 = h_sqr(fp_add(a1, a4));
    r.c0.c1 = fp_red_mk<3, -2>(h_add_xi_l(s1, s4), a2);
    r.c1.c2 = fp_red_mk<3, 2>(fp_sub2l(s14, s1, s4), a5);
  }
  {
    const Fp s2 = h_sqr(a2), s5 = h_sqr(a5), s25 = h_sqr(fp_add(a2, a5));
    r.c0.c2 = fp_red_mk<3, -2>(h_add_xi_l(s2, s5), a4);
    r.c1.c0 = fp_red_mk<3, 2>(h_add_xi_l(fp_zero(), fp_sub2l(s25, s2, s5)), a1);
  }
#endif
  return r;
}

// ---------------------------------------------------------------- compressed cyclotomic squaring
// Karabina's compressed form of a cyclotomic element keeps four of the six coefficients of
// sum a_k w^k: (a1, a2, a4, a5).  It is closed under squaring -- the new (a1, a2, a4, a5) are exactly
// the second and third blocks of h12_cyclo_sqr, which never read a0 or a3 -- so a chain of squarings
// costs six lane-pair squares each instead of nine.  a0 and a3 come back from
//   a3 = (xi a5^2 + 3 a2^2 - 2 a4) / (4 a1),  a0 = (2 a3^2 + a1 a5 - 3 a4 a2) xi + 1,
// valid whenever a1 != 0 (hc_decompress takes 1 / (4 a1) from the caller, who shares one inversion
// among several elements).  a1 = 0 happens for real inputs: 1 compresses to four zeros.
struct HC { Fp a1, a2, a4, a5; };

HP_D HC hc_compress(const H12& f) { return {f.c1.c0, f.c0.c1, f.c0.c2, f.c1.c2}; }
// input reduced, output reduced: h12_cyclo_sqr's formulas, bounds and carry passes (with HP_SQR4,
// the bounds in the comment at the head of its HP_SQR4 branch: 3 A - 2 a_k, 3 B + 2 a_k, and xi on B)
HP_D HC hc_sqr(const HC& c) {
  HC r;
#if HP_SQR4
  {
    const Sq4 s = h_sqr4(c.a1, c.a4);
    r.a2 = fp_red_mk<3, -2>(s.A, c.a2);
    r.a5 = fp_red_mk<3, 2>(s.B, c.a5);
  }
  {
    const Sq4 s = h_sqr4(c.a2, c.a5);
    r.a4 = fp_red_mk<3, -2>(s.A, c.a4);
    r.a1 = fp_red_mk<3, 2>(h_add_xi_l(fp_zero(), s.B), c.a1);
  }
#else
  {
    const Fp s1 = h_sqr(c.a1), s4 = h_sqr(c.a4), s14 = h_sqr(fp_add(c.a1, c.a4));
    r.a2 = fp_red_mk<3, -2>(h_add_xi_l(s1, s4), c.a2);
    r.a5 = fp_red_mk<3, 2>(fp_sub2l(s14, s1, s4), c.a5);
  }
  {
    const Fp s2 = h_sqr(c.a2), s5 = h_sqr(c.a5), s25 = h_sqr(fp_add(c.a2, c.a5));
    r.a4 = fp_red_mk<3, -2>(h_add_xi_l(s2, s5), c.a4);
    r.a1 = fp_red_mk<3, 2>(h_add_xi_l(fp_zero(), fp_sub2l(s25, s2, s5)), c.a1);
  }
#endif
  return r;
}
// the denominator 4 a1 of a3: a1 reduced -> normalised, |.| < 8p (a product operand)
HP_D Fp hc_denom(const Fp& a1) { return fp_lin(4, a1, 0, a1); }
// c reduced, di = 1 / (4 a1) normalised and < 2p -> the full element, reduced.  2 squares + 3
// products.
HP_D H12 hc_decompress(const HC& c, const Fp& di) {
  const Fp s5 = h_sqr(c.a5), s2 = h_sqr(c.a2);  // (-p/8, 9p/8)
  // xi s5 + 3 s2 - 2 a4: limbs < 2^29 + 3 2^28 before the pass, |.| < 2.25p + 3.4p + 4p
  Fp t = h_xi_l(s5);
#pragma unroll
  for (int i = 0; i < NL; i++) t.l[i] += 3 * s2.l[i];
  const Fp a3 = h_mul(fp_red_mk<1, -2>(t, c.a4), di);  // < 1.26p
  // 2 a3^2 - 3 a4 a2 normalised (|.| < 6.1p), + a1 a5 lazy (limbs < 2^29, |.| < 7.4p); times xi, plus
  // 1: limbs < 2^28 + 2 2^29 and |.| < 16p before the one carry pass
  const Fp u = fp_addl(fp_lin(2, h_sqr(a3), -3, h_mul(c.a4, c.a2)), h_mul(c.a1, c.a5));
  const Fp a0 = fp_red_l(h_add_xi_l(h_one(), u));
  return {{a0, c.a2, c.a4}, {c.a1, a3, c.a5}};
}

HP_D bool h12_is_one(const H12& f) {
  bool ok = fp_is_zero(fp_sub(f.c0.c0, h_one()));
  ok = ok && fp_is_zero(f.c0.c1) && fp_is_zero(f.c0.c2);
  ok = ok && fp_is_zero(f.c1.c0) && fp_is_zero(f.c1.c1) && fp_is_zero(f.c1.c2);
  return lp_both(ok);
}

// ---------------------------------------------------------------- G2 walk (pairing 0.14's line formulas)
// T in Jacobian coordinates; lines scaled as pairing 0.14 scales them (the Fp2 factors die in the final
// exponentiation).  Each lane holds its components of T, Q and the line.
struct HJac { Fp x, y, z; };
struct HLine { Fp c0, c1, c4; };

// ---------------------------------------------------------------- G2 walk, homogeneous coordinates
// T = (X : Y : Z) with x = X / Z, y = Y / Z on the twist y^2 = x^3 + b', b' = 4 xi (Costello-Lange-
// Naehrig's a = 0 formulas, scaled by 4 to clear the halves; tools/gen_wave_prog.py miller1 states
// the same walk for the wave kernels, there with 12 xi Z carried along, which a sequential lane pair
// does not need).  The lines are the Jacobian walk's (qfp.hpp h_dbl_step_q / h_add_step_q) times a
// nonzero Fp2 factor (a power of the Jacobian Z), which the final exponentiation removes.  No formula
// inverts, so the dummy walk of a masked pair from (1 : 1 : 1) is harmless.
//
// Bounds.  T's coordinates enter and leave every step normalised with |.| < 2p (fp_reduce's (R), or
// an h_mul output, < 1.26p whenever both operands are < 8p: 1.25p + 64 p^2 2^-392 and p 2^-392 <
// 2^-10).  h_sqr gives (-p/8, 9p/8) for |a| < 16p.  Every h_mul / h_sqr / fp_mul operand below is
// normalised, or lazy with |limb| <= 2^29, and stays under 8p; the sums are bounded line by line.
struct HProj { Fp x, y, z; };

// 6 lane-pair squares + 3 lane-pair products = 6 x 392 + 3 x 588 = 4,116 MADs per lane (the Jacobian
// doubling step: 7 squares + 4 products = 5,096).
//   E = 3 b' Z^2 = 12 xi Z^2;  line (Y^2 - E, -3 X^2, 2 Y Z)
//   X3 = 2 X Y (Y^2 - 3E),  Y3 = (Y^2 + 3E)^2 - 12 E^2,  Z3 = 4 Y^2 (2 Y Z)
HP_D HLine h_dbl_step_h(HProj& T) {
  // Z's and Y's squares first, X's uses last: 0.1 ms per 65,536 checks faster than starting with
  // X Y (fewer spills in the sign instantiation, profiles/r09/README.md)
  const Fp C = h_sqr(T.z);  // (-p/8, 9p/8)
  const Fp YZ = h_sqr(fp_add(T.y, T.z));  // (Y + Z) < 4p
  const Fp B = h_sqr(T.y);  // (-p/8, 9p/8)
  // H = (Y + Z)^2 - B - C = 2 Y Z: |H| < 3.4p, normalised by the two fp_sub
  const Fp H = fp_sub(fp_sub(YZ, B), C);
  // 12 xi C in one carry pass: h_xi_l's limbs are < 2^29 and its value < 2.25p, so 12 times it is
  // < 27p with int64 terms < 2^33 -- inside fp_red_mk's quotient estimate (top limb < 2^23).
  // |E| < 1.01p, normalised.
  const Fp E = fp_red_mk<12, 0>(h_xi_l(C), C);
  const Fp A = h_mul(T.x, T.y);  // < 1.26p
  const Fp S = h_sqr(T.x);
  HLine l;
  l.c0 = fp_red_mk<1, -1>(B, E);  // B - E, < 2.2p before the pass, reduced
  l.c1 = fp_lin(-3, S, 0, S);     // |.| < 3.4p, normalised: an fp_mul operand
  l.c4 = H;
  const Fp Bm = fp_lin(1, B, -3, E);  // B - 3E, |.| < 4.2p
  const Fp Bp = fp_lin(1, B, 3, E);   // B + 3E, |.| < 4.2p
  // X3 = (2A)(B - 3E): 2A is lazy (|limb| < 2^29), |2A| < 2.6p; the product is < 1.26p
  T.x = h_mul(fp_addl(A, A), Bm);
  // Y3 = Bp^2 - 12 E^2: 9p/8 + 12 x 9p/8 < 14.7p, int64 terms < 2^32; reduced in one pass
  const Fp EE = h_sqr(E);
  T.y = fp_red_mk<1, -12>(h_sqr(Bp), EE);
  // Z3 = 2 ((2B) H): the product is < 1.26p, doubled inside the carry pass
  const Fp BH = h_mul(fp_addl(B, B), H);
  T.z = fp_red_mk<2, 0>(BH, BH);
  return l;
}

// Mixed addition T += Q, Q affine: 2 squares + 11 products = 2 x 392 + 11 x 588 = 7,252 MADs per lane.
// The Jacobian addition step is 3 squares + 10 products = 7,056, but it needs T in Jacobian form, and
// the conversion (X Z : Y Z^2 : Z) costs a square and two products more than the 196 MADs it saves;
// there are 5 addition steps against 63 doublings.
//   theta = Y - yQ Z, lambda = X - xQ Z;  line (theta xQ - lambda yQ, -theta, lambda)
//   G = X lambda^2, H = lambda^3 + Z theta^2 - 2G
//   X3 = lambda H,  Y3 = theta (G - H) - Y lambda^3,  Z3 = Z lambda^3
// xQ, yQ are fp_from_words outputs (or 1): (-p/8, 9p/8).
HP_D HLine h_add_step_h(HProj& T, const Fp& xQ, const Fp& yQ) {
  const Fp th = fp_sub(T.y, h_mul(yQ, T.z));  // |.| < 3.3p
  const Fp la = fp_sub(T.x, h_mul(xQ, T.z));  // |.| < 3.3p
  HLine l;
  l.c0 = fp_reduce(fp_sub(h_mul(th, xQ), h_mul(la, yQ)));  // < 2.6p before the pass
  l.c1 = fp_neg(th);
  l.c4 = la;
  const Fp C = h_sqr(th);
  const Fp D = h_sqr(la);
  const Fp E = h_mul(la, D);   // lambda^3, < 1.26p
  const Fp F = h_mul(T.z, C);  // < 1.26p
  const Fp G = h_mul(T.x, D);  // < 1.26p
  const Fp H = fp_lin(1, fp_addl(E, F), -2, G);  // limbs < 2^30 before the pass; |H| < 5.1p
  const Fp X3 = h_mul(la, H);                    // < 1.26p
  // theta (G - H) - E Y: (G - H) < 6.4p; the difference of the two products is < 2.6p
  T.y = fp_reduce(fp_sub(h_mul(th, fp_sub(G, H)), h_mul(E, T.y)));
  T.z = h_mul(T.z, E);  // < 1.26p
  T.x = X3;
  return l;
}

// ---------------------------------------------------------------- one side of the Miller loop
// Register budget (2 waves per SIMD = 256 VGPRs per lane): a side whose P is the generator (GEN)
// keeps no P in registers -- the line evaluation multiplies by constants -- and a walked side keeps
// only T: Q itself is re-read from memory at the 5 addition steps instead of living in 28 VGPRs
// through the 63 doublings.
//
// PT: the coordinates T walks in, the width policy's Walk
template <class PT>
struct SideStateT {
  Fp xP, yP;      // P (Montgomery), both lanes (unused when GEN)
  bool act;       // pair contributes (P != O and Q != O)
  bool qinf;      // WALK: Q is the point at infinity (the walk runs from (1, 1), masked out)
  uint32_t q;     // Q index
  PT T;           // WALK: the running multiple of Q (own components)
};

template <bool GEN, class ST>
HP_D Fp side_xP(const ST& st) { return GEN ? fp_const(hb::G1X_M) : st.xP; }
template <bool GEN, class ST>
HP_D Fp side_yP(const ST& st, bool negate) {
  return GEN ? (negate ? fp_neg(fp_const(hb::G1Y_M)) : fp_const(hb::G1Y_M)) : st.yP;
}

// ---------------------------------------------------------------- Miller-loop parking
// A width's parking hook, G::Park<W1, W2, GEN>: where a WALK side's T and a read side's P wait while
// f is squared and multiplied by the lines, which is about three quarters of a Miller step and uses
// neither.  lane_verify (pair_side.hpp) makes one per check over the lane's column of the
// workgroup's LDS stash, calls init() once both sides are initialised, walks T through walk() and
// hands the hook to lines_at_p for P.  NoPark leaves everything in the sides' registers.
struct NoPark {
  HP_D explicit NoPark(uint32_t*) {}
  template <class ST>
  HP_D void init(const ST&, const ST&) const {}
  // f(T): one walk step of side SIDE (0 = A, 1 = B), which returns its raw line
  template <int SIDE, class ST, class F>
  HP_D HLine walk(ST& st, const F& f) const { return f(st.T); }
  template <int SIDE, class ST>
  HP_D Fp xP(const ST& st) const { return st.xP; }
  template <int SIDE, class ST>
  HP_D Fp yP(const ST& st) const { return st.yP; }
};

// The lane pair's: the Miller loop never touches the stash of the final exponentiation (the first
// stash12 comes after the loop), so the lane's column holds T and P as plain 32-bit words, limbs as
// they are -- word k at col[k * 256], a ds_read_b32 / ds_write_b32 per limb with the wave's lanes on
// consecutive banks.  Each lane reads only what it wrote: no barrier.  First fit into the
// PARK_WORDS words in the order T of side B, T of side A, P of side A, P of side B; what does not
// fit stays in the side's registers (slot -1):
//   TABLE / WALK (either order) with a generator side   T + P = 70 words
//   TABLE / TABLE, both P read                          P + P = 56
//   WALK / WALK                                         side B's T + one P = 70; side A's T stays
// The accesses are volatile: the calls between a store and its load have no memory effects, so the
// compiler would forward the stored registers to the load, and hoist P's loads out of the loop --
// that is, keep all of it in registers across the calls and spill it to scratch as before.
constexpr int PARK_WORDS = 72;  // a lane's column of the stash (pair_side.hpp STASH_WORDS)
constexpr int park_fit(int used, bool need, int words) { return need && used + words <= PARK_WORDS ? used : -1; }
typedef volatile __attribute__((address_space(3))) uint32_t* ParkCol;

HP_D void park_put(ParkCol c, int slot, const Fp& a) {
#pragma unroll
  for (int i = 0; i < NL; i++) c[(slot + i) * 256] = (uint32_t)a.l[i];
}
HP_D Fp park_get(ParkCol c, int slot) {
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = (int32_t)c[(slot + i) * 256];
  return r;
}

template <bool W1, bool W2, int GEN>
struct PairPark {
  static constexpr int TW = 3 * NL, PW = 2 * NL;
  static constexpr int T_B = park_fit(0, W2, TW);
  static constexpr int U1 = T_B < 0 ? 0 : TW;
  static constexpr int T_A = park_fit(U1, W1, TW);
  static constexpr int U2 = U1 + (T_A < 0 ? 0 : TW);
  static constexpr int P_A = park_fit(U2, GEN != 1, PW);
  static constexpr int U3 = U2 + (P_A < 0 ? 0 : PW);
  static constexpr int P_B = park_fit(U3, GEN != 2, PW);
  template <int SIDE>
  static constexpr int t_slot() { return SIDE == 0 ? T_A : T_B; }
  template <int SIDE>
  static constexpr int p_slot() { return SIDE == 0 ? P_A : P_B; }

  ParkCol col;
  HP_D explicit PairPark(uint32_t* c) : col((ParkCol)c) {}

  template <int SIDE>
  HP_D void put_T(const HProj& T) const {
    park_put(col, t_slot<SIDE>(), T.x);
    park_put(col, t_slot<SIDE>() + NL, T.y);
    park_put(col, t_slot<SIDE>() + 2 * NL, T.z);
  }
  template <int SIDE, class ST>
  HP_D void init_side(const ST& st) const {
    if constexpr (t_slot<SIDE>() >= 0) put_T<SIDE>(st.T);
    if constexpr (p_slot<SIDE>() >= 0) {
      park_put(col, p_slot<SIDE>(), st.xP);
      park_put(col, p_slot<SIDE>() + NL, st.yP);
    }
  }
  template <class ST>
  HP_D void init(const ST& A, const ST& B) const {
    init_side<0>(A);
    init_side<1>(B);
  }
  template <int SIDE, class ST, class F>
  HP_D HLine walk(ST& st, const F& f) const {
    if constexpr (t_slot<SIDE>() < 0) {
      return f(st.T);
    } else {
      HProj T;  // in the order the doubling step takes them up
      T.z = park_get(col, t_slot<SIDE>() + 2 * NL);
      T.y = park_get(col, t_slot<SIDE>() + NL);
      T.x = park_get(col, t_slot<SIDE>());
      const HLine l = f(T);
      put_T<SIDE>(T);
      return l;
    }
  }
  template <int SIDE, class ST>
  HP_D Fp xP(const ST& st) const {
    if constexpr (p_slot<SIDE>() < 0) return st.xP; else return park_get(col, p_slot<SIDE>());
  }
  template <int SIDE, class ST>
  HP_D Fp yP(const ST& st) const {
    if constexpr (p_slot<SIDE>() < 0) return st.yP; else return park_get(col, p_slot<SIDE>() + NL);
  }
};

// ---------------------------------------------------------------- the lane pair as a width policy
// What the shared Fp12 operations above and the kernel body and final exponentiation of
// pair_side.hpp ask of a width.  The lane pair runs every product on its own, one after the other.
struct LanePair {
  static constexpr int LANES = 2;
  static HP_D bool leader() { return lp_even(); }   // writes the verdict
  static HP_D bool value_writer() { return true; }  // each lane writes its component of the value
  using Walk = HProj;                               // a WALK side's T is homogeneous
  static HP_D HLine dbl_step(HProj& T) { return h_dbl_step_h(T); }
  static HP_D HLine add_step(HProj& T, const Fp& xQ, const Fp& yQ) { return h_add_step_h(T, xQ, yQ); }

  static HP_D H6 mul6(const H6& a, const H6& b) { return h6_mul(a, b); }
  template <class A1, class B1>
  static HP_D void mul6x2(const H6& a0, const H6& b0, const A1& a1, const B1& b1, H6& r0, H6& r1) {
    r0 = h6_mul(a0, b0);
    r1 = h6_mul(h6_of(a1), h6_of(b1));
  }
  static HP_D void mul6x2_12(const H6& a0, const H6& b0, const H6& a1, const Fp& c1, const Fp& c2, H6& r0, H6& r1) {
    r0 = h6_mul(a0, b0);
    r1 = h6_mul_12(a1, c1, c2);  // 5 products
  }
  // The Miller loop's products (h12_sqr, h12_mul_lines) come out times MILLER_SCALE, a factor in Fp
  // that the final exponentiation removes: 6 with the five-product h6_mul6, and the sparse product
  // brought to the same factor in its carry passes.  h12_mul, h12_inv and the whole final
  // exponentiation keep the exact products above: a cyclotomic element must not be scaled.
  // (Measured against Karatsuba products with no factor in profiles/r19.)
  static constexpr int MILLER_SCALE = 6;
  static HP_D H6 miller_mul6(const H6& a, const H6& b) { return h6_mul6(a, b); }
  template <class A1, class B1>
  static HP_D void miller_mul6x2(const H6& a0, const H6& b0, const A1& a1, const B1& b1, H6& r0, H6& r1) {
    r0 = h6_mul6(a0, b0);
    r1 = h6_mul6(h6_of(a1), h6_of(b1));
  }
  static HP_D void miller_mul6x2_12(const H6& a0, const H6& b0, const H6& a1, const Fp& c1, const Fp& c2, H6& r0,
                                    H6& r1) {
    r0 = h6_mul6(a0, b0);
    r1 = h6_mul_12<MILLER_SCALE>(a1, c1, c2);
  }
  // the first step's line product is taken as f (17 products less) in the checks that walk a side;
  // a TABLE / TABLE check was slower with it (profiles/r19)
  template <bool W1, bool W2>
  static constexpr bool first_line() { return W1 || W2; }
  // each coefficient is reduced (one carry pass) as soon as its products exist
  static HP_D void line_product(const Fp& a0, const Fp& a1, const Fp& a4, const Fp& b0, const Fp& b1, const Fp& b4,
                                H6& C0, Fp& c11, Fp& c12) {
    const Fp a0b0 = h_mul(a0, b0);
    const Fp a1b1 = h_mul(a1, b1);
    const Fp a4b4 = h_mul(a4, b4);
    c11 = fp_red_l(fp_sub2l(h_mul(fp_addl(a0, a4), fp_add(b0, b4)), a0b0, a4b4));
    c12 = fp_red_l(fp_sub2l(h_mul(fp_addl(a1, a4), fp_add(b1, b4)), a1b1, a4b4));
    C0 = {fp_red_l(h_add_xi_l(a0b0, a4b4)), fp_red_l(fp_sub2l(h_mul(fp_addl(a0, a1), fp_add(b0, b1)), a0b0, a1b1)),
          a1b1};
  }
  static HP_D H12 cyclo_sqr(const H12& f) { return h12_cyclo_sqr(f); }
  static HP_D H12 frob1(const H12& f) { return h12_frob1(f); }
  static HP_D H12 frob2(const H12& f) { return h12_frob2(f); }

  template <bool W1, bool W2, int GEN>
  using Park = PairPark<W1, W2, GEN>;  // against NoPark: profiles/r18

  // a side's line (c0, c1, c4) evaluated at its P: (c0, c1 xP, c4 yP), or 1 for an inactive pair.
  // P comes from the parking hook (the side's registers, or the stash), each coordinate as its
  // product is due.
  template <bool GEN, int SIDE, class ST, class PK>
  static HP_D HLine line_at_p(const HLine& l, const ST& st, bool negate, const PK& pk) {
    HLine e;
    e.c0 = st.act ? l.c0 : h_one();
    const Fp c1 = fp_mul(l.c1, GEN ? side_xP<true>(st) : pk.template xP<SIDE>(st));
    e.c1 = st.act ? c1 : fp_zero();
    const Fp c4 = fp_mul(l.c4, GEN ? side_yP<true>(st, negate) : pk.template yP<SIDE>(st));
    e.c4 = st.act ? c4 : fp_zero();
    return e;
  }
  // both sides' lines of a step: raw_a() / raw_b() walk the side's T or read its table.  A side is
  // walked and evaluated before the other one is walked: side A first, or, WALK_FIRST (TABLE / WALK),
  // side B, so that the table's evaluated line is not live across the walk.  la and lb are the same
  // values either way.
  template <bool G1, bool G2, bool WALK_FIRST, class RA, class RB, class ST, class PK>
  static HP_D void lines_at_p(const RA& raw_a, const RB& raw_b, const ST& A, const ST& B, bool neg2, HLine& la,
                              HLine& lb, const PK& pk) {
    if constexpr (WALK_FIRST) {
      lb = line_at_p<G2, 1>(raw_b(), B, neg2, pk);
      la = line_at_p<G1, 0>(raw_a(), A, false, pk);
    } else {
      la = line_at_p<G1, 0>(raw_a(), A, false, pk);
      lb = line_at_p<G2, 1>(raw_b(), B, neg2, pk);
    }
  }
};

// ---------------------------------------------------------------- boundary formats
// own component of an ABI G2 coordinate pair (x.c0 x.c1 y.c0 y.c1, 12 words each)
HP_D void h_g2_load(const uint32_t* __restrict__ w, Fp& x, Fp& y) {
  const int o = lp_even() ? 0 : 12;
  x = fp_from_words(w + o);
  y = fp_from_words(w + 24 + o);
}
HP_D bool words_zero(const uint32_t* __restrict__ w, int n) {
  uint32_t o = 0;
  for (int k = 0; k < n; k++) o |= w[k];
  return o == 0;
}

}  // namespace hbs
