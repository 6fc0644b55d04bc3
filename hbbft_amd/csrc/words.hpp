// Multi-word (32-bit limb) helpers shared by both field representations (fp.hpp, and the lane-pair
// kernels over sfp.hpp): canonical-word comparisons and the variable-time binary-Euclid inverse.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define HW_HD __host__ __device__ __forceinline__
#else
#define HW_HD inline
#endif

namespace hb {

// Variable-time inverse for public values (the affine outputs of combines and scalar multiples,
// the final exponentiation's one inversion in the wave kernel): a batched binary GCD over canonical
// 32-bit words.  Divergent across lanes, so kernels where every lane inverts keep the uniform
// Fermat form.
template <int N>
HW_HD bool words_is_one(const uint32_t* x) {
  uint32_t o = x[0] ^ 1u;
  for (int i = 1; i < N; i++) o |= x[i];
  return o == 0;
}
template <int N>
HW_HD void words_shr1(uint32_t* x, uint32_t top) {
  for (int i = 0; i < N - 1; i++) x[i] = (x[i] >> 1) | (x[i + 1] << 31);
  x[N - 1] = (x[N - 1] >> 1) | (top << 31);
}
template <int N>
HW_HD uint32_t words_add(uint32_t* x, const uint32_t* y) {
  uint64_t c = 0;
  for (int i = 0; i < N; i++) {
    c += (uint64_t)x[i] + y[i];
    x[i] = (uint32_t)c;
    c >>= 32;
  }
  return (uint32_t)c;
}
template <int N>
HW_HD uint32_t words_sub(uint32_t* x, const uint32_t* y) {  // returns the borrow
  uint64_t br = 0;
  for (int i = 0; i < N; i++) {
    const uint64_t d = (uint64_t)x[i] - y[i] - br;
    x[i] = (uint32_t)d;
    br = (d >> 63) & 1;
  }
  return (uint32_t)br;
}
template <int N>
HW_HD bool words_geq(const uint32_t* x, const uint32_t* y) {
  for (int i = N - 1; i >= 0; i--)
    if (x[i] != y[i]) return x[i] > y[i];
  return true;
}
// Bit length of an N-word value (0 for zero); branch-free over the words so that x stays in VGPRs.
template <int N>
HW_HD int words_bitlen(const uint32_t* x) {
  int len = 0;
#pragma unroll
  for (int i = 0; i < N; i++)
    if (x[i]) len = 32 * i + 32 - __builtin_clz(x[i]);
  return len;
}
// 64 bits of x starting at bit s (bits beyond the top read as zero), selected without dynamic
// register indexing
template <int N>
HW_HD uint64_t words_bits64(const uint32_t* x, int s) {
  const int w = s >> 5, sh = s & 31;
  uint32_t lo = 0, mid = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    lo = (i == w) ? x[i] : lo;
    mid = (i == w + 1) ? x[i] : mid;
    hi = (i == w + 2) ? x[i] : hi;
  }
  const uint64_t v = (uint64_t)lo | ((uint64_t)mid << 32);
  return sh ? (v >> sh) | ((uint64_t)hi << (64 - sh)) : v;
}
// t = x * fx + y * fy (x, y < 2^(32N) unsigned; |fx|, |fy| <= 2^31) as an (N+2)-word two's-complement
// value, shifted right (arithmetically) by 31 bits into N+1 words
template <int N>
HW_HD void words_lincomb_shr31(const uint32_t* x, int64_t fx, const uint32_t* y, int64_t fy, uint32_t* out) {
  uint32_t t[N + 2];
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const int64_t p1 = (int64_t)x[i] * fx, p2 = (int64_t)y[i] * fy;
    const int64_t sw = (int64_t)(uint32_t)p1 + (int64_t)(uint32_t)p2 + c;
    t[i] = (uint32_t)sw;
    c = (sw >> 32) + (p1 >> 32) + (p2 >> 32);
  }
  t[N] = (uint32_t)c;
  t[N + 1] = (uint32_t)(c >> 32);
#pragma unroll
  for (int i = 0; i <= N; i++) out[i] = (t[i] >> 31) | (t[i + 1] << 1);
}
template <int N>
HW_HD bool words_neg_if(uint32_t* x, bool neg) {  // two's-complement negation of N words when neg
  if (!neg) return false;
  uint64_t c = 1;
#pragma unroll
  for (int i = 0; i < N; i++) {
    c += (uint64_t)(uint32_t)~x[i];
    x[i] = (uint32_t)c;
    c >>= 32;
  }
  return true;
}

// out = (x fx + y fy + q mod) / 2^31 for signed (N+1)-word x, y (two's complement, top word signed),
// |fx|, |fy| <= 2^31, q in [0, 2^31) chosen (minv = -mod^-1 mod 2^32) so the sum is divisible by 2^31;
// out has N+1 words, signed (the caller keeps |out| < 2^(32N+31))
template <int N>
HW_HD void words_lin_mont31(const uint32_t* x, int64_t fx, const uint32_t* y, int64_t fy, const uint32_t* mod,
                            uint32_t minv, uint32_t* out) {
  const uint32_t t0 = (uint32_t)((uint64_t)x[0] * (uint64_t)fx + (uint64_t)y[0] * (uint64_t)fy);
  const uint64_t q = (uint64_t)((t0 * minv) & 0x7fffffffu);
  uint32_t t[N + 2];
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i <= N; i++) {
    const int64_t xi = i < N ? (int64_t)x[i] : (int64_t)(int32_t)x[N];
    const int64_t yi = i < N ? (int64_t)y[i] : (int64_t)(int32_t)y[N];
    const int64_t p1 = xi * fx, p2 = yi * fy;
    const uint64_t p3 = i < N ? q * mod[i] : 0;
    const int64_t sw = (int64_t)(uint32_t)p1 + (int64_t)(uint32_t)p2 + (int64_t)(uint32_t)p3 + c;
    t[i] = (uint32_t)sw;
    c = (sw >> 32) + (p1 >> 32) + (p2 >> 32) + (int64_t)(p3 >> 32);
  }
  t[N + 1] = (uint32_t)c;
#pragma unroll
  for (int i = 0; i <= N; i++) out[i] = (t[i] >> 31) | (t[i + 1] << 1);
}

// out = a^-1 mod `mod` (odd modulus of at most 32N - 2 bits, a canonical); 0 when a is 0 or not
// invertible.  Variable time, for public values only.  T. Pornin's optimized binary GCD
// (eprint 2020/972, Algorithm 2): the binary GCD's 2 len(m) - 1 divsteps in rounds of 31, each round
// deciding on 64-bit approximations of (a, b) -- the low 31 bits and the top 33 bits -- and then
// applying the round's 2x2 update matrix to the full a, b and to the coefficients u, v (divided
// by 2^31 mod m, Montgomery style).  ~25 rounds for a 381-bit modulus instead of ~760 multiword
// shift / subtract steps.  Fixed round count: no data-dependent termination.
// MODE (for callers whose lanes invert the same value, the wave kernels' one inversion; divergent
// callers keep 0): bit 0 (INV_BATCH) takes a run of even divsteps at once (count trailing zeros,
// shift, double the coefficients) -- the same divsteps in ~1/3 of the loop iterations; bit 1
// (INV_LAZY) takes the bit length of a | b once and keeps the coefficients u, v signed and unreduced across the
// rounds (one reduction at the end) -- fewer instructions, but more live registers: the two-wave
// k_wave64 takes it, the 256-register k_wave does not (it spills there).
// Bit 2 (INV_UNIFORM) is for callers whose lanes invert DIFFERENT values (the lane-pair pairing
// kernel: 32 checks, 32 GCD traces per wave): words_inv_uniform below, the same rounds and divsteps
// with no data-dependent branch, so that a wave runs one instruction stream instead of every side
// of every branch.  It ignores the other two bits.
constexpr int INV_BATCH = 1, INV_LAZY = 2, INV_UNIFORM = 4;

// A round's update factor f in (-2^31, 2^31], held in a wrapped 32-bit word (0x80000000 is +2^31:
// -2^31 does not occur, see words_inv_uniform), as magnitude and sign mask (0 or ~0)
HW_HD void words_fac_split(uint32_t f, uint32_t& mag, uint32_t& sgn) {
  const uint32_t s = 0u - (f >> 31);
  mag = (f ^ s) - s;
  sgn = mag == 0x80000000u ? 0u : s;
}
// out = (x f + y g [+ q mod]) / 2^31 in N+1 words, f = +-fm and g = +-gm given as magnitude and sign
// mask, fm + gm <= 2^31.  SIGNED: x, y are (N+1)-word two's-complement values and q in [0, 2^31) makes
// the sum divisible by 2^31 (words_lin_mont31's contract and value); else x, y are unsigned N-word
// values and the quotient is floored (words_lincomb_shr31's).  A negative factor multiplies the
// complemented words and adds its magnitude once (-x = ~x + 1), so every product is unsigned and the
// sum is right modulo 2^(32 (N+2)); a word's three products and the carry stay below 2^64.
template <int N, bool SIGNED>
HW_HD void words_lin_sm31(const uint32_t* x, uint32_t fm, uint32_t fs, const uint32_t* y, uint32_t gm, uint32_t gs,
                          const uint32_t* mod, uint32_t minv, uint32_t* out) {
  const uint32_t xe = SIGNED ? 0u - (x[N] >> 31) : 0u, ye = SIGNED ? 0u - (y[N] >> 31) : 0u;
  const uint32_t c0 = (fm & fs) + (gm & gs);
  uint64_t q = 0;
  if (SIGNED) q = (uint64_t)(((c0 + (x[0] ^ fs) * fm + (y[0] ^ gs) * gm) * minv) & 0x7fffffffu);
  uint32_t t[N + 2];
  uint64_t c = c0;
#pragma unroll
  for (int i = 0; i < N + 2; i++) {
    const uint32_t xi = (i < N + (SIGNED ? 1 : 0) ? x[i] : xe) ^ fs;
    const uint32_t yi = (i < N + (SIGNED ? 1 : 0) ? y[i] : ye) ^ gs;
    c += (uint64_t)xi * fm + (uint64_t)yi * gm;
    if (SIGNED && i < N) c += q * mod[i];
    t[i] = (uint32_t)c;
    c >>= 32;
  }
#pragma unroll
  for (int i = 0; i <= N; i++) out[i] = (t[i] >> 31) | (t[i + 1] << 1);
}
// t = x f modulo 2^(32 (N+2)) in N+2 words, one term of words_lin_sm31's sum: f = +-m as magnitude
// and sign mask, x an (N+1)-word two's-complement value if SIGNED, else unsigned N words
template <int N, bool SIGNED>
HW_HD void words_mul_sm(const uint32_t* x, uint32_t m, uint32_t s, uint32_t* t) {
  const uint32_t xe = SIGNED ? 0u - (x[N] >> 31) : 0u;
  uint64_t c = m & s;
#pragma unroll
  for (int i = 0; i < N + 2; i++) {
    const uint32_t xi = (i < N + (SIGNED ? 1 : 0) ? x[i] : xe) ^ s;
    c += (uint64_t)xi * m;
    t[i] = (uint32_t)c;
    c >>= 32;
  }
}
// |x| for an N-word two's-complement x; returns the sign mask (~0 if x was negative)
template <int N>
HW_HD uint32_t words_abs(uint32_t* x) {
  const uint32_t s = 0u - (x[N - 1] >> 31);
  uint64_t c = s & 1u;
#pragma unroll
  for (int i = 0; i < N; i++) {
    c += (uint64_t)(x[i] ^ s);
    x[i] = (uint32_t)c;
    c >>= 32;
  }
  return s;
}
// n = max(64, len(a | b)) for N-word a, b, by selects
template <int N>
HW_HD int words_len2(const uint32_t* a, const uint32_t* b) {
  int n = 64;
#pragma unroll
  for (int i = 2; i < N; i++) {
    const uint32_t o = a[i] | b[i];
    n = o ? 32 * i + 32 - __builtin_clz(o) : n;
  }
  return n;
}
// a round's 64-bit approximation of N-word x: its low 31 bits below its bits n-33 ... n-1 (n >= 64),
// picked by selects; no shift count reaches the operand width
template <int N>
HW_HD uint64_t words_approx(const uint32_t* x, int n) {
  const int s = n - 33, w = s >> 5, sh = s & 31;  // s >= 31
  uint32_t lo = 0, mid = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    lo = (i == w) ? x[i] : lo;
    mid = (i == w + 1) ? x[i] : mid;
    hi = (i == w + 2) ? x[i] : hi;
  }
  const uint64_t t = (((uint64_t)lo | ((uint64_t)mid << 32)) >> sh) | ((((uint64_t)hi) << 1) << (63 - sh));
  return ((uint64_t)x[0] & 0x7fffffffu) | (t << 31);
}
// one divstep on the approximations: if a is odd and a < b, (a, b) <- (b - a, a), else if a is odd,
// a <- a - b; then a <- a / 2.  odd: mask of "a was odd"; sw: the swap was taken
HW_HD void words_divstep_ab(uint64_t& ab, uint64_t& bb, uint32_t& odd, bool& sw) {
  odd = 0u - ((uint32_t)ab & 1u);
  const uint64_t bm = bb & (((uint64_t)odd << 32) | odd);
  sw = ab < bm;
  const uint64_t d = ab - bm, nd = bm - ab;
  bb = sw ? ab : bb;
  ab = (sw ? nd : d) >> 1;
}
// the same divstep on one column (f0, f1) or (g0, g1) of the round's update matrix
HW_HD void words_divstep_col(uint32_t& c0, uint32_t& c1, uint32_t odd, bool sw) {
  const uint32_t x0 = sw ? c1 : c0, x1 = sw ? c0 : c1;
  c0 = x0 - (x1 & odd);
  c1 = x1 << 1;
}
// signed (N+1)-word v, |v| < 32 m, into [0, m): v + 32 m is in (0, 64 m); subtract 2^k m, k = 5 ... 0,
// wherever it leaves no borrow
template <int N>
HW_HD void words_reduce_32m(uint32_t* v, const uint32_t* mod) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i <= N; i++) {
    const uint32_t mk = (i < N ? mod[i] << 5 : 0u) | (i > 0 ? mod[i - 1] >> 27 : 0u);
    c += (uint64_t)v[i] + mk;
    v[i] = (uint32_t)c;
    c >>= 32;
  }
#pragma unroll
  for (int k = 5; k >= 0; k--) {
    uint32_t t[N + 1];
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i <= N; i++) {
      const uint32_t mk = (i < N ? mod[i] << k : 0u) | (i > 0 ? (mod[i - 1] >> 1) >> (31 - k) : 0u);
      const uint64_t d = (uint64_t)v[i] - mk - br;
      t[i] = (uint32_t)d;
      br = (d >> 63) & 1;
    }
#pragma unroll
    for (int i = 0; i <= N; i++) v[i] = br ? v[i] : t[i];
  }
}

// words_inv_vartime<N, 0>'s value by the same rounds and divsteps without a data-dependent branch
// or loop.
//   * A divstep selects: swap if a is odd and a < b, subtract if a is odd, halve.
//   * The update factors are wrapped 32-bit words.  |f| + |g| <= 2^31 in each row, so 2^31 itself
//     occurs only beside a zero: the row then says a' 2^31 = +-2^31 a (or b) on the 64-bit
//     approximations, which are exact non-negative integers under the divsteps, and a' >= 0, a, b > 0
//     there make the sign +.  Hence (-2^31, 2^31], and 0x80000000 reads as +2^31.
//   * The rows are applied as magnitude and sign mask (words_lin_sm31); making a', b' non-negative
//     flips a row's sign masks.
//   * u, v stay signed and unreduced as in INV_LAZY: each round adds at most m to the bound, so
//     |v| <= rounds m; v + 32 m is in (0, 64 m) and six masked subtractions of 32 m ... m bring it
//     into [0, m).
template <int N>
HW_HD void words_inv_uniform(const uint32_t* y, const uint32_t* mod, uint32_t* out) {
  static_assert(N <= 15, "rounds <= 31: |v| < 32 m, and 64 m fits N+1 words");
  uint32_t a[N + 1], b[N + 1], u[N + 1], v[N + 1];
#pragma unroll
  for (int i = 0; i < N; i++) {
    a[i] = y[i];
    b[i] = mod[i];
    u[i] = 0;
    v[i] = 0;
  }
  a[N] = b[N] = u[N] = v[N] = 0;
  u[0] = 1;
  uint32_t inv = mod[0];
  for (int k = 0; k < 5; k++) inv *= 2u - mod[0] * inv;
  const uint32_t minv = 0u - inv;
  const int rounds = (2 * words_bitlen<N>(mod) - 1 + 30) / 31;
#pragma unroll 1
  for (int r = 0; r < rounds; r++) {
    const int n = words_len2<N>(a, b);
    uint64_t ab = words_approx<N>(a, n), bb = words_approx<N>(b, n);
    uint32_t f0 = 1, g0 = 0, f1 = 0, g1 = 1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int j = 0; j < 31; j++) {
      uint32_t odd;
      bool sw;
      words_divstep_ab(ab, bb, odd, sw);
      words_divstep_col(f0, f1, odd, sw);
      words_divstep_col(g0, g1, odd, sw);
    }
    uint32_t m0, s0, m1, s1, m2, s2, m3, s3;
    words_fac_split(f0, m0, s0);
    words_fac_split(g0, m1, s1);
    words_fac_split(f1, m2, s2);
    words_fac_split(g1, m3, s3);
    uint32_t na[N + 1], nb[N + 1];
    words_lin_sm31<N, false>(a, m0, s0, b, m1, s1, mod, minv, na);
    words_lin_sm31<N, false>(a, m2, s2, b, m3, s3, mod, minv, nb);
    const uint32_t fa = words_abs<N + 1>(na), fb = words_abs<N + 1>(nb);
    s0 ^= fa;
    s1 ^= fa;
    s2 ^= fb;
    s3 ^= fb;
#pragma unroll
    for (int i = 0; i <= N; i++) {
      a[i] = na[i];
      b[i] = nb[i];
    }
    uint32_t nu[N + 1], nv[N + 1];
    words_lin_sm31<N, true>(u, m0, s0, v, m1, s1, mod, minv, nu);
    words_lin_sm31<N, true>(u, m2, s2, v, m3, s3, mod, minv, nv);
#pragma unroll
    for (int i = 0; i <= N; i++) {
      u[i] = nu[i];
      v[i] = nv[i];
    }
  }
  const bool one = b[N] == 0 && words_is_one<N>(b);
  words_reduce_32m<N>(v, mod);
#pragma unroll
  for (int i = 0; i < N; i++) out[i] = one ? v[i] : 0u;
}

template <int N, int MODE = 0>
HW_HD void words_inv_vartime(const uint32_t* y, const uint32_t* mod, uint32_t* out) {
  if ((MODE & INV_UNIFORM) != 0) {
    words_inv_uniform<N>(y, mod, out);
    return;
  }
  constexpr bool BATCH = (MODE & INV_BATCH) != 0, LAZY = (MODE & INV_LAZY) != 0;
  uint32_t a[N + 1], b[N + 1], u[N + 1], v[N + 1];
#pragma unroll
  for (int i = 0; i < N; i++) {
    a[i] = y[i];
    b[i] = mod[i];
    u[i] = 0;
    v[i] = 0;
  }
  a[N] = b[N] = u[N] = v[N] = 0;
  u[0] = 1;
  // -mod^-1 mod 2^32 (Newton)
  uint32_t inv = mod[0];
  for (int k = 0; k < 5; k++) inv *= 2u - mod[0] * inv;
  const uint32_t minv = 0u - inv;
  const int rounds = (2 * words_bitlen<N>(mod) - 1 + 30) / 31;
  for (int r = 0; r < rounds; r++) {
    int n;
    if (LAZY) {  // max(len a, len b) = len(a | b) (in k_wave this form measured slower: kept to k_wave64)
      uint32_t o[N];
#pragma unroll
      for (int i = 0; i < N; i++) o[i] = a[i] | b[i];
      n = words_bitlen<N>(o);
    } else {
      n = words_bitlen<N>(a);
      const int nb = words_bitlen<N>(b);
      if (nb > n) n = nb;
    }
    if (n < 64) n = 64;
    uint64_t ab = ((uint64_t)a[0] & 0x7fffffffu) | (words_bits64<N>(a, n - 33) << 31);
    uint64_t bb = ((uint64_t)b[0] & 0x7fffffffu) | (words_bits64<N>(b, n - 33) << 31);
    int64_t f0 = 1, g0 = 0, f1 = 0, g1 = 1;
    if (BATCH) {
      int j = 0;
      while (true) {
        const int tz = ab ? __builtin_ctzll(ab) : 64;
        const int z = tz < 31 - j ? tz : 31 - j;  // even divsteps
        ab >>= z;
        f1 <<= z;
        g1 <<= z;
        j += z;
        if (j >= 31) break;
        if (ab < bb) {  // odd divstep
          const uint64_t t = ab;
          ab = bb;
          bb = t;
          int64_t q = f0;
          f0 = f1;
          f1 = q;
          q = g0;
          g0 = g1;
          g1 = q;
        }
        ab = (ab - bb) >> 1;
        f0 -= f1;
        g0 -= g1;
        f1 *= 2;
        g1 *= 2;
        if (++j >= 31) break;
      }
    }
    for (int j = 0; j < (BATCH ? 0 : 31); j++) {
      if (ab & 1) {
        if (ab < bb) {
          const uint64_t t = ab;
          ab = bb;
          bb = t;
          int64_t q = f0;
          f0 = f1;
          f1 = q;
          q = g0;
          g0 = g1;
          g1 = q;
        }
        ab = (ab - bb) >> 1;
        f0 -= f1;
        g0 -= g1;
      } else {
        ab >>= 1;
      }
      f1 *= 2;
      g1 *= 2;
    }
    uint32_t na[N + 1], nbw[N + 1];
    words_lincomb_shr31<N>(a, f0, b, g0, na);
    words_lincomb_shr31<N>(a, f1, b, g1, nbw);
    if (words_neg_if<N + 1>(na, (int32_t)na[N] < 0)) {
      f0 = -f0;
      g0 = -g0;
    }
    if (words_neg_if<N + 1>(nbw, (int32_t)nbw[N] < 0)) {
      f1 = -f1;
      g1 = -g1;
    }
#pragma unroll
    for (int i = 0; i <= N; i++) {
      a[i] = na[i];
      b[i] = nbw[i];
    }
    if (LAZY) {
      // (u, v) <- ((u f0 + v g0) / 2^31, (u f1 + v g1) / 2^31), signed and NOT reduced mod m: with
      // |f0| + |g0| <= 2^31 (and the same for f1, g1) each round adds at most m to the bound, so
      // |u|, |v| < 26 m < 2^386 after the 25 rounds of a 381-bit modulus; one reduction at the end
      uint32_t nu0[N + 1], nv0[N + 1];
      words_lin_mont31<N>(u, f0, v, g0, mod, minv, nu0);
      words_lin_mont31<N>(u, f1, v, g1, mod, minv, nv0);
#pragma unroll
      for (int i = 0; i <= N; i++) {
        u[i] = nu0[i];
        v[i] = nv0[i];
      }
      continue;
    }
    // (u, v) <- ((u f0 + v g0) / 2^31, (u f1 + v g1) / 2^31) mod m
    uint32_t nu[2][N + 1];
#pragma unroll
    for (int side = 0; side < 2; side++) {
      const int64_t fu = side ? f1 : f0, fv = side ? g1 : g0;
      uint32_t t[N + 2];
      int64_t c = 0;
#pragma unroll
      for (int i = 0; i < N; i++) {
        const int64_t p1 = (int64_t)u[i] * fu, p2 = (int64_t)v[i] * fv;
        const int64_t sw = (int64_t)(uint32_t)p1 + (int64_t)(uint32_t)p2 + c;
        t[i] = (uint32_t)sw;
        c = (sw >> 32) + (p1 >> 32) + (p2 >> 32);
      }
      t[N] = (uint32_t)c;
      t[N + 1] = (uint32_t)(c >> 32);
      // + q m with q = -t mod^-1 mod 2^31: the sum is divisible by 2^31
      const uint64_t q = (uint64_t)((t[0] * minv) & 0x7fffffffu);
      uint64_t cc = 0;
#pragma unroll
      for (int i = 0; i < N; i++) {
        cc += (uint64_t)t[i] + q * mod[i];
        t[i] = (uint32_t)cc;
        cc >>= 32;
      }
#pragma unroll
      for (int i = N; i < N + 2; i++) {
        cc += (uint64_t)t[i];
        t[i] = (uint32_t)cc;
        cc >>= 32;
      }
      uint32_t w[N + 1];
#pragma unroll
      for (int i = 0; i <= N; i++) w[i] = (t[i] >> 31) | (t[i + 1] << 1);
      // |w| < 3m: bring into [0, m)
      for (int k = 0; k < 3 && (int32_t)w[N] < 0; k++) {
        uint64_t ac = 0;
#pragma unroll
        for (int i = 0; i < N; i++) {
          ac += (uint64_t)w[i] + mod[i];
          w[i] = (uint32_t)ac;
          ac >>= 32;
        }
        w[N] += (uint32_t)ac;
      }
      for (int k = 0; k < 3 && (w[N] != 0 || words_geq<N>(w, mod)); k++) {
        const uint32_t br = words_sub<N>(w, mod);
        w[N] -= br;
      }
#pragma unroll
      for (int i = 0; i <= N; i++) nu[side][i] = w[i];
    }
#pragma unroll
    for (int i = 0; i <= N; i++) {
      u[i] = nu[0][i];
      v[i] = nu[1][i];
    }
  }
  bool one = b[N] == 0 && words_is_one<N>(b);
  if (LAZY && one) {  // v signed, |v| < 26 m: into [0, m)
    while ((int32_t)v[N] < 0) {
      const uint32_t c = words_add<N>(v, mod);
      v[N] += c;
    }
    while (v[N] != 0 || words_geq<N>(v, mod)) {
      const uint32_t br = words_sub<N>(v, mod);
      v[N] -= br;
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++) out[i] = one ? v[i] : 0u;
}

}  // namespace hb
