// Host Fr (4 x 64-bit Montgomery, R = 2^256) for the Lagrange digits of one or two combines: on the
// host they cost tens of microseconds, less than a kernel launch of k_interp_digits.  No HIP here:
// tests/native/engine_host_test.cpp compiles this header for the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/hbbft_hip.h"

struct HFr {
  uint64_t l[4];
};
constexpr uint64_t HFR_P[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull,
                               0x73eda753299d7d48ull};
constexpr uint64_t HFR_NP = 0xfffffffeffffffffull;  // -r^-1 mod 2^64
constexpr uint64_t HFR_R2[4] = {0xc999e990f3f29c6dull, 0x2b6cedcb87925c23ull, 0x05d314967254398full,
                                0x0748d9d99f59ff11ull};
// the BLS parameter |x| (base of the GLS digits) and x^2 (base of the G1 digits), as 64-bit words
constexpr uint64_t XA = 0xd201000000010000ull;
constexpr uint64_t X2_LO = 0x0000000100000000ull, X2_HI = 0xac45a4010001a402ull;
using u128 = unsigned __int128;

inline bool hfr_geq_p(const uint64_t* a) {
  for (int i = 3; i >= 0; i--)
    if (a[i] != HFR_P[i]) return a[i] > HFR_P[i];
  return true;
}
inline void hfr_sub_p(uint64_t* a) {
  u128 br = 0;
  for (int i = 0; i < 4; i++) {
    const u128 d = (u128)a[i] - HFR_P[i] - br;
    a[i] = (uint64_t)d;
    br = (d >> 64) ? 1 : 0;
  }
}
inline HFr hfr_mul(const HFr& a, const HFr& b) {  // CIOS
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    u128 c = 0;
    for (int j = 0; j < 4; j++) {
      c += (u128)a.l[j] * b.l[i] + t[j];
      t[j] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[4] = (uint64_t)c;
    t[5] = (uint64_t)(c >> 64);
    const uint64_t m = t[0] * HFR_NP;
    c = (u128)m * HFR_P[0] + t[0];
    c >>= 64;
    for (int j = 1; j < 4; j++) {
      c += (u128)m * HFR_P[j] + t[j];
      t[j - 1] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[3] = (uint64_t)c;
    t[4] = t[5] + (uint64_t)(c >> 64);
  }
  HFr r{{t[0], t[1], t[2], t[3]}};
  if (t[4] || hfr_geq_p(r.l)) hfr_sub_p(r.l);
  return r;
}
inline HFr hfr_from_u64(uint64_t v) {
  return hfr_mul(HFr{{v, 0, 0, 0}}, HFr{{HFR_R2[0], HFR_R2[1], HFR_R2[2], HFR_R2[3]}});
}
inline HFr hfr_sub(const HFr& a, const HFr& b) {
  HFr r;
  u128 br = 0;
  for (int i = 0; i < 4; i++) {
    const u128 d = (u128)a.l[i] - b.l[i] - br;
    r.l[i] = (uint64_t)d;
    br = (d >> 64) ? 1 : 0;
  }
  if (br) {
    u128 c = 0;
    for (int i = 0; i < 4; i++) {
      c += (u128)r.l[i] + HFR_P[i];
      r.l[i] = (uint64_t)c;
      c >>= 64;
    }
  }
  return r;
}
inline bool hfr_is_zero(const HFr& a) { return !(a.l[0] | a.l[1] | a.l[2] | a.l[3]); }
inline HFr hfr_inv(const HFr& a) {  // a^(r-2)
  uint64_t e[4] = {HFR_P[0] - 2, HFR_P[1], HFR_P[2], HFR_P[3]};
  HFr r = hfr_from_u64(1);
  for (int i = 255; i >= 0; i--) {
    r = hfr_mul(r, r);
    if ((e[i >> 6] >> (i & 63)) & 1) r = hfr_mul(r, a);
  }
  return r;
}
inline void hfr_to_canon(const HFr& a, uint64_t* out) {
  const HFr c = hfr_mul(a, HFr{{1, 0, 0, 0}});
  for (int i = 0; i < 4; i++) out[i] = c.l[i];
}

// q (4 x u64) <- q / x^2, rem <- q mod x^2 (bit-serial, the host twin of k_curve.hip div_x2)
inline void host_div_x2(uint64_t q[4], uint64_t rem[2]) {
  uint64_t r0 = 0, r1 = 0;
  for (int w = 3; w >= 0; w--) {
    uint64_t qw = 0;
    for (int b = 63; b >= 0; b--) {
      const bool top = (r1 >> 63) != 0;
      r1 = (r1 << 1) | (r0 >> 63);
      r0 = (r0 << 1) | ((q[w] >> b) & 1);
      const bool ge = top || r1 > X2_HI || (r1 == X2_HI && r0 >= X2_LO);
      if (ge) {
        const uint64_t nr0 = r0 - X2_LO;
        r1 = r1 - X2_HI - (r0 < X2_LO ? 1 : 0);
        r0 = nr0;
      }
      qw |= (uint64_t)ge << b;
    }
    q[w] = qw;
  }
  rem[0] = r0;
  rem[1] = r1;
}

// lambda_k(0) = prod_{j != k} x_j / (x_j - x_k) of every sample of each combine, canonical (4 x u64
// LE per sample); status[c] = HBH_ERR_DUPLICATE_ENTRY and zero lambdas on a repeated x
inline void host_lagrange(const uint32_t* xs, size_t ncomb, size_t m, uint64_t* lam, int* status) {
  std::vector<HFr> x(m), num(m), den(m), pre(m);
  for (size_t c = 0; c < ncomb; c++) {
    const uint32_t* cx = xs + c * m;
    for (size_t k = 0; k < m; k++) x[k] = hfr_from_u64(cx[k]);
    bool dup = false;
    for (size_t k = 0; k < m; k++) {
      HFr n = hfr_from_u64(1), d = hfr_from_u64(1);
      for (size_t j = 0; j < m; j++) {
        if (j == k) continue;
        n = hfr_mul(n, x[j]);
        d = hfr_mul(d, hfr_sub(x[j], x[k]));
      }
      dup = dup || hfr_is_zero(d);
      num[k] = n;
      den[k] = d;
    }
    status[c] = dup ? HBH_ERR_DUPLICATE_ENTRY : HBH_OK;
    uint64_t* lc = lam + c * m * 4;
    if (dup) {
      std::memset(lc, 0, m * 4 * sizeof(uint64_t));
      continue;
    }
    pre[0] = den[0];
    for (size_t k = 1; k < m; k++) pre[k] = hfr_mul(pre[k - 1], den[k]);
    HFr inv = hfr_inv(pre[m - 1]);
    for (size_t k = m; k-- > 0;) {
      const HFr ik = k ? hfr_mul(inv, pre[k - 1]) : inv;
      if (k) inv = hfr_mul(inv, den[k]);
      hfr_to_canon(hfr_mul(num[k], ik), lc + k * 4);
    }
  }
}

// the four GLS digits (base |x|) of n canonical scalars (4 x u64 each): q <- q / |x| three times, digit j
// = remainder, digit 3 = the last quotient.  dg may be lam (each scalar is read before its digits are
// written).
inline void host_gls_digits(const uint64_t* lam, size_t n, uint64_t* dg) {
  for (size_t k = 0; k < n; k++) {
    uint64_t q[4] = {lam[k * 4], lam[k * 4 + 1], lam[k * 4 + 2], lam[k * 4 + 3]};
    for (int j = 0; j < 3; j++) {
      u128 rem = 0;
      for (int w = 3; w >= 0; w--) {
        const u128 cur = (rem << 64) | q[w];
        q[w] = (uint64_t)(cur / XA);
        rem = cur % XA;
      }
      dg[k * 4 + j] = (uint64_t)rem;
    }
    dg[k * 4 + 3] = q[0];
  }
}

// k_interp_digits on the host: the four GLS digits (base |x|) of every lambda_k(0) of each combine,
// or with g1 its two 128-bit digits base x^2; status[c] = HBH_ERR_DUPLICATE_ENTRY and zero digits on
// a repeated x
inline void host_interp_digits(const uint32_t* xs, size_t ncomb, size_t m, uint64_t* digits, int* status,
                               bool g1 = false) {
  host_lagrange(xs, ncomb, m, digits, status);  // in place: lambda_k's 4 words become its 4 digits
  for (size_t c = 0; c < ncomb; c++) {
    uint64_t* dg = digits + c * m * 4;
    if (status[c] != HBH_OK) continue;
    if (!g1) {
      host_gls_digits(dg, m, dg);
      continue;
    }
    for (size_t k = 0; k < m; k++) {  // lambda = d0 + d1 x^2
      uint64_t q[4] = {dg[k * 4], dg[k * 4 + 1], dg[k * 4 + 2], dg[k * 4 + 3]};
      uint64_t rem[2];
      host_div_x2(q, rem);
      dg[k * 4 + 0] = rem[0];
      dg[k * 4 + 1] = rem[1];
      dg[k * 4 + 2] = q[0];
      dg[k * 4 + 3] = q[1];
    }
  }
}
