// Latency form of the G2 Lagrange combine (PublicKeySet::combine_signatures,
// src/threshold_sign.rs:249-259, for the one document of combine_and_verify_sig): the curve work of
// k_interp_endo on LANE QUADS.  Two lanes hold the c0 / c1 components of every Fp2 coordinate
// (pfp.hpp), so each Fp2 product is one lane-pair product; two lane pairs (a quad) hold the same
// point and split each group operation's independent products between them, trading results with
// one DPP quad permute per limb: a doubling is 4 product rounds instead of 7 serial products, a
// mixed addition 6 instead of 11, a general addition 9 instead of 16.  The work split is the one
// of k_interp_endo: term (k, j) = digit chunk s of GLS digit j of lambda_k(0) times psi^j(P_k)
// (sign (-1)^j), 32-bit chunks, one quad per (chunk, term).  One workgroup per (combine, chunk,
// half of the terms): an LDS tree sums its terms, the chunk-1 workgroups scale their sums by 2^32
// (Horner), and k_interp_join adds the four partial sums and writes the affine result.  Formulas:
// dbl-2009-l, add-2007-bl, madd-2007-bl (curve.hpp) -- the same group law, so the affine output is
// byte-identical to the C oracle's.  Digits come from the host or k_interp_digits (k_curve.hip).
#define HS_MULFN static __device__ __noinline__
#include "g2quad.hpp"
#include "interp_pair.hpp"
#include "launch.hpp"
#include "pfp.hpp"
#include "words.hpp"

namespace hbs {

constexpr int IP_THREADS = 256;          // one workgroup per (combine, chunk, half): 64 lane quads
constexpr int IP_NCHUNK = 2;             // 32-bit chunks of the 64-bit digits
constexpr int IP_NHALF = 2;              // workgroups per chunk (terms interleaved between them)
constexpr int IP_WG = IP_NCHUNK * IP_NHALF;
constexpr int IP_Q = IP_THREADS / 4;     // lane quads per workgroup (power of two)
constexpr int IP_WORDS = 3 * NL;         // one lane's Jacobian point (x, y, z own components)

// k * (x, y) for a 32-bit k, double-and-add from the top set bit (jac_mul_affine)
HP_D HJac qj_mul_affine(const Fp& x, const Fp& y, bool inf, uint32_t k) {
  if (inf || k == 0) return hj_zero();
  const int top = 31 - __builtin_clz(k);
  return dbl_and_add(HJac{x, y, h_one()}, k, top - 1, [](const HJac& a) HS_LAMBDA { return qj_dbl(a); },
                     [&](const HJac& a) HS_LAMBDA { return qj_add_affine(a, x, y); });
}

// psi on own components: psi(x) = conj(x) * (0 + c u) -> (x1 c, x0 c); psi(y) = conj(y) * c2
HP_D Fp psi_xh(const Fp& x) { return fp_reduce(fp_mul(dpp_fp<DPP_SWAP>(x), fp_const(hb::PSI_C1_C1))); }
HP_D Fp psi_yh(const Fp& y) { return fp_reduce(h_mul(h_conj(y), h_const(hb::PSI_C2_C0, hb::PSI_C2_C1))); }

HP_D void lds_put(uint32_t* s, const HJac& p) {
#pragma unroll
  for (int i = 0; i < NL; i++) {
    s[i] = (uint32_t)p.x.l[i];
    s[NL + i] = (uint32_t)p.y.l[i];
    s[2 * NL + i] = (uint32_t)p.z.l[i];
  }
}
HP_D HJac lds_get(const uint32_t* s) {
  HJac p;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    p.x.l[i] = (int32_t)s[i];
    p.y.l[i] = (int32_t)s[NL + i];
    p.z.l[i] = (int32_t)s[2 * NL + i];
  }
  return p;
}

// Workgroup (c, chunk, half): every other term of the chunk on 64 lane quads (4 waves, one per
// SIMD), an LDS tree, then quad 0 scales a chunk-1 sum by 2^32 (Horner) and writes the partial sum.
__global__ void __launch_bounds__(IP_THREADS) k_interp_pair(int ncomb, int m, const uint64_t* __restrict__ digits,
                                                            const uint32_t* __restrict__ pts, int32_t* __restrict__ part) {
  extern __shared__ uint32_t sm[];  // IP_Q quads x 2 lanes x IP_WORDS
  const int c = blockIdx.x / IP_WG, chunk = (blockIdx.x / IP_NHALF) % IP_NCHUNK, half = blockIdx.x % IP_NHALF;
  if (c >= ncomb) return;  // uniform per workgroup
  const int g = threadIdx.x >> 2, h = threadIdx.x & 1;
  HJac acc = hj_zero();
  for (int t = half + IP_NHALF * g; t < m * 4; t += IP_NHALF * IP_Q) {
    const int k = t >> 2, j = t & 3;
    const uint32_t* w = pts + ((size_t)c * m + k) * 48;
    const bool inf = lp_both(words_zero(w + (lp_even() ? 0 : 12), 12) && words_zero(w + (lp_even() ? 24 : 36), 12));
    Fp x, y;
    h_g2_load(w, x, y);
    for (int s = 0; s < j; s++) {
      x = psi_xh(x);
      y = psi_yh(y);
    }
    if (j & 1) y = fp_neg(y);
    const uint64_t d = digits[((size_t)c * m + k) * 4 + j];
    const uint32_t kc = (uint32_t)(d >> (32 * chunk));
    acc = qj_add(acc, qj_mul_affine(x, y, inf, kc));
  }
  uint32_t* mine = sm + (size_t)(g * 2 + h) * IP_WORDS;
  if (!q_hi()) lds_put(mine, acc);
  __syncthreads();
  for (int s = IP_Q / 2; s > 0; s >>= 1) {
    if (g < s) {
      acc = qj_add(lds_get(mine), lds_get(sm + (size_t)((g + s) * 2 + h) * IP_WORDS));
    }
    __syncthreads();
    if (g < s && !q_hi()) lds_put(mine, acc);
    __syncthreads();
  }
  if (g != 0) return;
  HJac r = lds_get(sm + (size_t)h * IP_WORDS);
  if (chunk == 1) {
#pragma unroll 1
    for (int b = 0; b < 32; b++) r = qj_dbl(r);
  }
  if (!q_hi()) lds_put((uint32_t*)part + ((size_t)blockIdx.x * 2 + h) * IP_WORDS, r);
}

// out[c] = affine(sum of the four partial sums): one lane quad per combine
__global__ void __launch_bounds__(64) k_interp_join(int ncomb, const int32_t* __restrict__ part,
                                                    uint32_t* __restrict__ out) {
  const int c = (int)((blockIdx.x * 64u + threadIdx.x) >> 2);
  if (c >= ncomb) return;
  const int h = threadIdx.x & 1;
  const uint32_t* p = (const uint32_t*)part + (size_t)c * IP_WG * 2 * IP_WORDS;
  HJac s1 = qj_add(lds_get(p + (size_t)(2 * 2 + h) * IP_WORDS), lds_get(p + (size_t)(3 * 2 + h) * IP_WORDS));
  HJac s0 = qj_add(lds_get(p + (size_t)(0 * 2 + h) * IP_WORDS), lds_get(p + (size_t)(1 * 2 + h) * IP_WORDS));
  HJac r = qj_add(s1, s0);
  uint32_t* o = out + (size_t)c * 48 + (lp_even() ? 0 : 12);
  if (hj_is_zero(r)) {
    if (!q_hi()) {
#pragma unroll
      for (int i = 0; i < 12; i++) {
        o[i] = 0u;
        o[24 + i] = 0u;
      }
    }
    return;
  }
  const Fp zi = h_inv_vartime(fp_reduce(r.z));
  const Fp zi2 = h_sqr(zi);
  Fp xa, zi3;
  h_mul2(r.x, zi2, zi2, zi, xa, zi3);
  const Fp ya = h_mul(r.y, zi3);
  if (!q_hi()) {
    fp_to_words(xa, o);
    fp_to_words(ya, o + 24);
  }
}

}  // namespace hbs

namespace hbl {

bool interp_g2_pair_fits(int m) { return m >= 1 && m <= 512; }

size_t interp_g2_pair_part_bytes(int ncomb) { return (size_t)ncomb * hbs::IP_WG * 2 * hbs::IP_WORDS * 4; }

hipError_t interp_g2_pair(hipStream_t s, int ncomb, int m, const uint64_t* digits, const void* pts, void* part,
                          void* out) {
  if (ncomb <= 0) return hipSuccess;
  const size_t lds = (size_t)hbs::IP_Q * 2 * hbs::IP_WORDS * 4;
  hipLaunchKernelGGL(hbs::k_interp_pair, dim3((unsigned)ncomb * hbs::IP_WG), dim3(hbs::IP_THREADS), lds, s, ncomb, m,
                     digits, (const uint32_t*)pts, (int32_t*)part);
  hipLaunchKernelGGL(hbs::k_interp_join, dim3((unsigned)((4 * ncomb + 63) / 64)), dim3(64), 0, s, ncomb,
                     (const int32_t*)part, (uint32_t*)out);
  return hipGetLastError();
}

}  // namespace hbl
