// Grouped random-combination sums for the DIGIT forms of the scalars (gfx950): the tile sums of
// k_group_sum (k_rlc.hip) -- same tile records, same Jacobian tile sums, so k_group_join serves both --
// with an item's scalar read as short digits in the endomorphism basis (group_digits.hpp: X4, X2) and
// each pair of digits run as ONE joint double-and-add chain of 32 (G2), 96 (G1, X4) or 64 (G1, X2) steps.
// The scalars are public randomness and the points public inputs: variable time throughout.
//
// Exceptional additions inside an item's own chain.  The chain of (u, v) on the base B keeps
// acc = (U + V lambda) B with integers |U|, |V| <= 2^K (K <= 96 steps) and lambda = |x|^2 < 2^128; after
// the doubling of a step U and V are both even.  A table entry is (s + t lambda) B with (s, t) one of
// (1, 0), (0, -1), (1, -1).  acc = +-entry, or acc = O, would need
//     (U -+ s) + (V -+ t) lambda = 0 mod r.
// The left side is an integer of magnitude < 2^98 + 2^98 2^128 < r, so it would have to vanish as an
// integer, and with |U -+ s| < lambda that means U = +-s and V = +-t: both even, so s = t = 0, which is
// no entry.  acc = O happens only for U = V = 0 (the steps above the leading digit bits).  So within a
// chain an addition meets neither P + P nor P - P, only O + entry; jac_add_affine handles all three
// anyway.  (B is in the prime-order subgroup and not O: the ABI's contract, and items at infinity are
// skipped.)  Additions between items and between tiles use the complete jac_add.
#define HB_FP_LATENCY 1
#include <hip/hip_runtime.h>

#include "curve.hpp"
#include "endo.hpp"
#include "group_digits.hpp"
#include "group_plan.hpp"
#include "launch.hpp"

namespace hb {

// lambda (X, Y) = (k X, -Y) and B - lambda B = (k^2 X, -Y): the two scaled abscissae of a base
//   G1: [x^2] P = (beta X, -Y), k = beta.   G2: psi^2 (X, Y) = (beta^2 X, -Y), k = beta^2, k^2 = beta.
__device__ __forceinline__ void lambda_xs(const Fp& x, Fp& kx, Fp& k2x) {
  kx = fp_mul(x, fp_const(BETA_M));
  k2x = fp_mul(x, fp_const(FROB2_4_C0));  // beta^2
}
__device__ __forceinline__ void lambda_xs(const Fp2& x, Fp2& kx, Fp2& k2x) {
  const Fp b = fp_const(BETA_M), b2 = fp_const(FROB2_4_C0);
  kx = {fp_mul(x.c0, b2), fp_mul(x.c1, b2)};
  k2x = {fp_mul(x.c0, b), fp_mul(x.c1, b)};
}

__device__ __forceinline__ Fp fsel(bool c, const Fp& a, const Fp& b) {
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = c ? a.l[i] : b.l[i];
  return r;
}
__device__ __forceinline__ Fp2 fsel(bool c, const Fp2& a, const Fp2& b) { return {fsel(c, a.c0, b.c0), fsel(c, a.c1, b.c1)}; }

// u B + v lambda B for the recoded chain c of (u, v) on the affine base B = (x, y), `steps` joint
// double-and-add steps (wave-uniform: the count comes from the form, not from the digits)
template <class F>
__device__ Jac<F> joint_chain(const F& x, const F& y, const gd::Chain& c, int steps) {
  F kx, k2x;
  lambda_xs(x, kx, k2x);
  const F ny = fneg(y);
  Jac<F> acc = c.lead ? jac_from_affine(kx, ny, false) : jac_zero<F>();  // 2^steps lambda B after the doublings
  for (int i = steps - 1; i >= 0; i--) {
    acc = jac_dbl(acc);
    const int e = gd::entry(c, i);
    if (e) acc = jac_add_affine(acc, fsel(e == 1, x, fsel(e == 2, kx, k2x)), fsel(e == 3, ny, y));
  }
  return acc;
}

// Chain `digit` of an item under `form` (gd::FORM_X4 / FORM_X2)
template <class F>
struct DigitSplit;
template <>
struct DigitSplit<Fp2> {
  static constexpr int DIGITS = 2, WORDS = G2_WORDS;
  __device__ static Jac<Fp2> term(const uint32_t* w, const uint32_t* a, int digit, int /*form*/) {
    Fp2 x, y;
    bool inf;
    load_g2(w, x, y, inf);
    if (inf) return jac_zero<Fp2>();
    if (digit) {  // the base -psi(Q) = |x| Q
      x = psi_x(x);
      y = f2_neg(psi_y(y));
    }
    return joint_chain(x, y, gd::chain_x4_g2(a, digit), gd::steps_g2());
  }
};
template <>
struct DigitSplit<Fp> {
  static constexpr int DIGITS = 1, WORDS = G1_WORDS;
  __device__ static Jac<Fp> term(const uint32_t* w, const uint32_t* a, int /*digit*/, int form) {
    Fp x, y;
    bool inf;
    load_g1(w, x, y, inf);
    if (inf) return jac_zero<Fp>();
    return joint_chain(x, y, gd::chain_g1(form, a), gd::steps_g1(form));
  }
};

// The workgroup of k_group_sum: width * DIGITS threads per tile, width = 64 or 128 slots >= the call's
// longest tile; thread (digit d, slot i) = (t / width, t % width) runs chain d of item
// perm[tile_off + i] (a slot past the tile's length holds O), so the lanes of a wave run the same chain
// kind.  The partial sums go up an LDS tree of `width` entries (the chains of digit 1 are added into
// digit 0's registers first); thread 0 writes the tile's Jacobian sum.  Items at infinity contribute O.
template <class F>
__global__ void __launch_bounds__(256) k_group_digits(int ntile, int n, const uint32_t* __restrict__ pts,
                                                      const uint32_t* __restrict__ scalars,
                                                      const uint32_t* __restrict__ perm,
                                                      const uint32_t* __restrict__ tile_off,
                                                      const uint32_t* __restrict__ tile_len,
                                                      uint32_t* __restrict__ tile_out, int width, int form) {
  extern __shared__ unsigned char smem_raw[];
  Jac<F>* sm = reinterpret_cast<Jac<F>*>(smem_raw);
  using S = DigitSplit<F>;
  const int T = width;
  const int tile = blockIdx.x;
  if (tile >= ntile) return;  // uniform per workgroup
  const int t = threadIdx.x, digit = t / T, slot = t % T;
  const uint32_t len = tile_len[tile] < (uint32_t)T ? tile_len[tile] : (uint32_t)T;
  Jac<F> acc = jac_zero<F>();
  if ((uint32_t)slot < len && digit < S::DIGITS) {
    const uint32_t pos = tile_off[tile] + slot;
    const uint32_t item = pos < (uint32_t)n ? perm[pos] : 0xffffffffu;
    if (item < (uint32_t)n) {
      uint32_t a[4];
      for (int j = 0; j < 4; j++) a[j] = scalars[(size_t)item * 4 + j];
      acc = S::term(pts + (size_t)item * S::WORDS, a, digit, form);
    }
  }
  if (S::DIGITS > 1) {
    if (digit == 1) sm[slot] = acc;
    __syncthreads();
    if (digit == 0) acc = jac_add(acc, sm[slot]);
    __syncthreads();
  }
  if (digit == 0) sm[slot] = acc;
  __syncthreads();
  for (int s = T / 2; s > 0; s >>= 1) {
    if (t < s) sm[t] = jac_add(sm[t], sm[t + s]);
    __syncthreads();
  }
  if (t == 0) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&sm[0]);
    uint32_t* dst = tile_out + (size_t)tile * (sizeof(Jac<F>) / 4);
    for (int i = 0; i < (int)(sizeof(Jac<F>) / 4); i++) dst[i] = src[i];
  }
}

// The per-item G1 scaling of the batched checks: out[i] = r_i P_i for X4 digits, the G1 chain of
// k_group_digits (96 joint steps) with one chain -- one lane -- per item and an affine ABI point out
// (all-zero for P_i = O).  64-thread workgroups: a call of 10,100 items still spreads over 158 CUs.
__global__ void __launch_bounds__(64) k_scale_digits_g1(int n, const uint32_t* __restrict__ pts,
                                                        const uint32_t* __restrict__ scalars,
                                                        uint32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t a[4];
  for (int j = 0; j < 4; j++) a[j] = scalars[(size_t)i * 4 + j];
  const Jac<Fp> acc = DigitSplit<Fp>::term(pts + (size_t)i * G1_WORDS, a, 0, gd::FORM_X4);
  g1_jac_to_words(acc, out + (size_t)i * G1_WORDS);
}

}  // namespace hb

namespace hbl {

hipError_t scale_digits_g1(hipStream_t s, int n, const void* pts, const uint32_t* scalars, void* out) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(hb::k_scale_digits_g1, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, n, (const uint32_t*)pts,
                     scalars, (uint32_t*)out);
  return hipGetLastError();
}

template <class F>
static hipError_t group_digits(hipStream_t s, int form, int ntile, int n, int max_len, const void* pts,
                               const uint32_t* scalars, const uint32_t* perm, const uint32_t* tile_off,
                               const uint32_t* tile_len, void* tile_sums) {
  if (ntile <= 0) return hipSuccess;
  static_assert(GROUP_TILE * hb::DigitSplit<F>::DIGITS <= 256 && GROUP_TILE >= 64 && (GROUP_TILE & (GROUP_TILE - 1)) == 0,
                "a tile's chains fit one 256-thread workgroup; the LDS tree halves a power of two");
  if (max_len < 1 || max_len > (int)GROUP_TILE) return hipErrorInvalidValue;
  int width = 64;  // whole waves, a power of two for the tree
  while (width < max_len) width *= 2;
  hipLaunchKernelGGL(hb::k_group_digits<F>, dim3((unsigned)ntile), dim3(width * hb::DigitSplit<F>::DIGITS),
                     width * sizeof(hb::Jac<F>), s, ntile, n, (const uint32_t*)pts, scalars, perm, tile_off, tile_len,
                     (uint32_t*)tile_sums, width, form);
  return hipGetLastError();
}

hipError_t group_digits_g1(hipStream_t s, int form, int ntile, int n, int max_len, const void* pts,
                           const uint32_t* scalars, const uint32_t* perm, const uint32_t* tile_off,
                           const uint32_t* tile_len, void* tile_sums) {
  if (form != gd::FORM_X4 && form != gd::FORM_X2) return hipErrorInvalidValue;
  return group_digits<hb::Fp>(s, form, ntile, n, max_len, pts, scalars, perm, tile_off, tile_len, tile_sums);
}
hipError_t group_digits_g2(hipStream_t s, int form, int ntile, int n, int max_len, const void* pts,
                           const uint32_t* scalars, const uint32_t* perm, const uint32_t* tile_off,
                           const uint32_t* tile_len, void* tile_sums) {
  if (form != gd::FORM_X4) return hipErrorInvalidValue;  // no call sums G2 points under X2
  return group_digits<hb::Fp2>(s, form, ntile, n, max_len, pts, scalars, perm, tile_off, tile_len, tile_sums);
}

}  // namespace hbl
