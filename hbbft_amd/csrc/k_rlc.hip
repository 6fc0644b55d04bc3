// Grouped random-combination sums (gfx950): sum_i r_i P_i over the items of a group, r_i < 2^128, for
// the opt-in share checks hbh_verify_*_shares_grouped.  k_group_sum sums one tile of a group per
// workgroup, k_group_join adds a group's tile sums and writes the affine ABI point.  The scalars are
// public randomness and the points public inputs: variable time throughout (the variable-time Fp
// inverse of fp.hpp for the single-thread affine outputs).  Host launchers at the bottom.
#define HB_FP_LATENCY 1
#include <hip/hip_runtime.h>

#include "curve.hpp"
#include "endo.hpp"
#include "group_plan.hpp"
#include "launch.hpp"

namespace hb {

// A Jacobian point as raw limbs (the device representation, between the two kernels only)
template <class F>
struct JacWords {
  static constexpr int N = sizeof(Jac<F>) / 4;
};
template <class F>
__device__ __forceinline__ void jac_put(uint32_t* __restrict__ w, const Jac<F>& p) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&p);
#pragma unroll
  for (int i = 0; i < JacWords<F>::N; i++) w[i] = src[i];
}
template <class F>
__device__ __forceinline__ Jac<F> jac_get(const uint32_t* __restrict__ w) {
  Jac<F> p;
  uint32_t* dst = reinterpret_cast<uint32_t*>(&p);
#pragma unroll
  for (int i = 0; i < JacWords<F>::N; i++) dst[i] = w[i];
  return p;
}

// Chain `digit` of item scalar r (4 LE words, < 2^128) on point w:
//   G2 (2 chains): r = d0 + d1 |x| + d2 |x|^2 in base |x| (d0, d1 < |x| < 2^64, d2 <= 1 since
//       |x|^2 > 2^127); psi = [x] = [-|x|] on G2, so r P = d0 P + d1 (-psi(P)) + d2 psi^2(P).  Chain 0
//       is d0 P; chain 1 is d1 (-psi(P)) and, for the scalars >= |x|^2, one addition of psi^2(P).
//   G1 (1 chain): r P with r as a plain 128-bit integer.  The GLV split (div_x2) would cut only the
//       scalars >= x^2 > 2^127 and leave every other chain at its length, so it is not used.
template <class F>
struct GroupSplit;
template <>
struct GroupSplit<Fp2> {
  static constexpr int DIGITS = 2, WORDS = G2_WORDS;
  __device__ static Jac<Fp2> term(const uint32_t* w, const uint32_t* r, int digit) {
    Fp2 x, y;
    bool inf;
    load_g2(w, x, y, inf);
    if (inf) return jac_zero<Fp2>();
    uint64_t q[4] = {(uint64_t)r[0] | ((uint64_t)r[1] << 32), (uint64_t)r[2] | ((uint64_t)r[3] << 32), 0, 0};
    const uint64_t d0 = div_x_abs(q);
    const uint64_t d1 = div_x_abs(q);  // q[0] is now d2 <= 1
    const uint64_t d = digit ? d1 : d0;
    if (digit) {  // the base -psi(P)
      x = psi_x(x);
      y = f2_neg(psi_y(y));
    }
    const uint32_t kk[8] = {(uint32_t)d, (uint32_t)(d >> 32), 0, 0, 0, 0, 0, 0};
    Jac<Fp2> acc = jac_mul_affine(x, y, false, kk);
    if (digit && q[0]) acc = jac_add_affine(acc, psi_x(x), f2_neg(psi_y(y)));  // psi^2(P) = -psi(-psi(P))
    return acc;
  }
  __device__ static void store(const Jac<Fp2>& p, uint32_t* out) { g2_jac_to_words(p, out); }
};
template <>
struct GroupSplit<Fp> {
  static constexpr int DIGITS = 1, WORDS = G1_WORDS;
  __device__ static Jac<Fp> term(const uint32_t* w, const uint32_t* r, int /*digit*/) {
    Fp x, y;
    bool inf;
    load_g1(w, x, y, inf);
    const uint32_t kk[8] = {r[0], r[1], r[2], r[3], 0, 0, 0, 0};
    return jac_mul_affine(x, y, inf, kk);
  }
  __device__ static void store(const Jac<Fp>& p, uint32_t* out) { g1_jac_to_words(p, out); }
};

// One workgroup of width * DIGITS threads per tile, width = 64 or 128 slots >= the call's longest tile
// (a call of 64-share documents runs two waves per tile, none of them idle): thread (digit d, slot i) =
// (t / width, t % width) runs chain d of item perm[tile_off + i] (a slot past the tile's length holds
// O), so the lanes of a wave run the same chain kind.  The partial sums go up an LDS tree of `width`
// entries (the chains of digit 1 are added into digit 0's registers first); thread 0 writes the tile's
// Jacobian sum.  Items at infinity contribute O.
template <class F>
__global__ void __launch_bounds__(256) k_group_sum(int ntile, int n, const uint32_t* __restrict__ pts,
                                                   const uint32_t* __restrict__ scalars,
                                                   const uint32_t* __restrict__ perm,
                                                   const uint32_t* __restrict__ tile_off,
                                                   const uint32_t* __restrict__ tile_len,
                                                   uint32_t* __restrict__ tile_out, int width) {
  extern __shared__ unsigned char smem_raw[];
  Jac<F>* sm = reinterpret_cast<Jac<F>*>(smem_raw);
  using S = GroupSplit<F>;
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
      uint32_t r[4];
      for (int j = 0; j < 4; j++) r[j] = scalars[(size_t)item * 4 + j];
      acc = S::term(pts + (size_t)item * S::WORDS, r, digit);
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
  if (t == 0) jac_put<F>(tile_out + (size_t)tile * JacWords<F>::N, sm[0]);
}

// One thread per combined group: the sum of its tiles [ctile[c], ctile[c + 1]) as the affine ABI point
// (all-zero when the sum is O).
template <class F>
__global__ void __launch_bounds__(64) k_group_join(int ngroup, const uint32_t* __restrict__ ctile,
                                                   const uint32_t* __restrict__ tile_sums, uint32_t* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ngroup) return;
  Jac<F> acc = jac_zero<F>();
  for (uint32_t k = ctile[c]; k < ctile[c + 1]; k++) acc = jac_add(acc, jac_get<F>(tile_sums + (size_t)k * JacWords<F>::N));
  GroupSplit<F>::store(acc, out + (size_t)c * GroupSplit<F>::WORDS);
}

}  // namespace hb

namespace hbl {

template <class F>
static hipError_t group_sum(hipStream_t s, int ntile, int n, int max_len, const void* pts, const uint32_t* scalars,
                            const uint32_t* perm, const uint32_t* tile_off, const uint32_t* tile_len, void* tile_sums) {
  if (ntile <= 0) return hipSuccess;
  static_assert(GROUP_TILE * hb::GroupSplit<F>::DIGITS <= 256 && GROUP_TILE >= 64 && (GROUP_TILE & (GROUP_TILE - 1)) == 0,
                "a tile's chains fit one 256-thread workgroup; the LDS tree halves a power of two");
  if (max_len < 1 || max_len > (int)GROUP_TILE) return hipErrorInvalidValue;
  int width = 64;  // whole waves, a power of two for the tree
  while (width < max_len) width *= 2;
  hipLaunchKernelGGL(hb::k_group_sum<F>, dim3((unsigned)ntile), dim3(width * hb::GroupSplit<F>::DIGITS),
                     width * sizeof(hb::Jac<F>), s, ntile, n, (const uint32_t*)pts, scalars, perm, tile_off, tile_len,
                     (uint32_t*)tile_sums, width);
  return hipGetLastError();
}
template <class F>
static hipError_t group_join(hipStream_t s, int ngroup, const uint32_t* ctile, const void* tile_sums, void* out) {
  if (ngroup <= 0) return hipSuccess;
  hipLaunchKernelGGL(hb::k_group_join<F>, dim3((unsigned)((ngroup + 63) / 64)), dim3(64), 0, s, ngroup, ctile,
                     (const uint32_t*)tile_sums, (uint32_t*)out);
  return hipGetLastError();
}

size_t group_tile_bytes(bool g2) { return g2 ? sizeof(hb::Jac<hb::Fp2>) : sizeof(hb::Jac<hb::Fp>); }
hipError_t group_sum_g1(hipStream_t s, int ntile, int n, int max_len, const void* pts, const uint32_t* scalars,
                        const uint32_t* perm, const uint32_t* tile_off, const uint32_t* tile_len, void* tile_sums) {
  return group_sum<hb::Fp>(s, ntile, n, max_len, pts, scalars, perm, tile_off, tile_len, tile_sums);
}
hipError_t group_sum_g2(hipStream_t s, int ntile, int n, int max_len, const void* pts, const uint32_t* scalars,
                        const uint32_t* perm, const uint32_t* tile_off, const uint32_t* tile_len, void* tile_sums) {
  return group_sum<hb::Fp2>(s, ntile, n, max_len, pts, scalars, perm, tile_off, tile_len, tile_sums);
}
hipError_t group_join_g1(hipStream_t s, int ngroup, const uint32_t* ctile, const void* tile_sums, void* out) {
  return group_join<hb::Fp>(s, ngroup, ctile, tile_sums, out);
}
hipError_t group_join_g2(hipStream_t s, int ngroup, const uint32_t* ctile, const void* tile_sums, void* out) {
  return group_join<hb::Fp2>(s, ngroup, ctile, tile_sums, out);
}

}  // namespace hbl
