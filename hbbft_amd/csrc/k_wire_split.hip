// Latency form of the point decoders of k_wire.hip (HBH_DEC_SPLIT): the same two roles per
// workgroup and the same LDS hand-off, but the subgroup role -- the longer serial chain of the
// throughput form -- runs on LANE QUADS: four lanes cooperate on one point's [|x|] chain(s) with the
// group law of g1quad.hpp (a doubling in 3 product rounds instead of 7 serial products, an addition
// in 5 instead of 11 / 16) and g2quad.hpp (4 instead of 7, 6 instead of 11).  The root role is the
// code of the throughput form (wire_root.hpp), one lane per point, so the bytes are the same; the
// subgroup verdict is the same equality of points (criteria and the isomorphic point P' = (rhs x,
// rhs^2): see k_wire.hip), evaluated on the signed-limb Fp of sfp.hpp.  Both fields use radix 2^28
// and R = 2^392, so N(y) crosses the LDS as its 14 limbs.
//
// A workgroup decodes WS_POINTS = 16 points on 80 threads: wave 0 is 16 lane quads (subgroup role),
// wave 1 holds 16 root lanes.  4,096 points are 256 workgroups, one per CU, every wave on a SIMD of
// its own, so the time of a small batch is the longer role's chain: G1 428 product rounds against
// the root's 467 products, G2 282 lane-pair rounds against the root's two dependent (p - 3) / 4
// chains (workcount.py).  G2 takes quads, not pairs: a lane-pair product is 1.5 Fp products of
// multiply-adds, which would put the pair form's 496 rounds within a fifth of the root.
//
// Lock-step: every branch a subgroup lane takes depends only on its point (flags, x, the chain's
// values -- identical in the four lanes), never on the lane's place in the quad, so DPP source
// lanes are always active; a dead slot (i >= n) reads as a rejected encoding and its whole quad
// skips the chain; no lane leaves before the last barrier.
#define HS_MULFN static __device__ __noinline__
#include <hip/hip_runtime.h>

#include "wire_root.hpp"
#include "g1quad.hpp"
#include "g2quad.hpp"

namespace hbw {

constexpr int WS_POINTS = 16;                // points per workgroup
constexpr int WS_THREADS = 64 + WS_POINTS;   // one wave of lane quads + the root lanes

// x < p for canonical words
__device__ __forceinline__ bool below_p(const uint32_t* x) {
  uint32_t p[12];
  for (int k = 0; k < 12; k++) p[k] = hb::PM2_W[k];
  p[0] += 2;
  return hb::words_gt(p, x, 12);
}

// [|x|] P for the quad's affine P (not infinity): one mixed addition per set bit
__device__ __forceinline__ hbs::QJ g1q_mul_absx_affine(const hbs::Fp& x, const hbs::Fp& y) {
  return hbs::dbl_and_add(hbs::QJ{x, y, hbs::fp_one()}, hb::X_ABS, 62,
                          [](const hbs::QJ& a) HS_LAMBDA { return hbs::g1q_dbl(a); },
                          [&](const hbs::QJ& a) HS_LAMBDA { return hbs::g1q_add_affine(a, x, y); });
}
__device__ __forceinline__ hbs::QJ g1q_mul_absx(const hbs::QJ& p) {
  return hbs::dbl_and_add(p, hb::X_ABS, 62, [](const hbs::QJ& a) HS_LAMBDA { return hbs::g1q_dbl(a); },
                          [&](const hbs::QJ& a) HS_LAMBDA { return hbs::g1q_add(a, p); });
}

// The G1 criterion on P' = (rhs x, rhs^2): [|x|]([|x|] P') == (beta X, -Y).  xw: canonical x < p.
__device__ __forceinline__ bool g1q_in_subgroup(const uint32_t* xw) {
  using namespace hbs;
  const Fp xm = fp_from_words(xw);
  const Fp rhs = fp_add(fp_mul(fp_sqr(xm), xm), fp_const(hb::B1_M));
  Fp X, Y;
  q2(rhs, xm, rhs, rhs, X, Y);
  const QJ q = g1q_mul_absx(g1q_mul_absx_affine(X, Y));
  if (qj_zero(q)) return false;
  Fp z2, bx, tx, z3;
  q2(q.z, q.z, X, fp_const(hb::BETA_M), z2, bx);
  q2(bx, z2, z2, q.z, tx, z3);
  if (!fp_is_zero(fp_sub(q.x, tx))) return false;
  return fp_is_zero(fp_add(q.y, fp_mul(Y, z3)));
}

__global__ void __launch_bounds__(WS_THREADS) k_g1_decompress_split(int n, const uint32_t* __restrict__ xw,
                                                                     const uint8_t* __restrict__ flags,
                                                                     uint32_t* __restrict__ out,
                                                                     uint8_t* __restrict__ ok) {
  __shared__ uint8_t in_group[WS_POINTS];
  const int role = threadIdx.x >> 6;  // 0: subgroup test, four lanes per point; 1: square root, one lane
  const int slot = role == 0 ? (int)(threadIdx.x >> 2) : (int)threadIdx.x - 64;
  const int i = blockIdx.x * WS_POINTS + slot;
  const bool live = i < n;
  const uint8_t f = live ? flags[i] : hbl::WIRE_REJECT;
  uint32_t x[12];
  for (int k = 0; k < 12; k++) x[k] = live ? xw[(size_t)i * 12 + k] : 0u;
  const bool try_point = !(f & hbl::WIRE_INFINITY) && !(f & hbl::WIRE_REJECT) && below_p(x);
  bool valid = false;
  uint32_t y[12];
  for (int k = 0; k < 12; k++) y[k] = 0;
  if (role == 0) {
    bool g = false;
    if (try_point) g = g1q_in_subgroup(x);  // the same in the quad's four lanes
    if ((threadIdx.x & 3) == 0) in_group[slot] = g ? 1 : 0;
  } else if (f & hbl::WIRE_INFINITY) {
    valid = true;  // the point at infinity (all-zero ABI words)
    for (int k = 0; k < 12; k++) x[k] = 0;
  } else if (try_point) {  // the square root, beside the other wave's subgroup test
    uint32_t p[12];
    for (int k = 0; k < 12; k++) p[k] = hb::PM2_W[k];
    p[0] += 2;
    const hb::Fp xm = hb::fp_from_words(x);
    const hb::Fp rhs = hb::fp_add(hb::fp_mul(hb::fp_sqr(xm), xm), hb::fp_const(hb::B1_M));
    valid = hb::g1_root_y(rhs, f, p, y);  // on the curve; the subgroup verdict joins after the barrier
  }
  __syncthreads();
  if (role == 0 || !live) return;
  if (try_point) valid = valid && in_group[slot] != 0;
  uint32_t* o = out + (size_t)i * hb::G1_WORDS;
  for (int k = 0; k < 12; k++) {
    o[k] = valid ? x[k] : 0u;
    o[12 + k] = valid ? y[k] : 0u;
  }
  ok[i] = valid ? 1 : 0;
}

// G2: a quad is two lane pairs; a lane holds its own component (even: c0, odd: c1) of every Fp2
// value.  The root lane publishes N(y) through LDS; the quad finishes the Y comparison after the
// first barrier, as the throughput form does.
__global__ void __launch_bounds__(WS_THREADS) k_g2_decompress_split(int n, const uint32_t* __restrict__ xw,
                                                                     const uint8_t* __restrict__ flags,
                                                                     uint32_t* __restrict__ out,
                                                                     uint8_t* __restrict__ ok) {
  __shared__ uint32_t nrm[hb::NL * WS_POINTS];
  __shared__ uint8_t in_group[WS_POINTS];
  const int role = threadIdx.x >> 6;
  const int slot = role == 0 ? (int)(threadIdx.x >> 2) : (int)threadIdx.x - 64;
  const int i = blockIdx.x * WS_POINTS + slot;
  const bool live = i < n;
  const uint8_t f = live ? flags[i] : hbl::WIRE_REJECT;
  const uint32_t* xi = xw + (size_t)(live ? i : 0) * 24;
  uint32_t* o = out + (size_t)(live ? i : 0) * hb::G2_WORDS;
  bool try_point;
  {
    uint32_t x[24];
    for (int k = 0; k < 24; k++) x[k] = xi[k];
    try_point = !(f & hbl::WIRE_INFINITY) && !(f & hbl::WIRE_REJECT) && below_p(x) && below_p(x + 12);
  }
  bool valid = false, gx = false;
  hbs::Fp qy = hbs::fp_zero(), w = hbs::fp_zero();  // quads only, across the barrier (own components)
  if (role == 0) {
    if (try_point) {
      using namespace hbs;
      const Fp xm = fp_from_words(xi + (lp_even() ? 0 : 12));
      const Fp rhs = fp_add(h_mul(h_sqr(xm), xm), h_const(hb::B1_M, hb::B1_M));  // b = 4 (1 + u)
      Fp X, Y;
      h_mul2(rhs, xm, rhs, rhs, X, Y);
      // [|x|] P', written out: through dbl_and_add this loop compiles to other registers here
      HJac q{X, Y, h_one()};
#pragma unroll 1
      for (int b = 62; b >= 0; b--) {
        q = qj_dbl(q);
        if ((hb::X_ABS >> b) & 1) q = qj_add_affine(q, X, Y);
      }
      // target iota(-psi(P)) = (C1 rhs conj(x), -C2 rhs N(y)); C1 = c1 u, so C1 conj(x) = (x1 c1, x0 c1)
      const Fp cx = fp_mul(dpp_fp<DPP_SWAP>(xm), fp_const(hb::PSI_C1_C1));
      const Fp z2 = h_sqr(q.z);
      Fp tx, z3, txz, rc2;
      h_mul2(rhs, cx, z2, q.z, tx, z3);
      h_mul2(tx, z2, rhs, h_const(hb::PSI_C2_C0, hb::PSI_C2_C1), txz, rc2);
      gx = !hj_is_zero(q) && h_is_zero(fp_sub(q.x, txz));
      w = fp_neg(h_mul(rc2, z3));
      qy = q.y;
    }
  } else if (f & hbl::WIRE_INFINITY) {
    valid = live;  // the point at infinity (all-zero ABI words)
    if (live)
      for (int k = 0; k < hb::G2_WORDS; k++) o[k] = 0u;
  } else if (try_point) {
    using namespace hb;
    const Fp2 b2 = {fp_const(B1_M), fp_const(B1_M)};  // 4 (1 + u)
    const Fp2 xm = {fp_from_words(xi), fp_from_words(xi + 12)};
    const Fp2 rhs = f2_add(f2_mul(f2_sqr(xm), xm), b2);
    Fp2 ym;
    if (g2_root_y(rhs, f, ym)) {
      const Fp nm = fp_add(fp_sqr(ym.c0), fp_sqr(ym.c1));
      for (int k = 0; k < NL; k++) nrm[k * WS_POINTS + slot] = nm.l[k];
      // on the curve: written now, zeroed after the second barrier when not in the subgroup
      for (int k = 0; k < 24; k++) o[k] = xi[k];
      fp_to_words(ym.c0, o + 24);
      fp_to_words(ym.c1, o + 36);
      valid = true;
    }
  }
  __syncthreads();
  if (role == 0) {
    bool g = false;
    if (try_point && gx) {  // gx: the same in the quad's four lanes
      hbs::Fp nm;
      for (int k = 0; k < hb::NL; k++) nm.l[k] = (int32_t)nrm[k * WS_POINTS + slot];
      g = hbs::h_is_zero(hbs::fp_sub(qy, hbs::fp_mul(w, nm)));
    }
    if ((threadIdx.x & 3) == 0) in_group[slot] = g ? 1 : 0;
  }
  __syncthreads();
  if (role == 0 || !live) return;
  if (try_point) valid = valid && in_group[slot] != 0;
  if (!valid)
    for (int k = 0; k < hb::G2_WORDS; k++) o[k] = 0u;
  ok[i] = valid ? 1 : 0;
}

}  // namespace hbw

namespace hbl {

hipError_t g1_decompress_split(hipStream_t s, int n, const uint32_t* xw, const uint8_t* flags, void* out, uint8_t* ok) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(hbw::k_g1_decompress_split, dim3((unsigned)((n + hbw::WS_POINTS - 1) / hbw::WS_POINTS)),
                     dim3(hbw::WS_THREADS), 0, s, n, xw, flags, (uint32_t*)out, ok);
  return hipGetLastError();
}

hipError_t g2_decompress_split(hipStream_t s, int n, const uint32_t* xw, const uint8_t* flags, void* out, uint8_t* ok) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(hbw::k_g2_decompress_split, dim3((unsigned)((n + hbw::WS_POINTS - 1) / hbw::WS_POINTS)),
                     dim3(hbw::WS_THREADS), 0, s, n, xw, flags, (uint32_t*)out, ok);
  return hipGetLastError();
}

}  // namespace hbl
