// The G1 group law on LANE QUADS (namespace hbs, signed-limb Fp of sfp.hpp): four lanes hold the
// same point and split every group operation's independent Fp products between them, one product
// per lane per round, exchanging results with DPP quad broadcasts: a doubling takes 3 rounds
// instead of 7 serial products, a mixed or general addition 5 instead of 11 / 16.  Formulas:
// dbl-2009-l, madd-2007-bl, add-2007-bl (the group law of curve.hpp, exceptional cases included).
// Shared by the Ack-check / interpolation kernels (k_g1quad.hip) and the latency form of the G1
// decoder (k_wire_split.hip).  Every branch depends only on the point, never on the lane's place
// in the quad, so a DPP source lane is always active.
#pragma once
#include "sfp.hpp"

namespace hbs {

struct QJ {
  Fp x, y, z;
};

__device__ __forceinline__ int q_lane() { return threadIdx.x & 3; }
template <int CTRL>
__device__ __forceinline__ Fp q_dpp(const Fp& a) {
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = __builtin_amdgcn_mov_dpp(a.l[i], CTRL, 0xF, 0xF, true);
  return r;
}
__device__ __forceinline__ Fp q_sel4(int q, const Fp& a0, const Fp& a1, const Fp& a2, const Fp& a3) {
  return fp_sel(q == 0, a0, fp_sel(q == 1, a1, fp_sel(q == 2, a2, a3)));
}
// one round: lane k of the quad forms a_k * b_k; every lane gets all four products
__device__ __forceinline__ void q4(const Fp& a0, const Fp& b0, const Fp& a1, const Fp& b1, const Fp& a2, const Fp& b2,
                                   const Fp& a3, const Fp& b3, Fp& r0, Fp& r1, Fp& r2, Fp& r3) {
  const int q = q_lane();
  const Fp r = fp_mul(q_sel4(q, a0, a1, a2, a3), q_sel4(q, b0, b1, b2, b3));
  r0 = q_dpp<0x00>(r);
  r1 = q_dpp<0x55>(r);
  r2 = q_dpp<0xAA>(r);
  r3 = q_dpp<0xFF>(r);
}
__device__ __forceinline__ void q3(const Fp& a0, const Fp& b0, const Fp& a1, const Fp& b1, const Fp& a2, const Fp& b2,
                                   Fp& r0, Fp& r1, Fp& r2) {
  const int q = q_lane();
  const Fp r = fp_mul(q_sel4(q, a0, a1, a2, a2), q_sel4(q, b0, b1, b2, b2));
  r0 = q_dpp<0x00>(r);
  r1 = q_dpp<0x55>(r);
  r2 = q_dpp<0xAA>(r);
}
__device__ __forceinline__ void q2(const Fp& a0, const Fp& b0, const Fp& a1, const Fp& b1, Fp& r0, Fp& r1) {
  const bool odd = (q_lane() & 1) != 0;
  const Fp r = fp_mul(fp_sel(odd, a1, a0), fp_sel(odd, b1, b0));
  r0 = q_dpp<0x00>(r);
  r1 = q_dpp<0x55>(r);
}

__device__ __forceinline__ bool qj_zero(const QJ& p) { return fp_is_zero(p.z); }
__device__ __forceinline__ QJ qj_inf() { return {fp_one(), fp_one(), fp_zero()}; }

// dbl-2009-l, 3 rounds; inputs reduced, outputs reduced
__device__ __forceinline__ QJ g1q_dbl(const QJ& p) {
  Fp A, B, YZ, C, XB2, F, u;
  q3(p.x, p.x, p.y, p.y, p.y, p.z, A, B, YZ);
  const Fp E = fp_lin(3, A, 0, A);
  const Fp XB = fp_add(p.x, B);
  q3(B, B, XB, XB, E, E, C, XB2, F);
  const Fp D = fp_reduce(fp_lin(2, fp_sub(fp_sub(XB2, A), C), 0, C));
  QJ r;
  r.x = fp_reduce(fp_sub(F, fp_add(D, D)));
  u = fp_mul(E, fp_sub(D, r.x));
  r.y = fp_reduce(fp_sub(u, fp_lin(8, C, 0, C)));
  r.z = fp_reduce(fp_add(YZ, YZ));
  return r;
}

// madd-2007-bl: p + (x2, y2) with (x2, y2) affine and not infinity, 5 rounds
__device__ __forceinline__ QJ g1q_add_affine(const QJ& p, const Fp& x2, const Fp& y2) {
  if (qj_zero(p)) return {x2, y2, fp_one()};
  Fp Z1Z1, YZ, U2, S2;
  q2(p.z, p.z, y2, p.z, Z1Z1, YZ);
  q2(x2, Z1Z1, YZ, Z1Z1, U2, S2);
  const Fp H = fp_reduce(fp_sub(U2, p.x));
  const Fp rr = fp_reduce(fp_lin(2, S2, -2, p.y));
  if (fp_is_zero(H)) {
    if (fp_is_zero(rr)) return g1q_dbl(p);
    return qj_inf();
  }
  Fp HH, RR, ZH, J, V, EV, YJ;
  q3(H, H, rr, rr, p.z, H, HH, RR, ZH);
  const Fp I = fp_lin(4, HH, 0, HH);
  q2(H, I, p.x, I, J, V);
  QJ r;
  r.x = fp_reduce(fp_sub(fp_sub(RR, J), fp_add(V, V)));
  q2(rr, fp_sub(V, r.x), p.y, J, EV, YJ);
  r.y = fp_reduce(fp_sub(EV, fp_add(YJ, YJ)));
  r.z = fp_reduce(fp_add(ZH, ZH));
  return r;
}

// add-2007-bl (general), 5 rounds
__device__ __forceinline__ QJ g1q_add(const QJ& p, const QJ& q) {
  if (qj_zero(p)) return q;
  if (qj_zero(q)) return p;
  Fp Z1Z1, Z2Z2, Y1Z2, Y2Z1, U1, U2, S1, S2;
  q4(p.z, p.z, q.z, q.z, p.y, q.z, q.y, p.z, Z1Z1, Z2Z2, Y1Z2, Y2Z1);
  q4(p.x, Z2Z2, q.x, Z1Z1, Y1Z2, Z2Z2, Y2Z1, Z1Z1, U1, U2, S1, S2);
  const Fp H = fp_reduce(fp_sub(U2, U1));
  const Fp rr = fp_reduce(fp_lin(2, S2, -2, S1));
  if (fp_is_zero(H)) {
    if (fp_is_zero(rr)) return g1q_dbl(p);
    return qj_inf();
  }
  Fp I, RR, Z12, J, V, Z12H, EV, SJ;
  const Fp H2 = fp_add(H, H);
  q3(H2, H2, rr, rr, p.z, q.z, I, RR, Z12);
  q3(H, I, U1, I, Z12, H, J, V, Z12H);
  QJ r;
  r.x = fp_reduce(fp_sub(fp_sub(RR, J), fp_add(V, V)));
  q2(rr, fp_sub(V, r.x), S1, J, EV, SJ);
  r.y = fp_reduce(fp_sub(EV, fp_add(SJ, SJ)));
  r.z = fp_reduce(fp_add(Z12H, Z12H));
  return r;
}

}  // namespace hbs
