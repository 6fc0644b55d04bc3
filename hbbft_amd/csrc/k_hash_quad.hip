// Latency form of hashing to G2 on the device (HBH_HFORM_QUAD): the kernels of k_hash.hip with FOUR
// lanes per message, for the batches whose time is the length of one lane's chain, not its work.
//
//   k_hash_sample_quad  the four lanes of a quad try the message's NEXT FOUR candidates side by side:
//                  lane j opens the stream at the saved position (hash_sample.hpp), steps over j
//                  candidates (skip_candidate: no field work) and draws its own; rhs and the first
//                  chain of the norm-method root are k_hash_sample's one-lane arithmetic (hb::Fp,
//                  wire_root.hpp), each lane on its own candidate.  The quad then agrees (two DPP
//                  quad permutes, at a point all four lanes reach) on the lowest DECISIVE lane: one that
//                  accepted its candidate (rhs a square, or 0) or whose draw failed.  G2::rand takes
//                  the first acceptable candidate, which is that lane's, so an accepting winner
//                  alone runs the second chain and the sign choice, stores (x, y) and the position
//                  behind its own candidate; a failed-draw winner reports HASH_FAILED; with no
//                  decisive lane the last trying lane saves its position and appends the message to
//                  the next worklist.  A message is resolved in one launch with probability 15/16
//                  instead of 1/2, and the launch is as long as two (p - 3) / 4 chains whatever the
//                  luck of its messages.
//   k_hash_clear_quad<FULL>  one lane quad per sampled point: cofactor_bp and (FULL) kcof_mul of
//                  k_hash.hip, the same formulas and the same digit identity, on the lane-pair Fp2 of
//                  pfp.hpp with the group law of g2quad.hpp (a doubling in 4 product rounds instead
//                  of 7 serial Fp2 products, a mixed addition in 6 instead of 11, a general one in 9
//                  instead of 16), psi and negation on the lane-pair layout, then one inversion for
//                  the affine ABI words.  Both field forms use radix 2^28 and R = 2^392, so the
//                  sampler's limbs are read as they are.
//
// Same bytes: the sampler's arithmetic is k_hash.hip's, and the clearing kernel writes the canonical
// affine coordinates of the same group element.  Same leftovers: the round cap stays a cap on
// CANDIDATES -- a launch takes `budget` <= 4 of them and the lanes past the budget try nothing -- so a
// message is resolved under cap c exactly when its candidate count is <= c, as in the lane form.
//
// Lock-step: the four lanes of a quad read the same message index and state, so a dead slot leaves as
// a whole quad; in the clearing kernel every branch depends on the point only (g2quad.hpp), never on
// the lane's place in the quad, so DPP source lanes are always active.  In the sampler the lanes
// diverge on their candidates and meet again at the exchange.
#define HB_FP_LATENCY 1
#define HS_MULFN static __device__ __noinline__
#include <hip/hip_runtime.h>

#include "curve.hpp"
#include "g2quad.hpp"
#include "hash_sample.hpp"
#include "hash_work.hpp"
#include "launch.hpp"
#include "wire_root.hpp"

namespace hb {

constexpr int HQ_MSGS = 16;  // messages per 64-lane workgroup

// k_hash.hip's: pairing's Montgomery limbs (R = 2^384) -> this field's form, one product
__device__ __forceinline__ Fp fq_limbs_to_fp(const uint32_t w[12]) {
  return fp_mul(fp_limbs_from_words(w), fp_const(FQ_RAND_M));
}

// budget: the candidates this launch may try per message, 1..4 (the round cap's remainder)
__global__ void __launch_bounds__(64) k_hash_sample_quad(int n, int budget, const uint32_t* __restrict__ count,
                                                         const uint32_t* __restrict__ list,
                                                         const uint8_t* __restrict__ seeds, uint32_t* __restrict__ pos,
                                                         uint32_t* __restrict__ xy, uint8_t* __restrict__ state,
                                                         uint32_t* __restrict__ next_list,
                                                         uint32_t* __restrict__ next_count) {
  const uint32_t g = blockIdx.x * HQ_MSGS + (threadIdx.x >> 2);
  const int j = (int)(threadIdx.x & 3);
  const uint32_t m = count ? min(*count, (uint32_t)n) : (uint32_t)n;  // the first launch takes every message
  if (g >= m) return;  // the whole quad
  const uint32_t i = list ? list[g] : g;
  if (i >= (uint32_t)n) return;  // the whole quad
  enum { REJECTED = 0, ACCEPTED = 1, DRAW_FAILED = 2 };
  int verdict = REJECTED;  // also a lane past the budget, and one behind an earlier lane's failed draw
  hsample::Stream st;
  bool greatest = false, zero = false;
  Fp2 x = f2_zero(), rhs = f2_zero();
  Fp s = fp_zero();
  if (j < budget) {
    uint8_t seed[32];
    for (int k = 0; k < 32; k++) seed[k] = seeds[(size_t)i * 32 + k];
    hsample::stream_open(st, seed, pos[2 * (size_t)i], pos[2 * (size_t)i + 1]);
    bool there = true;
    for (int k = 0; k < j; k++) there = there && hsample::skip_candidate(st);
    if (there) {
      uint32_t w0[12], w1[12];
      if (!hsample::gen_fq(st, w0) || !hsample::gen_fq(st, w1)) {
        verdict = DRAW_FAILED;  // 64 draws >= p in a row (0.187^64): left to the host stage
      } else {
        greatest = hsample::gen_bool(st);
        x = {fq_limbs_to_fp(w0), fq_limbs_to_fp(w1)};
        const Fp2 b2 = {fp_const(B1_M), fp_const(B1_M)};  // 4 (1 + u)
        rhs = f2_add(f2_mul(f2_sqr(x), x), b2);
        zero = f2_is_zero(rhs);  // its own root (k_hash_sample)
        if (zero || f2_sqrt_norm_first(rhs, s)) verdict = ACCEPTED;
      }
    }
  }
  // every lane of the quad is here (the lanes of a wave that left above belong to other quads): bit k
  // of `decisive` is lane k's flag, OR-ed over the quad in two DPP quad permutations.  Nothing behind
  // this point reads threadIdx: j alone names the lane.
  int32_t mine = verdict != REJECTED ? 1 << j : 0;
  mine |= hbs::dpp<hbs::DPP_SWAP>(mine);
  const uint32_t decisive = (uint32_t)(mine | hbs::dpp<hbs::DPP_QSWAP>(mine));
  if (decisive == 0) {
    if (j == budget - 1) {  // the last candidate tried: the next launch starts behind it
      pos[2 * (size_t)i] = (uint32_t)st.block;
      pos[2 * (size_t)i + 1] = st.word;
      const uint32_t k = atomicAdd(next_count, 1u);
      if (k < (uint32_t)n) next_list[k] = i;  // each message joins a launch's list at most once, so k < n
    }
    return;
  }
  if (j != __builtin_ctz(decisive)) return;
  if (verdict == DRAW_FAILED) {
    state[i] = hbl::HASH_FAILED;
    return;
  }
  // the position behind this candidate, for a retry after k_hash_clear_quad
  pos[2 * (size_t)i] = (uint32_t)st.block;
  pos[2 * (size_t)i + 1] = st.word;
  Fp2 y = f2_zero();
  if (!zero) (void)f2_sqrt_norm_second(rhs, s, y);
  const Fp2 ny = f2_neg(y);
  if (f2_gt_canon(y, ny) != greatest) y = ny;  // keep y iff (y > -y) == greatest
  uint32_t* o = xy + (size_t)i * XY_WORDS;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    o[k] = x.c0.l[k];
    o[NL + k] = x.c1.l[k];
    o[2 * NL + k] = y.c0.l[k];
    o[3 * NL + k] = y.c1.l[k];
  }
  state[i] = hbl::HASH_SAMPLED;
}

}  // namespace hb

namespace hbs {

HP_D HJac hj_neg(const HJac& p) { return {p.x, fp_neg(p.y), p.z}; }

// psi on Jacobian coordinates, own components: (conj(X) cx, conj(Y) cy, conj(Z)) with cx = c u, so
// conj(X) cx = (X1 c, X0 c) -- the partner's component times c (k_interp_pair.hip psi_xh / psi_yh)
HP_D HJac hj_psi(const HJac& p) {
  return {fp_reduce(fp_mul(dpp_fp<DPP_SWAP>(p.x), fp_const(hb::PSI_C1_C1))),
          fp_reduce(h_mul(h_conj(p.y), h_const(hb::PSI_C2_C0, hb::PSI_C2_C1))), h_conj(p.z)};
}

// [k] P over a constant 64-bit k with its top bit at `top`, P in Jacobian coordinates
HP_D HJac hj_mul_const(const HJac& p, uint64_t k, int top) {
  return dbl_and_add(p, k, top - 1, [](const HJac& a) HS_LAMBDA { return qj_dbl(a); },
                     [&](const HJac& a) HS_LAMBDA { return qj_add(a, p); });
}

// k_hash.hip kcof_mul: [KCOF] Q = [d0] (B0 + 2 B1 + 2 B2 + B3) - (B1 + 2 B2 + B3), B_j = (-psi)^j(Q)
HP_D HJac hq_kcof_mul(const HJac& q) {
  const HJac b1 = hj_neg(hj_psi(q));
  const HJac b2 = hj_neg(hj_psi(b1));
  const HJac b3 = hj_neg(hj_psi(b2));
  const HJac b12 = qj_add(b1, b2);
  const HJac t = qj_add(b12, qj_add(b2, b3));
  const HJac s = qj_add(qj_add(qj_dbl(b12), q), b3);
  return qj_add(hj_mul_const(s, hb::KCOF_D[0], 62), hj_neg(t));
}

// k_hash.hip cofactor_bp for the affine sampled point (x, y): the first chain and the last addition
// take the mixed addition
HP_D HJac hq_cofactor_bp(const Fp& x, const Fp& y) {
  const HJac p = {x, y, h_one()};
  const HJac t1 = hj_neg(dbl_and_add(p, hb::X_ABS, 62, [](const HJac& a) HS_LAMBDA { return qj_dbl(a); },
                                     [&](const HJac& a) HS_LAMBDA { return qj_add_affine(a, x, y); }));  // [x] P
  HJac t2 = hj_psi(p);
  HJac t3 = hj_psi(hj_psi(qj_dbl(p)));
  t3 = qj_add(t3, hj_neg(t2));
  t2 = qj_add(t1, t2);
  t2 = hj_neg(hj_mul_const(t2, hb::X_ABS, 63));  // [x] ([x] P + psi(P))
  t3 = qj_add(t3, t2);
  t3 = qj_add(t3, hj_neg(t1));
  return qj_add_affine(t3, x, fp_neg(y));
}

template <bool FULL>
HP_D void hash_clear_quad(int n, const uint32_t* __restrict__ xy, uint8_t* __restrict__ state,
                          uint32_t* __restrict__ out, uint32_t* __restrict__ retry_list,
                          uint32_t* __restrict__ retry_count) {
  const int i = (int)(blockIdx.x * hb::HQ_MSGS + (threadIdx.x >> 2));
  if (i >= n) return;  // the whole quad
  const bool leader = (threadIdx.x & 3) == 0;
  // the four lanes read the state before the leader's store below: it stands behind the quad's last
  // cross-lane exchange, which no lane passes alone
  const uint8_t st = state[i];
  if (st == hbl::HASH_DONE) return;
  uint32_t* o = out + (size_t)i * hb::G2_WORDS;
  if (st != hbl::HASH_SAMPLED) {  // unresolved: no point is ever left unwritten
    if (leader)
      for (int k = 0; k < hb::G2_WORDS; k++) o[k] = 0u;
    return;
  }
  const uint32_t* w = xy + (size_t)i * hb::XY_WORDS + (lp_even() ? 0 : NL);
  Fp x, y;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    x.l[k] = (int32_t)w[k];
    y.l[k] = (int32_t)w[2 * NL + k];
  }
  const HJac q = hq_cofactor_bp(x, y);
  if (hj_is_zero(q)) {
    // h2 (x, y) = O: back to the sampler, whose saved position stands behind this candidate (k_hash.hip)
    if (leader) {
      state[i] = hbl::HASH_PENDING;
      for (int k = 0; k < hb::G2_WORDS; k++) o[k] = 0u;
      if (retry_list) {
        const uint32_t k = atomicAdd(retry_count, 1u);
        if (k < (uint32_t)n) retry_list[k] = (uint32_t)i;
      }
    }
    return;
  }
  const HJac r = FULL ? hq_kcof_mul(q) : q;
  if (hj_is_zero(r)) {  // g2_jac_to_words's zero; [KCOF] of a nonzero point of G2 is never O
    if (leader) {
      for (int k = 0; k < hb::G2_WORDS; k++) o[k] = 0u;
      state[i] = hbl::HASH_DONE;
    }
    return;
  }
  const Fp zi = h_inv_vartime(fp_reduce(r.z));
  const Fp zi2 = h_sqr(zi);
  Fp xa, zi3;
  h_mul2(r.x, zi2, zi2, zi, xa, zi3);
  const Fp ya = h_mul(r.y, zi3);
  if (!q_hi()) {  // pair 0: each lane its own component
    uint32_t* oc = o + (lp_even() ? 0 : 12);
    fp_to_words(xa, oc);
    fp_to_words(ya, oc + 24);
  }
  if (leader) state[i] = hbl::HASH_DONE;
}

__global__ void __launch_bounds__(64) k_hash_clear_quad(int n, const uint32_t* __restrict__ xy,
                                                        uint8_t* __restrict__ state, uint32_t* __restrict__ out,
                                                        uint32_t* __restrict__ retry_list,
                                                        uint32_t* __restrict__ retry_count) {
  hash_clear_quad<true>(n, xy, state, out, retry_list, retry_count);
}

__global__ void __launch_bounds__(64) k_hash_clear_quad_bp(int n, const uint32_t* __restrict__ xy,
                                                           uint8_t* __restrict__ state, uint32_t* __restrict__ out,
                                                           uint32_t* __restrict__ retry_list,
                                                           uint32_t* __restrict__ retry_count) {
  hash_clear_quad<false>(n, xy, state, out, retry_list, retry_count);
}

}  // namespace hbs

namespace hbl {

namespace {
// sampler launches for `candidates` more candidates per message: four per launch, the last one the
// remainder.  Launch k reads cnt entries of lst (nullptr: every message) and appends the messages it
// leaves to w.list[(par + k + 1) & 1], counted in cnts[k].  Returns the list and count the last
// launch wrote through lst / cnt.
void sample_launches(hipStream_t s, int n, int candidates, const uint8_t* seeds, const HashWork& w, uint8_t* state,
                     const uint32_t*& cnt, const uint32_t*& lst, uint32_t* cnts, int par) {
  const dim3 grid((unsigned)((n + hb::HQ_MSGS - 1) / hb::HQ_MSGS)), block(64);
  for (int k = 0; 4 * k < candidates; k++) {
    const int budget = candidates - 4 * k < 4 ? candidates - 4 * k : 4;
    uint32_t* nl = w.list[(par + k + 1) & 1];
    hipLaunchKernelGGL(hb::k_hash_sample_quad, grid, block, 0, s, n, budget, cnt, lst, seeds, w.pos, w.xy, state, nl,
                       cnts + k);
    cnt = cnts + k;
    lst = nl;
  }
}
}  // namespace

hipError_t hash_g2_quad(hipStream_t s, int n, int rounds, const uint8_t* seeds, void* work, uint8_t* state, void* out,
                        HashForm form) {
  if (n <= 0) return hipSuccess;
  const auto clear = form == HASH_FORM_BP ? hbs::k_hash_clear_quad_bp : hbs::k_hash_clear_quad;
  const HashWork w = hash_carve(work, (size_t)n, rounds);
  hipError_t err = hipMemsetAsync(w.counts, 0, (size_t)((uint8_t*)w.xy - (uint8_t*)w.counts), s);
  if (err != hipSuccess) return err;
  err = hipMemsetAsync(state, 0, (size_t)n, s);  // HASH_PENDING
  if (err != hipSuccess) return err;
  const dim3 grid((unsigned)((n + hb::HQ_MSGS - 1) / hb::HQ_MSGS)), block(64);
  // ceil(rounds / 4) launches over the work layout of hash_g2: launch k counts its leftovers in counts[k + 1]
  // (of the rounds + 1 words hash_g2 uses), the retry count and the retry launches' counts behind them.  The
  // grid covers n quads every launch: the host never reads a count, so the call stays asynchronous.
  const uint32_t* cnt = nullptr;
  const uint32_t* lst = nullptr;
  sample_launches(s, n, rounds, seeds, w, state, cnt, lst, w.counts + 1, 0);
  uint32_t* rc = w.counts + rounds + 1;
  hipLaunchKernelGGL(clear, grid, block, 0, s, n, w.xy, state, (uint32_t*)out, w.retry, rc);
  // messages whose multiple was O (none in practice): HASH_RETRY_ROUNDS more candidates and a second
  // clearing, which also zeroes whatever is still unresolved
  cnt = rc;
  lst = w.retry;
  sample_launches(s, n, HASH_RETRY_ROUNDS, seeds, w, state, cnt, lst, rc + 1, 1);
  hipLaunchKernelGGL(clear, grid, block, 0, s, n, w.xy, state, (uint32_t*)out, (uint32_t*)nullptr,
                     (uint32_t*)nullptr);
  return hipGetLastError();
}

}  // namespace hbl
