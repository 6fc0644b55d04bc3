// Hashing to G2 on the device (gfx950): the curve half of threshold_crypto hash_g2 -- pairing 0.14
// G2::rand over ChaChaRng::from_seed(sha3_256(msg)), as csrc/host_hash.cpp g2_rand_bp + hash_g2 and
// oracle/tc.py restate it.  SHA3 and the message assembly stay on the host; the kernels take 32-byte
// seeds and write ABI G2 points, byte for byte the host stage's.
//
//   k_hash_sample  one lane per unresolved message tries that message's NEXT candidate: x = (gen_fq,
//                  gen_fq) and the sign flag from the saved stream position (hash_sample.hpp), rhs =
//                  x^3 + 4 (1 + u), the first chain of the norm-method root (wire_root.hpp).  That chain
//                  decides squareness, so a rejected candidate costs one (p - 3) / 4 chain; an accepted one
//                  runs the second chain, picks y or -y by pairing's Ord and stores (x, y).  A rejected
//                  message saves its stream position and joins the next round's worklist.  Rounds over a
//                  compacted worklist instead of a per-lane loop: half the candidates fail, and a wave
//                  that loops waits for its unluckiest lane (12 candidates among 2,000 test messages).
//   k_hash_clear   one lane per sampled point: h2 (x, y) to affine ABI words with one inversion.
//   k_hash_clear_bp  the Q form of the same body: it stops at the Budroni-Pintore image Q_bp (h2 (x, y) =
//                  [KCOF] Q_bp), the bytes of the host stage's hbh_hash_g1_g2_bp, for callers that fold
//                  [KCOF] into a pairing side or a scalar (Ciphertext::verify, encrypt's W).
//
// Outputs are keyed by message index, so the order in which lanes append to a worklist does not matter.
// Every loop is bounded: the launcher runs a fixed number of rounds, gen_fq draws at most 64 times, and a
// message that is still unresolved is reported (state != HASH_DONE, all-zero output) for the caller to
// hash on the host stage.
// Variable-time Fp inverse (fp.hpp) for the affine output: public inputs only take this path.
#define HB_FP_LATENCY 1
#include <hip/hip_runtime.h>

#include "curve.hpp"
#include "hash_sample.hpp"
#include "hash_work.hpp"
#include "launch.hpp"
#include "wire_root.hpp"

namespace hb {

// pairing's Montgomery limbs (R = 2^384, twelve 32-bit words < p) -> this field's form: one product
__device__ __forceinline__ Fp fq_limbs_to_fp(const uint32_t w[12]) {
  return fp_mul(fp_limbs_from_words(w), fp_const(FQ_RAND_M));
}

__global__ void __launch_bounds__(64) k_hash_sample(int n, const uint32_t* __restrict__ count,
                                                    const uint32_t* __restrict__ list,
                                                    const uint8_t* __restrict__ seeds, uint32_t* __restrict__ pos,
                                                    uint32_t* __restrict__ xy, uint8_t* __restrict__ state,
                                                    uint32_t* __restrict__ next_list,
                                                    uint32_t* __restrict__ next_count) {
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  const uint32_t m = count ? min(*count, (uint32_t)n) : (uint32_t)n;  // the first round takes every message
  if (g >= m) return;
  const uint32_t i = list ? list[g] : g;
  if (i >= (uint32_t)n) return;
  hsample::Stream st;
  {
    uint8_t seed[32];
    for (int k = 0; k < 32; k++) seed[k] = seeds[(size_t)i * 32 + k];
    hsample::stream_open(st, seed, pos[2 * (size_t)i], pos[2 * (size_t)i + 1]);
  }
  uint32_t w0[12], w1[12];
  if (!hsample::gen_fq(st, w0) || !hsample::gen_fq(st, w1)) {
    state[i] = hbl::HASH_FAILED;  // 64 draws >= p in a row (0.187^64): left to the host stage
    return;
  }
  const bool greatest = hsample::gen_bool(st);
  // the position behind this candidate, for the next round (or for a retry after k_hash_clear)
  pos[2 * (size_t)i] = (uint32_t)st.block;
  pos[2 * (size_t)i + 1] = st.word;
  const Fp2 x = {fq_limbs_to_fp(w0), fq_limbs_to_fp(w1)};
  const Fp2 b2 = {fp_const(B1_M), fp_const(B1_M)};  // 4 (1 + u)
  const Fp2 rhs = f2_add(f2_mul(f2_sqr(x), x), b2);
  // (rhs = 0 would be its own root, as in f2_sqrt_norm; #E'(Fp2) = h2 r is odd, so no x gives it)
  const bool zero = f2_is_zero(rhs);
  Fp s;
  if (!zero && !f2_sqrt_norm_first(rhs, s)) {
    const uint32_t k = atomicAdd(next_count, 1u);
    if (k < (uint32_t)n) next_list[k] = i;  // each message joins a round's list at most once, so k < n
    return;
  }
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

// psi on Jacobian coordinates: (conj(X) cx, conj(Y) cy, conj(Z)), an endomorphism of all of E'(Fp2)
__device__ __forceinline__ Jac<Fp2> jac_psi(const Jac<Fp2>& p) {
  const Fp c = fp_const(PSI_C1_C1);
  const Fp2 c2 = {fp_const(PSI_C2_C0), fp_const(PSI_C2_C1)};
  return {{fp_mul(p.x.c1, c), fp_mul(p.x.c0, c)}, f2_mul(f2_conj(p.y), c2), f2_conj(p.z)};
}

// [k] P by double-and-add over a constant (wave-uniform) 64-bit k with its top bit at `top`
__device__ __forceinline__ Jac<Fp2> jac_mul_const(const Jac<Fp2>& p, uint64_t k, int top) {
  Jac<Fp2> acc = p;
#pragma unroll 1
  for (int i = top - 1; i >= 0; i--) {
    acc = jac_dbl(acc);
    if ((k >> i) & 1) acc = jac_add(acc, p);
  }
  return acc;
}

// KCOF = d0 + d1 |x| + d2 |x|^2 + d3 |x|^3 with d1 = 2 d0 - 1, d2 = 2 d0 - 2, d3 = d0 - 1
// (tools/gen_constants.py computes the digits), so on G2, where [|x|] = -psi and B_j = (-psi)^j(Q),
//   [KCOF] Q = [d0] (B0 + 2 B1 + 2 B2 + B3) - (B1 + 2 B2 + B3):
// one 63-bit chain instead of four.
static_assert(KCOF_D[1] == 2 * KCOF_D[0] - 1 && KCOF_D[2] == 2 * KCOF_D[0] - 2 && KCOF_D[3] == KCOF_D[0] - 1 &&
                  (KCOF_D[0] >> 62) == 1,
              "the digit relations behind kcof_mul");
__device__ __forceinline__ Jac<Fp2> kcof_mul(const Jac<Fp2>& q) {
  const Jac<Fp2> b1 = jac_neg(jac_psi(q));
  const Jac<Fp2> b2 = jac_neg(jac_psi(b1));
  const Jac<Fp2> b3 = jac_neg(jac_psi(b2));
  const Jac<Fp2> b12 = jac_add(b1, b2);
  const Jac<Fp2> t = jac_add(b12, jac_add(b2, b3));                    // B1 + 2 B2 + B3
  const Jac<Fp2> s = jac_add(jac_add(jac_dbl(b12), q), b3);            // B0 + 2 B1 + 2 B2 + B3
  return jac_add(jac_mul_const(s, KCOF_D[0], 62), jac_neg(t));
}

// Q_bp = [x^2 - x - 1] P + [x - 1] psi(P) + psi^2(2 P) for any P on E'(Fp2) (Budroni-Pintore; the chain of
// host_hash.cpp cofactor_bp): Q_bp lies in G2 and h2 P = [KCOF] Q_bp.
__device__ __forceinline__ Jac<Fp2> cofactor_bp(const Jac<Fp2>& p) {
  const Jac<Fp2> t1 = jac_neg(jac_mul_const(p, X_ABS, 63));  // [x] P
  Jac<Fp2> t2 = jac_psi(p);
  Jac<Fp2> t3 = jac_psi(jac_psi(jac_dbl(p)));
  t3 = jac_add(t3, jac_neg(t2));
  t2 = jac_add(t1, t2);
  t2 = jac_neg(jac_mul_const(t2, X_ABS, 63));  // [x] ([x] P + psi(P))
  t3 = jac_add(t3, t2);
  t3 = jac_add(t3, jac_neg(t1));
  return jac_add(t3, jac_neg(p));
}

// FULL: out = h2 (x, y) = [KCOF] Q_bp (hash_g2's bytes); otherwise out = Q_bp
template <bool FULL>
__device__ __forceinline__ void hash_clear(int n, const uint32_t* __restrict__ xy, uint8_t* __restrict__ state,
                                           uint32_t* __restrict__ out, uint32_t* __restrict__ retry_list,
                                           uint32_t* __restrict__ retry_count) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint8_t st = state[i];
  if (st == hbl::HASH_DONE) return;
  uint32_t* o = out + (size_t)i * G2_WORDS;
  if (st != hbl::HASH_SAMPLED) {  // unresolved: no point is ever left unwritten
    for (int k = 0; k < G2_WORDS; k++) o[k] = 0u;
    return;
  }
  const uint32_t* w = xy + (size_t)i * XY_WORDS;
  Jac<Fp2> p;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    p.x.c0.l[k] = w[k];
    p.x.c1.l[k] = w[NL + k];
    p.y.c0.l[k] = w[2 * NL + k];
    p.y.c1.l[k] = w[3 * NL + k];
  }
  p.z = f2_one();
  const Jac<Fp2> q = cofactor_bp(p);
  if (jac_is_zero(q)) {
    // h2 (x, y) = O: G2::rand's loop continues with the next candidate, so the message goes back to the
    // sampler (its saved position already stands behind this candidate).  No test can reach this branch:
    // a sampled point lies in the h2-torsion with probability about 1 / r.
    state[i] = hbl::HASH_PENDING;
    for (int k = 0; k < G2_WORDS; k++) o[k] = 0u;
    if (retry_list) {
      const uint32_t k = atomicAdd(retry_count, 1u);
      if (k < (uint32_t)n) retry_list[k] = (uint32_t)i;
    }
    return;
  }
  if (FULL)
    g2_jac_to_words(kcof_mul(q), o);
  else
    g2_jac_to_words(q, o);
  state[i] = hbl::HASH_DONE;
}

__global__ void __launch_bounds__(64) k_hash_clear(int n, const uint32_t* __restrict__ xy, uint8_t* __restrict__ state,
                                                   uint32_t* __restrict__ out, uint32_t* __restrict__ retry_list,
                                                   uint32_t* __restrict__ retry_count) {
  hash_clear<true>(n, xy, state, out, retry_list, retry_count);
}

// The Q form saves kcof_mul's 62 doublings + 27 additions per message, not registers: cofactor_bp's second
// chain keeps p, t1, t3, the chain's base and its accumulator live (five Jacobian points, 420 words) beside
// jac_add's temporaries, so this instantiation fills the 512-register budget of one wave per SIMD as the
// full form does (profiles/r15/README.md has both reports).
__global__ void __launch_bounds__(64) k_hash_clear_bp(int n, const uint32_t* __restrict__ xy,
                                                      uint8_t* __restrict__ state, uint32_t* __restrict__ out,
                                                      uint32_t* __restrict__ retry_list,
                                                      uint32_t* __restrict__ retry_count) {
  hash_clear<false>(n, xy, state, out, retry_list, retry_count);
}

}  // namespace hb

namespace hbl {

size_t hash_work_bytes(size_t n, int rounds) {
  return (hash_count_words(rounds) + (2 + (size_t)hb::XY_WORDS + 3) * n) * sizeof(uint32_t);
}

hipError_t hash_g2(hipStream_t s, int n, int rounds, const uint8_t* seeds, void* work, uint8_t* state, void* out,
                   HashForm form) {
  if (n <= 0) return hipSuccess;
  const auto clear = form == HASH_FORM_BP ? hb::k_hash_clear_bp : hb::k_hash_clear;
  const HashWork w = hash_carve(work, (size_t)n, rounds);
  hipError_t err = hipMemsetAsync(w.counts, 0, (size_t)((uint8_t*)w.xy - (uint8_t*)w.counts), s);
  if (err != hipSuccess) return err;
  err = hipMemsetAsync(state, 0, (size_t)n, s);  // HASH_PENDING
  if (err != hipSuccess) return err;
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
  // round k reads counts[k] entries of list[k & 1] (round 0: every message) and appends its rejects
  // to list[(k + 1) & 1], counted in counts[k + 1].  The grid covers n lanes every round: the host
  // never reads a count, so the call stays asynchronous; lanes past the count leave at once.
  for (int k = 0; k < rounds; k++)
    hipLaunchKernelGGL(hb::k_hash_sample, grid, block, 0, s, n, k ? w.counts + k : nullptr, k ? w.list[k & 1] : nullptr,
                       seeds, w.pos, w.xy, state, w.list[(k + 1) & 1], w.counts + k + 1);
  uint32_t* rc = w.counts + rounds + 1;
  hipLaunchKernelGGL(clear, grid, block, 0, s, n, w.xy, state, (uint32_t*)out, w.retry, rc);
  // messages whose multiple was O (none in practice): a short series of rounds and a second clearing,
  // which also zeroes whatever is still unresolved
  const uint32_t* cnt = rc;
  const uint32_t* lst = w.retry;
  for (int k = 0; k < HASH_RETRY_ROUNDS; k++) {
    hipLaunchKernelGGL(hb::k_hash_sample, grid, block, 0, s, n, cnt, lst, seeds, w.pos, w.xy, state, w.list[k & 1],
                       rc + 1 + k);
    cnt = rc + 1 + k;
    lst = w.list[k & 1];
  }
  hipLaunchKernelGGL(clear, grid, block, 0, s, n, w.xy, state, (uint32_t*)out, (uint32_t*)nullptr,
                     (uint32_t*)nullptr);
  return hipGetLastError();
}

}  // namespace hbl
