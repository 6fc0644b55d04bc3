// HBH_IMPL_PAIR: the fused lane-pair pairing-equality kernel (gfx950).
//
// verdict[i] = e(P1_i, Q1_i) == e(P2_i, Q2_i), computed as FE(f_{|x|,Q1}(P1) f_{|x|,Q2}(-P2)) == 1 with
// one 2-pair multi-Miller loop and one final exponentiation per check -- SURVEY §8(d)'s unit of work,
// pairing 0.14's Miller loop and final exponentiation (oracle/c/bls_cpu.c miller_loop /
// final_exponentiation restate them) on the lane-pair tower of
// pfp.hpp: TWO lanes per check, so a 65,536-check batch is 2,048 waves = two waves per SIMD.
// The kernel body and the final-exponentiation chain are pair_side.hpp's (lane_verify, final_exp),
// shared with the lane-quad and lane-octo kernels; this file has the lane pair's exponentiation by x.
//
// Each G2 side is one of
//   TABLE: Q is shared by many checks (H per document, W / H_uv per ciphertext): its 68 lines are
//          computed once by k_oct_prep (k_oct_prep.hip) into a table that the checks of a wave read as broadcasts;
//   WALK : Q is per check (sigma_i, or both sides of Ciphertext::verify): T walks inside the Miller
//          loop in registers -- no per-share line table ever reaches HBM.
// The whole check is one kernel: the Fp12 state never leaves the CU.  During the final
// exponentiation one Fp12 (6 components per lane, packed to 72 words) is parked in LDS:
// 256 lanes x 288 B = 72 KiB per workgroup, two workgroups per CU.
#define HS_MULFN static __device__ __noinline__
// A wave holds 32 checks with 32 different GCD traces: the six inversions of a check (h6_inv's, and
// one per exponentiation in h_exp_tail) take the branch-free form (profiles/r13/README.md)
#ifndef HP_INV_MODE
#define HP_INV_MODE 12  // hb::INV_UNIFORM | hbs::INV_PAIR
#endif
#include "pair_side.hpp"

namespace hbs {

// ---------------------------------------------------------------- exponentiation by x
// f^|x| (|x| + 1 if PLUS1) for f in the cyclotomic subgroup.
//
// |x| has six set bits (63, 62, 60, 57, 48, 16), so f^|x| is a product of powers f^(2^k).  The
// squarings run bottom-up in Karabina's compressed form (pfp.hpp hc_sqr: six lane-pair squares
// instead of Granger-Scott's nine) up to bit EXP_TOP = 57; the compressed value is parked in per-lane
// private memory as it passes a set bit (16, 48, 57), so the squaring loop holds four coefficients
// and nothing else.  The parked powers are then decompressed with ONE Fp2 inversion (Montgomery's
// simultaneous inversion of the denominators 4 a1: prefix products, h_inv_vartime,
// back-substitution).  The four set bits from 57 up are close together: t = f^(2^57) is raised to
// |x| >> 57 = 105 = 7 x 15 with seven Granger-Scott squarings and two products (h_exp_high), which
// costs less than decompressing three more powers (measured with six squarings and three products:
// EXP_TOP = 57 against 60 and 63, profiles/r10/README.md).  f^|x| = t^105 f^(2^48) f^(2^16).
//
// The compressed form needs every parked a1 != 0.  The product of the denominators tells (one zero
// test); then the exponentiation runs the Granger-Scott square-and-multiply loop instead (h_exp_gs).
// Real inputs take that path: a pair at infinity gives f = 1, which compresses to four zeros.
constexpr int EXP_TOP = 57;                          // the last compressed squaring
constexpr uint64_t EXP_HIGH = hb::X_ABS >> EXP_TOP;  // |x| = EXP_HIGH 2^EXP_TOP + the bits below
constexpr int EXP_HIGH_BITS = 64 - EXP_TOP;
constexpr int EXP_NPARK = __builtin_popcountll(hb::X_ABS) - __builtin_popcountll(EXP_HIGH) + 1;
static_assert((hb::X_ABS & 1) == 0 && (hb::X_ABS >> 63) == 1 && (EXP_HIGH & 1) == 1 && EXP_NPARK >= 1,
              "the base is no factor of f^|x|, and the power at bit EXP_TOP is the last one parked");
struct ExpPark {
  int32_t c[EXP_NPARK][4][NL];   // the compressed powers at |x|'s set bits up to EXP_TOP, lowest first
  int32_t base[6][NL];           // f itself: the PLUS1 factor and the fallback's operand
  int32_t pre[EXP_NPARK][NL];    // prefix products of the denominators
};

HP_D void park_fp(int32_t (&d)[NL], const Fp& a) {
#pragma unroll
  for (int i = 0; i < NL; i++) d[i] = a.l[i];
}
HP_D Fp unpark_fp(const int32_t (&s)[NL]) {
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = s[i];
  return r;
}
HP_D H12 unpark12(const int32_t (&s)[6][NL]) {
  return {{unpark_fp(s[0]), unpark_fp(s[1]), unpark_fp(s[2])}, {unpark_fp(s[3]), unpark_fp(s[4]), unpark_fp(s[5])}};
}

// the cold path: square-and-multiply from the top with Granger-Scott squarings
static __device__ __noinline__ void h_exp_gs(const ExpPark& pk, bool plus1, H12& out) {
  const uint64_t e = hb::X_ABS + (plus1 ? 1 : 0);
  H12 r = unpark12(pk.base);
#pragma unroll 1
  for (int k = 62; k >= 0; k--) {
    r = h12_cyclo_sqr(r);
    if ((e >> k) & 1) r = h12_mul<LanePair>(r, unpark12(pk.base));
  }
  out = r;
}

// t^EXP_HIGH with Granger-Scott squarings.  A/B switch (profiles/r21): 1 = 105 = 7 x 15 with the
// inverses as conjugates, u = t^8 conj(t) and u^16 conj(u): seven squarings and two products; 0 =
// square-and-multiply from the top, six and three.
#ifndef HP_EXP715
#define HP_EXP715 1
#endif
HP_D H12 h_exp_high(const H12& t) {
#if HP_EXP715
  static_assert(EXP_HIGH == 105 && EXP_HIGH_BITS == 7, "the chain is 105 = (8 - 1)(16 - 1)");
  // both passes through one copy of the square and of the product: r <- r^(2^(3 + pass)) / b, b <- r.
  // Bounds: b is reduced (|.| < 2p, normalised) -- t, hc_decompress's output, in pass 0 and an h12_mul
  // output in pass 1 -- so h12_conj(b)'s fp_neg (0 - x, one carry pass) is normalised with |.| < 2p,
  // and r is an h12_cyclo_sqr output, reduced: both are h12_mul's "inputs reduced", whose sums of two
  // components stay normalised and < 4p, h6_mul's input bound.
  H12 r = t, b = t;
#pragma unroll 1
  for (int pass = 0; pass < 2; pass++) {
#pragma unroll 1
    for (int k = 0; k < 3 + pass; k++) r = h12_cyclo_sqr(r);
    r = h12_mul<LanePair>(r, h12_conj(b));
    b = r;
  }
  return r;
#else
  H12 r = t;
#pragma unroll 1
  for (int k = EXP_HIGH_BITS - 2; k >= 0; k--) {
    r = h12_cyclo_sqr(r);
    if ((EXP_HIGH >> k) & 1) r = h12_mul<LanePair>(r, t);
  }
  return r;
#endif
}

// decompress the parked powers with one shared inversion, raise the highest to EXP_HIGH and
// multiply them (and f if plus1); false, with out untouched, if a denominator is zero.  Not inlined:
// the register allocator sees a call boundary, as at the products, and there is one copy for the
// five exponentiations.
static __device__ __noinline__ bool h_exp_tail(ExpPark& pk, bool plus1, H12& out) {
  Fp P;
#pragma unroll 1
  for (int j = 0; j < EXP_NPARK; j++) {
    const Fp d = hc_denom(unpark_fp(pk.c[j][0]));
    if (j == 0) P = d; else P = h_mul(P, d);
    park_fp(pk.pre[j], P);
  }
  if (h_is_zero(P)) return false;  // the same on both lanes of the pair (lp_both)
  Fp I = fp_reduce(h_inv_vartime<HP_INV_MODE>(P));
  H12 acc;
#pragma unroll 1
  for (int j = EXP_NPARK - 1; j >= (plus1 ? -1 : 0); j--) {
    H12 E;
    if (j >= 0) {
      const HC c = {unpark_fp(pk.c[j][0]), unpark_fp(pk.c[j][1]), unpark_fp(pk.c[j][2]), unpark_fp(pk.c[j][3])};
      Fp di = I;
      if (j > 0) {
        di = h_mul(I, unpark_fp(pk.pre[j - 1]));
        I = h_mul(I, hc_denom(c.a1));
      }
      E = hc_decompress(c, di);
    } else {
      E = unpark12(pk.base);
    }
    if (j == EXP_NPARK - 1) acc = h_exp_high(E); else acc = h12_mul<LanePair>(acc, E);
  }
  out = acc;
  return true;
}

template <bool PLUS1>
HP_D H12 h_exp_abs_x(const H12& base, ExpPark& pk) {
  park_fp(pk.base[0], base.c0.c0); park_fp(pk.base[1], base.c0.c1); park_fp(pk.base[2], base.c0.c2);
  park_fp(pk.base[3], base.c1.c0); park_fp(pk.base[4], base.c1.c1); park_fp(pk.base[5], base.c1.c2);
  HC c = hc_compress(base);
  int slot = 0;
#pragma unroll 1
  for (int k = 1; k <= EXP_TOP; k++) {
    c = hc_sqr(c);
    if ((hb::X_ABS >> k) & 1) {  // EXP_NPARK times
      park_fp(pk.c[slot][0], c.a1); park_fp(pk.c[slot][1], c.a2);
      park_fp(pk.c[slot][2], c.a4); park_fp(pk.c[slot][3], c.a5);
      slot++;
    }
  }
  H12 r;
  if (!h_exp_tail(pk, PLUS1, r)) h_exp_gs(pk, PLUS1, r);
  return r;
}
// the lane pair's exponentiation by x for final_exp (pair_side.hpp): one parking area for the five
struct ExpCompressed {
  ExpPark pk;
  HP_D H12 x(const H12& f) { return h12_conj(h_exp_abs_x<false>(f, pk)); }
  HP_D H12 xm1(const H12& f) { return h12_conj(h_exp_abs_x<true>(f, pk)); }
};

// GEN: 0 = both P read per check, 1 = P1 is the generator, 2 = P2 is the generator
template <bool W1, bool W2, int GEN>
__global__ void __launch_bounds__(256, 2) k_pair_verify(PairArgs a) {
  extern __shared__ uint32_t stash_lds[];
  lane_verify<LanePair, ExpCompressed, W1, W2, GEN>(a, stash_lds);
}

}  // namespace hbs

namespace hbl {

struct PairKernels {
  static constexpr int LANES = hbs::LanePair::LANES;
  template <bool W1, bool W2, int GEN>
  static constexpr auto kernel = hbs::k_pair_verify<W1, W2, GEN>;
};

size_t pair_table_bytes(size_t nq) { return nq * (size_t)hbs::PAIR_STEPS * hbs::LINE_Q4 * 16; }

hipError_t pair_verify(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                       uint8_t* verdict, uint32_t* value_out) {
  if (n <= 0) return hipSuccess;
  const int gen = pair_gen_mode(d1, d2);
  if (gen == 1) return lane_launch<PairKernels, 1>(s, n, d1, d2, flags, verdict, value_out);
  if (gen == 2) return lane_launch<PairKernels, 2>(s, n, d1, d2, flags, verdict, value_out);
  return lane_launch<PairKernels, 0>(s, n, d1, d2, flags, verdict, value_out);
}

}  // namespace hbl
