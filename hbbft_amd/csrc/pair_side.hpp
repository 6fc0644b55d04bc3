// Shared by the lane-pair (k_pair.hip), lane-quad (k_quad.hpp) and lane-octo (k_oct.hpp) pairing
// kernels: the LDS stash of the final exponentiation, the Miller-loop sides (line tables, walked G2
// points, P), and the one kernel body, final-exponentiation chain and launcher of the three, each
// written over a width policy (pfp.hpp LanePair, qfp.hpp LaneQuad, ofp.hpp LaneOcto).
#pragma once
#include "launch.hpp"
#include "qfp.hpp"

namespace hbs {

constexpr int PAIR_STEPS = 68;   // 63 doubling + 5 addition steps of |x|
constexpr int PL_Q4 = 11;        // 16-byte chunks per (line, lane component): c0, c1, c4 = 42 words (+2 pad)
constexpr int STASH_WORDS = 72;  // 6 packed Fp per lane
static_assert(PARK_WORDS <= STASH_WORDS, "the Miller loop parks T and P in the stash (pfp.hpp PairPark)");

// ---------------------------------------------------------------- LDS stash (6 components)
// component reduced to [0, 2p) (< 2^382) and packed 14 x 28 -> 12 x 32 bits; Montgomery form kept
HP_D void stash_fp(uint32_t* __restrict__ s, const Fp& a) {
  const Fp r = fp_reduce(a);
  Fp rp = fp_addl(r, fp_const(P_L));
  fp_norm(rp);
  const Fp c = (r.l[NL - 1] < 0) ? rp : r;
#pragma unroll
  for (int w = 0; w < 12; w++) {
    const int bit = 32 * w, li = bit / 28, sh = bit % 28;
    uint64_t v = (uint64_t)(uint32_t)c.l[li] >> sh;
    if (li + 1 < NL) v |= (uint64_t)(uint32_t)c.l[li + 1] << (28 - sh);
    if (li + 2 < NL) v |= (uint64_t)(uint32_t)c.l[li + 2] << (56 - sh);
    s[w * 256] = (uint32_t)v;
  }
}
HP_D Fp unstash_fp(const uint32_t* __restrict__ s) {
  uint32_t w[12];
#pragma unroll
  for (int k = 0; k < 12; k++) w[k] = s[k * 256];
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const int bit = 28 * i, wi = bit >> 5, sh = bit & 31;
    uint64_t v = w[wi];
    if (wi + 1 < 12) v |= (uint64_t)w[wi + 1] << 32;
    r.l[i] = (int32_t)((uint32_t)(v >> sh) & (uint32_t)MASK28);
  }
  return r;
}
// s = this lane's column of the workgroup's stash (word k of lane l at stash[k * 256 + l])
HP_D void stash12(uint32_t* __restrict__ s, const H12& f) {
  stash_fp(s + 0 * 12 * 256, f.c0.c0);
  stash_fp(s + 1 * 12 * 256, f.c0.c1);
  stash_fp(s + 2 * 12 * 256, f.c0.c2);
  stash_fp(s + 3 * 12 * 256, f.c1.c0);
  stash_fp(s + 4 * 12 * 256, f.c1.c1);
  stash_fp(s + 5 * 12 * 256, f.c1.c2);
}
HP_D H12 unstash12(const uint32_t* __restrict__ s) {
  H12 f;
  f.c0.c0 = unstash_fp(s + 0 * 12 * 256);
  f.c0.c1 = unstash_fp(s + 1 * 12 * 256);
  f.c0.c2 = unstash_fp(s + 2 * 12 * 256);
  f.c1.c0 = unstash_fp(s + 3 * 12 * 256);
  f.c1.c1 = unstash_fp(s + 4 * 12 * 256);
  f.c1.c2 = unstash_fp(s + 5 * 12 * 256);
  return f;
}

// ---------------------------------------------------------------- Miller-loop sides
struct PairSide {
  const uint32_t* p;    // G1 points, 24 words each; nullptr: the generator g1 for every check
  const uint32_t* q;    // WALK: G2 points, 48 words each
  const int4* lines;    // TABLE: line tables written by k_oct_prep
  const uint8_t* qinf;  // TABLE: 1 = table point at infinity
  const uint32_t* idx;  // Q index per check (nullptr = identity)
  uint32_t nq;          // number of Q points / tables
};

template <class ST>
HP_D void side_q(const PairSide& s, const ST& st, Fp& xQ, Fp& yQ) {
  h_g2_load(s.q + (size_t)st.q * 48, xQ, yQ);
  if (st.qinf) {
    xQ = h_one();
    yQ = h_one();
  }
}

template <bool WALK, bool GEN, class ST>
HP_D bool side_init(const PairSide& s, int i, bool negate, ST& st) {
  st.q = s.idx ? s.idx[i] : (uint32_t)i;
  if (st.q >= s.nq) return false;
  bool pinf;
  if (GEN) {
    pinf = false;
  } else if (s.p) {
    const uint32_t* w = s.p + (size_t)i * 24;
    pinf = words_zero(w, 24);
    st.xP = fp_from_words(w);
    st.yP = fp_from_words(w + 12);
  } else {
    pinf = false;
    st.xP = fp_const(hb::G1X_M);
    st.yP = fp_const(hb::G1Y_M);
  }
  if (!GEN && negate) st.yP = fp_neg(st.yP);
  if (WALK) {
    const uint32_t* w = s.q + (size_t)st.q * 48;
    st.qinf = lp_both(words_zero(w + (lp_even() ? 0 : 12), 12) && words_zero(w + (lp_even() ? 24 : 36), 12));
    Fp xQ, yQ;
    side_q(s, st, xQ, yQ);  // dummy walk from (1, 1) when Q = O: the pair is masked out
    st.T = {xQ, yQ, h_one()};  // Z = 1 in Jacobian and in homogeneous coordinates alike
  } else {
    st.qinf = s.qinf[st.q] != 0;
  }
  st.act = !pinf && !st.qinf;
  return true;
}

// ---------------------------------------------------------------- line tables
// A table holds, per shared G2 point, the PAIR_STEPS raw lines of its walk.  Entry e = q PAIR_STEPS +
// step is two runs of PL_Q4 16-byte chunks, one per lane component (even lane first): c0, c1, c4 as
// 3 x 14 signed limbs and two words of padding.  k_oct_prep writes it, every verify kernel reads it.
// line_at: the offset in chunks of this lane's run of entry e; line_load / line_store take the run.
constexpr int LINE_Q4 = 2 * PL_Q4;  // chunks per entry
HP_D size_t line_at(size_t e) { return e * LINE_Q4 + (lp_even() ? 0 : PL_Q4); }
HP_D HLine line_load(const int4* __restrict__ p) {
  int32_t w[4 * PL_Q4];
#pragma unroll
  for (int k = 0; k < PL_Q4; k++) {
    const int4 v = p[k];
    w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
  }
  HLine l;
#pragma unroll
  for (int j = 0; j < NL; j++) {
    l.c0.l[j] = w[j];
    l.c1.l[j] = w[NL + j];
    l.c4.l[j] = w[2 * NL + j];
  }
  return l;
}
HP_D void line_store(int4* __restrict__ p, const HLine& l) {
  int32_t w[4 * PL_Q4];
#pragma unroll
  for (int j = 0; j < NL; j++) {
    w[j] = l.c0.l[j];
    w[NL + j] = l.c1.l[j];
    w[2 * NL + j] = l.c4.l[j];
  }
  w[3 * NL] = 0;
  w[3 * NL + 1] = 0;
#pragma unroll
  for (int k = 0; k < PL_Q4; k++) p[k] = make_int4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// a side's raw line of this step: the walk of T (WALK; SIDE's T comes from and goes back to the
// parking hook pk) or the table entry (TABLE)
template <class G, bool WALK, bool DBL, int SIDE, class ST, class PK>
HP_D HLine side_raw(const PairSide& s, ST& st, int step, const PK& pk) {
  if constexpr (!WALK) {
    return line_load(s.lines + line_at(st.q * PAIR_STEPS + step));
  } else if constexpr (DBL) {
    return pk.template walk<SIDE>(st, [&](typename G::Walk& T) HS_LAMBDA { return G::dbl_step(T); });
  } else {
    Fp xQ, yQ;
    side_q(s, st, xQ, yQ);
    return pk.template walk<SIDE>(st, [&](typename G::Walk& T) HS_LAMBDA { return G::add_step(T, xQ, yQ); });
  }
}

struct PairArgs {
  int n;
  PairSide s1, s2;
  int flags;            // bit 0: negate P2 (pairing equality); bit 1: conjugate f (single pairing value)
  uint8_t* verdict;     // 1 byte per check (may be null)
  uint32_t* value_out;  // 144 canonical words per check (may be null)
};


// ---------------------------------------------------------------- final exponentiation
// f^|x| (|x| + 1 if PLUS1) for f in the cyclotomic subgroup: square-and-multiply from the top with
// Granger-Scott squarings
template <class G, bool PLUS1>
HP_D H12 exp_abs_x_gs(const H12& base) {
  const uint64_t e = PLUS1 ? hb::X_ABS + 1 : hb::X_ABS;
  H12 r = base;
#pragma unroll 1
  for (int k = 62; k >= 0; k--) {
    r = G::cyclo_sqr(r);
    if ((e >> k) & 1) r = h12_mul<G>(r, base);
  }
  return r;
}
// How final_exp takes f^x and f^(x-1): x < 0, so f^x = conj(f^|x|), f^(x-1) = conj(f^(|x|+1)).  This
// one is the plain loop; k_pair.hip has the lane pair's.
template <class G>
struct ExpGs {
  HP_D H12 x(const H12& f) { return h12_conj(exp_abs_x_gs<G, false>(f)); }
  HP_D H12 xm1(const H12& f) { return h12_conj(exp_abs_x_gs<G, true>(f)); }
};

// e = f^(3 (p^12 - 1) / r), pairing 0.14's hard-part chain (x3) reordered so that at most one
// Fp12 has to outlive an exponentiation (it waits in the LDS stash):
//   g = f^((p^6 - 1)(p^2 + 1));  a = (g^(x-1))^(x-1);  b = a^x frob1(a);
//   w = frob2(b) conj(b) g^3;    e = (b^x)^x w
// Exp: the exponentiation by x (ExpGs, or one with state of its own that the five share)
template <class G, class Exp>
HP_D H12 final_exp(const H12& f, uint32_t* __restrict__ stash) {
  const H12 f1 = h12_mul<G>(h12_conj(f), h12_inv<G>(f));
  const H12 g = h12_mul<G>(G::frob2(f1), f1);
  stash12(stash, g);
  Exp ex;
  H12 a = ex.xm1(ex.xm1(g));
  const H12 b = h12_mul<G>(ex.x(a), G::frob1(a));
  {
    const H12 gs = unstash12(stash);
    const H12 w = h12_mul<G>(h12_mul<G>(G::frob2(b), h12_conj(b)), h12_mul<G>(G::cyclo_sqr(gs), gs));
    stash12(stash, w);
  }
  const H12 c = ex.x(ex.x(b));
  return h12_mul<G>(c, unstash12(stash));
}

// ---------------------------------------------------------------- the pairing-equality check
// verdict[i] = e(P1_i, Q1_i) == e(P2_i, Q2_i), computed as FE(f_{|x|,Q1}(P1) f_{|x|,Q2}(-P2)) == 1 with
// one 2-pair multi-Miller loop and one final exponentiation, on G::LANES lanes per check: the body of
// k_pair_verify, k_quad_verify and k_oct_verify.  W1 / W2: the side WALKs (else TABLE); GEN: 0 = both
// P read per check, 1 = P1 is the generator, 2 = P2 is the generator.  stash: the workgroup's LDS
// stash.
template <class G, class Exp, bool W1, bool W2, int GEN>
HP_D void lane_verify(const PairArgs& a, uint32_t* stash) {
  const int i = (int)((blockIdx.x * 256u + threadIdx.x) / (unsigned)G::LANES);
  if (i >= a.n) return;  // the lanes of a check leave together
  constexpr bool G1 = GEN == 1, G2 = GEN == 2;
  const bool neg2 = (a.flags & 1) != 0;
  SideStateT<typename G::Walk> A, B;
  const bool ok1 = side_init<W1, G1>(a.s1, i, false, A);
  const bool ok2 = side_init<W2, G2>(a.s2, i, neg2, B);
  if (!ok1 || !ok2) {  // index out of range: reject, never read past a table
    if (G::leader() && a.verdict) a.verdict[i] = 0;
    return;
  }
  // T and P wait in the stash between their uses (LanePair; the first stash12 comes after the loop).
  // Lanes that left above never touch it.
  const typename G::template Park<W1, W2, GEN> pk(stash + threadIdx.x);
  pk.init(A, B);
  constexpr bool WF = !W1 && W2;  // TABLE / WALK: a width may walk side B first
  H12 f = h12_one();
  int step = 0;
#pragma unroll 1
  for (int b = 62; b >= 0; b--) {
    // the two sides' lines are multiplied together first, then into f (h12_mul_lines)
    if (b != 62) f = h12_sqr<G>(f);
    {
      HLine la, lb;
      G::template lines_at_p<G1, G2, WF>([&]() HS_LAMBDA { return side_raw<G, W1, true, 0>(a.s1, A, step, pk); },
                                         [&]() HS_LAMBDA { return side_raw<G, W2, true, 1>(a.s2, B, step, pk); }, A, B,
                                         neg2, la, lb, pk);
      // b == 62: f is still 1, and a width may take the line product as f
      constexpr bool FL = G::template first_line<W1, W2>();
      f = h12_mul_lines<G>(f, la.c0, la.c1, la.c4, lb.c0, lb.c1, lb.c4, FL && b == 62);
    }
    step++;
    if ((hb::X_ABS >> b) & 1) {
      HLine la, lb;
      G::template lines_at_p<G1, G2, WF>([&]() HS_LAMBDA { return side_raw<G, W1, false, 0>(a.s1, A, step, pk); },
                                         [&]() HS_LAMBDA { return side_raw<G, W2, false, 1>(a.s2, B, step, pk); }, A, B,
                                         neg2, la, lb, pk);
      f = h12_mul_lines<G>(f, la.c0, la.c1, la.c4, lb.c0, lb.c1, lb.c4);
      step++;
    }
  }
  if (a.flags & 2) f = h12_conj(f);
  const H12 e = final_exp<G, Exp>(f, stash + threadIdx.x);
  if (a.value_out && G::value_writer()) {
    uint32_t* o = a.value_out + (size_t)i * 144 + (lp_even() ? 0 : 12);
    fp_to_words(e.c0.c0, o + 0);
    fp_to_words(e.c0.c1, o + 24);
    fp_to_words(e.c0.c2, o + 48);
    fp_to_words(e.c1.c0, o + 72);
    fp_to_words(e.c1.c1, o + 96);
    fp_to_words(e.c1.c2, o + 120);
  }
  const bool one = h12_is_one(e);
  if (G::leader() && a.verdict) a.verdict[i] = one ? 1 : 0;
}

// ---------------------------------------------------------------- the Miller product
// The batched checks' lane kernel (hbh_verify_signatures_batched, hbh_verify_ciphertexts_uv_batched,
// hbh_dbg_pairing_product): no final exponentiation here.  A group of G::LANES lanes takes TWO
// CONSECUTIVE ITEMS (P_i, Q_i), (P_i+1, Q_i+1) as the two sides of lane_verify's loop (both WALK, both P
// read), so a 256-thread workgroup -- a tile -- holds T = 2 * 256 / G::LANES items; the Miller values of
// the tile's 256 / G::LANES slots are multiplied up a binary tree through the LDS stash, and the tile's
// product is written as 144 canonical words in the layout wave_prod_fe reads (k_wave.hpp: the w-basis,
// component k at word 24 k; tower component c0.cj is k = 2 j, c1.cj is k = 2 j + 1).  An item past n, or
// with P = O or Q = O, is an inactive pair and contributes 1 (side_init's act); every lane stays to the
// last barrier.  The value is the raw product of f_{|x|,Q}(P), times subfield factors that the final
// exponentiation removes: FE(conj(value)) = prod e(P_i, Q_i)^3.
struct MillerProdArgs {
  int n;              // items; tile b takes the items [b T, min(n, (b + 1) T))
  const uint32_t* p;  // G1 points, 24 words per item
  const uint32_t* q;  // G2 points, 48 words per item
  int tpg, nf;        // tile b is value (b / tpg) * nf + b % tpg of out (tpg tiles per group, nf values per group)
  uint32_t* out;      // 144 words per value
};

template <class G>
HP_D void lane_miller_prod(const MillerProdArgs& a, uint32_t* stash) {
  constexpr int SLOTS = 256 / G::LANES;
  const int slot = (int)threadIdx.x / G::LANES;
  const int i0 = 2 * ((int)blockIdx.x * SLOTS + slot), i1 = i0 + 1, last = a.n - 1;
  const PairSide sd = {a.p, a.q, nullptr, nullptr, nullptr, (uint32_t)a.n};
  SideStateT<typename G::Walk> A, B;
  // an item past n reads item n - 1 and is masked out: its lanes walk along to the barriers
  side_init<true, false>(sd, i0 < last ? i0 : last, false, A);
  side_init<true, false>(sd, i1 < last ? i1 : last, false, B);
  A.act = A.act && i0 < a.n;
  B.act = B.act && i1 < a.n;
  uint32_t* col = stash + threadIdx.x;
  const typename G::template Park<true, true, 0> pk(col);
  pk.init(A, B);
  H12 f = h12_one();
  int step = 0;
#pragma unroll 1
  for (int b = 62; b >= 0; b--) {
    if (b != 62) f = h12_sqr<G>(f);
    {
      HLine la, lb;
      G::template lines_at_p<false, false, false>([&]() HS_LAMBDA { return side_raw<G, true, true, 0>(sd, A, step, pk); },
                                                  [&]() HS_LAMBDA { return side_raw<G, true, true, 1>(sd, B, step, pk); },
                                                  A, B, false, la, lb, pk);
      constexpr bool FL = G::template first_line<true, true>();
      f = h12_mul_lines<G>(f, la.c0, la.c1, la.c4, lb.c0, lb.c1, lb.c4, FL && b == 62);
    }
    step++;
    if ((hb::X_ABS >> b) & 1) {
      HLine la, lb;
      G::template lines_at_p<false, false, false>([&]() HS_LAMBDA { return side_raw<G, true, false, 0>(sd, A, step, pk); },
                                                  [&]() HS_LAMBDA { return side_raw<G, true, false, 1>(sd, B, step, pk); },
                                                  A, B, false, la, lb, pk);
      f = h12_mul_lines<G>(f, la.c0, la.c1, la.c4, lb.c0, lb.c1, lb.c4);
      step++;
    }
  }
  // The tree: a slot's value waits in its lanes' columns (reduced to [0, 2p) by stash_fp: h12_mul's
  // input bound).  At level L the slots that are multiples of 2^(L+1) multiply in slot + 2^L, whose
  // columns nobody writes at this level, so one barrier per level orders writes and reads.  The lanes
  // of a slot branch together (the cross-lane moves of a product stay inside the slot).
  stash12(col, f);
  __syncthreads();
#pragma unroll 1
  for (int L = 0; (1 << L) < SLOTS; L++) {
    if ((slot & ((2 << L) - 1)) == 0) {
      const H12 g = unstash12(col + (G::LANES << L));
      const H12 m = h12_mul<G>(unstash12(col), g);
      stash12(col, m);
    }
    __syncthreads();
  }
  if (slot == 0 && G::value_writer()) {
    const H12 e = unstash12(col);
    uint32_t* o = a.out + ((size_t)(blockIdx.x / a.tpg) * a.nf + blockIdx.x % a.tpg) * 144 + (lp_even() ? 0 : 12);
    fp_to_words(e.c0.c0, o + 0);
    fp_to_words(e.c1.c0, o + 24);
    fp_to_words(e.c0.c1, o + 48);
    fp_to_words(e.c1.c1, o + 72);
    fp_to_words(e.c0.c2, o + 96);
    fp_to_words(e.c1.c2, o + 120);
  }
}

}  // namespace hbs

// ---------------------------------------------------------------- launching
namespace hbl {

// the Miller-product kernel K (a width's k_*_miller_prod) over ntile tiles of 2 * 256 / LANES items
template <class K>
hipError_t miller_prod_launch(K kernel, hipStream_t s, int ntile, int n, const void* p, const void* q, int tpg, int nf,
                              uint32_t* out) {
  if (ntile <= 0) return hipSuccess;
  if (n <= 0 || tpg <= 0 || nf < tpg || !p || !q || !out) return hipErrorInvalidValue;
  const hbs::MillerProdArgs a = {n, (const uint32_t*)p, (const uint32_t*)q, tpg, nf, out};
  hipLaunchKernelGGL(kernel, dim3((unsigned)ntile), dim3(256), (size_t)hbs::STASH_WORDS * 256 * 4, s, a);
  return hipGetLastError();
}

inline hbs::PairArgs pair_args(int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags, uint8_t* verdict,
                               uint32_t* value_out) {
  hbs::PairArgs a;
  a.n = n;
  const PairSideDesc* d[2] = {&d1, &d2};
  hbs::PairSide* o[2] = {&a.s1, &a.s2};
  for (int k = 0; k < 2; k++) {
    o[k]->p = (const uint32_t*)d[k]->p;
    o[k]->q = (const uint32_t*)d[k]->q;
    o[k]->lines = (const int4*)d[k]->lines;
    o[k]->qinf = d[k]->qinf;
    o[k]->idx = d[k]->idx;
    o[k]->nq = (uint32_t)d[k]->nq;
  }
  a.flags = flags;
  a.verdict = verdict;
  a.value_out = value_out;
  return a;
}

// a null P on exactly one side selects the generator instantiation (1 or 2); both null keeps the
// run-time generator path of side_init (P1 and P2 held in registers)
inline int pair_gen_mode(const PairSideDesc& d1, const PairSideDesc& d2) {
  return (d1.p == nullptr) == (d2.p == nullptr) ? 0 : (d1.p == nullptr ? 1 : 2);
}

// launch the WALK / TABLE variant that the two sides ask for, of generator mode GEN.  K names a
// width's kernels: K::LANES and K::kernel<W1, W2, GEN>.
template <class K, int GEN>
hipError_t lane_launch(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                       uint8_t* verdict, uint32_t* value_out) {
  const hbs::PairArgs a = pair_args(n, d1, d2, flags, verdict, value_out);
  const dim3 grid((unsigned)((K::LANES * (size_t)n + 255) / 256)), block(256);
  const size_t lds = (size_t)hbs::STASH_WORDS * 256 * 4;
  const bool w1 = d1.lines == nullptr, w2 = d2.lines == nullptr;
  if (w1 && w2)
    hipLaunchKernelGGL((K::template kernel<true, true, GEN>), grid, block, lds, s, a);
  else if (w1)
    hipLaunchKernelGGL((K::template kernel<true, false, GEN>), grid, block, lds, s, a);
  else if (w2)
    hipLaunchKernelGGL((K::template kernel<false, true, GEN>), grid, block, lds, s, a);
  else
    hipLaunchKernelGGL((K::template kernel<false, false, GEN>), grid, block, lds, s, a);
  return hipGetLastError();
}

}  // namespace hbl
