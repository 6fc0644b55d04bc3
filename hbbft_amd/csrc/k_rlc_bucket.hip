// Bucket form of the grouped random-combination sums (gfx950): the tile sums of k_group_sum (k_rlc.hip)
// by a windowed bucket method, for hbh_engine_set_group_sum_impl(HBH_GSUM_BUCKET).  Same inputs, same
// Jacobian tile record, so k_group_join and everything after it are shared.  The chain form runs one
// double-and-add chain per (item, digit) and pays the doublings once per item; this one pays them once
// per tile: with two-bit windows (group_bucket.hpp)
//     tile sum = sum_w 4^w B_w,   B_w = sum over the tile's terms of digit_w(term) * point(term).
// One workgroup (one wave) per tile:
//   stage       one thread per item, gb::stage_items per round: the item's terms (G1: P; G2: P, -psi(P)
//               and, for r >= |x|^2, psi^2(P)) to internal form and its digits, once, into LDS.  An item
//               at infinity or a perm entry >= n gets all-zero digits, so it contributes nothing.
//   accumulate  lane = window; three buckets (digits 1, 2, 3) in LDS, indexed by the digit.  For each
//               staged term with a nonzero digit d: bucket[d] += term (jac_add_affine: O, P + P and
//               P - P occur, a tile may hold one point several times).  Trip count uniform.
//   reduce      B = (b1 + b3) + 2 (b2 + b3) per lane.
//   tail        gb::TAIL_SEGS lanes each run Horner over their windows and shift by their weight; a tree
//               adds the segment sums; thread 0 writes the tile's Jacobian sum.
// Critical path of a tile of L items, in group operations (one lane; the lanes of the wave run in step):
//   G1: L madd + (3 add + 1 dbl) + [7 (2 dbl + add) + 112 dbl] + 3 add  = L madd + 127 dbl + 13 add
//   G2: 3 L madd slots (P, -psi(P): every slot taken; psi^2(P): only for r >= |x|^2, a third of them)
//       + (3 add + 1 dbl) + [3 (2 dbl + add) + 56 dbl] + 3 add           = ~2.3 L madd + 63 dbl + 9 add
// against L-independent 128 dbl + 128 masked madd (G1) and 64 dbl + 64 masked madd (+ 1) per chain plus
// the 7- or 8-level addition tree of the chain form.  The doubling tail is the floor of either form.
// One slice per window (gb::SLICES): a second slice of Jacobian buckets is another 32 KiB of LDS per
// tile, which halves the tiles a CU holds and gives back what the shorter term loop gains; so the G2
// term loop is the long pole of this form (measured: profiles/r17/README.md).
// Scalars and points are public: variable time throughout.  Host launchers at the bottom.
#define HB_FP_LATENCY 1
#include <hip/hip_runtime.h>

#include "curve.hpp"
#include "endo.hpp"
#include "group_bucket.hpp"
#include "group_plan.hpp"
#include "launch.hpp"

namespace hb {

template <class F>
struct Aff {
  F x, y;
};
// A bucket in LDS (gb::slot_bytes)
template <class F>
struct alignas(16) Slot {
  Jac<F> p;
};

// The terms of one item in internal form; false when the item is the point at infinity
template <class F>
struct BucketKind;
template <>
struct BucketKind<Fp> {
  static constexpr bool G2 = false;
  static constexpr int WORDS = G1_WORDS;
  __device__ static bool stage(const uint32_t* w, const gb::Digits&, Aff<Fp>* out) {
    bool inf;
    load_g1(w, out[0].x, out[0].y, inf);
    return !inf;
  }
};
template <>
struct BucketKind<Fp2> {
  static constexpr bool G2 = true;
  static constexpr int WORDS = G2_WORDS;
  __device__ static bool stage(const uint32_t* w, const gb::Digits& d, Aff<Fp2>* out) {
    Fp2 x, y;
    bool inf;
    load_g2(w, x, y, inf);
    if (inf) return false;
    out[0].x = x;
    out[0].y = y;
    x = psi_x(x);  // -psi(P)
    y = f2_neg(psi_y(y));
    out[1].x = x;
    out[1].y = y;
    if (d.top) {  // psi^2(P) = -psi(-psi(P)); its slot is read only under a nonzero digit
      out[2].x = psi_x(x);
      out[2].y = f2_neg(psi_y(y));
    }
    return true;
  }
};

template <class F>
__global__ void __launch_bounds__(gb::THREADS) k_group_bucket(int ntile, int n, const uint32_t* __restrict__ pts,
                                                              const uint32_t* __restrict__ scalars,
                                                              const uint32_t* __restrict__ perm,
                                                              const uint32_t* __restrict__ tile_off,
                                                              const uint32_t* __restrict__ tile_len,
                                                              uint32_t* __restrict__ tile_out) {
  using K = BucketKind<F>;
  constexpr bool G2 = K::G2;
  constexpr int NW = gb::windows(G2), NLANE = gb::lanes(G2), NT = gb::terms_per_item(G2), SI = gb::stage_items(G2);
  constexpr int NB = gb::NBUCKET;
  static_assert(NW * gb::SLICES == NLANE, "lane = (window, slice)");
  static_assert(sizeof(Aff<F>) * 3 == sizeof(Jac<F>) * 2, "stage_bytes counts an affine term as 2/3 of a Jacobian one");
  static_assert(gb::lds_bytes(G2, sizeof(Jac<F>)) <= gb::LDS_BUDGET, "LDS per workgroup");
  static_assert(gb::bucket_bytes(G2, sizeof(Jac<F>)) % 8 == 0 && (SI * NT * sizeof(Aff<F>)) % 8 == 0, "Digits alignment");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  static_assert(sizeof(Slot<F>) == gb::slot_bytes(sizeof(Jac<F>)), "bucket_bytes counts these slots");
  Slot<F>* bk = reinterpret_cast<Slot<F>*>(smem_raw);                                // [lane][NB]
  Aff<F>* st = reinterpret_cast<Aff<F>*>(smem_raw + gb::bucket_bytes(G2, sizeof(Jac<F>)));  // [SI][NT]
  gb::Digits* dg = reinterpret_cast<gb::Digits*>(st + SI * NT);                      // [SI]

  const int tile = blockIdx.x;
  if (tile >= ntile) return;  // uniform per workgroup
  const int t = threadIdx.x;
  const bool lane_on = t < NLANE;
  const int win = gb::lane_window(G2, t), slice = gb::lane_slice(G2, t);
  const int len = (int)(tile_len[tile] < GROUP_TILE ? tile_len[tile] : GROUP_TILE);
  const uint32_t off = tile_off[tile];
  if (lane_on) {
#pragma unroll 1
    for (int b = 0; b < NB; b++) bk[t * NB + b].p = jac_zero<F>();
  }
#pragma unroll 1
  for (int base = 0; base < len; base += SI) {  // uniform trip count
    __syncthreads();                            // the previous round's terms are no longer read
    if (t < SI) {
      gb::Digits d = gb::digits_zero();
      if (base + t < len) {
        const uint32_t pos = off + (uint32_t)(base + t);
        const uint32_t item = pos < (uint32_t)n ? perm[pos] : 0xffffffffu;
        if (item < (uint32_t)n) {
          uint32_t r[4];
          for (int j = 0; j < 4; j++) r[j] = scalars[(size_t)item * 4 + j];
          d = gb::digits_of(G2, r);
          if (!K::stage(pts + (size_t)item * K::WORDS, d, st + t * NT)) d = gb::digits_zero();
        }
      }
      dg[t] = d;
    }
    __syncthreads();
    const int cnt = (len - base < SI ? len - base : SI) * NT;
    if (lane_on) {
#pragma unroll 1
      for (int k = slice; k < cnt; k += gb::SLICES) {
        const uint32_t d = gb::digit(dg[k / NT], G2, k % NT, win);
        if (d) {
          Jac<F>* b = &bk[t * NB + (int)d - 1].p;
          *b = jac_add_affine(*b, st[k].x, st[k].y);
        }
      }
    }
  }
  // reduce: B = b1 + 2 b2 + 3 b3 into the lane's first bucket, then the slices of a window
  if (lane_on) {
    const Jac<F> b3 = bk[t * NB + 2].p;
    const Jac<F> hi = jac_add(bk[t * NB + 1].p, b3);
    bk[t * NB].p = jac_add(jac_add(bk[t * NB].p, b3), jac_dbl(hi));
  }
  __syncthreads();
  if (gb::SLICES > 1) {
    if (lane_on && slice == 0) {
      Jac<F> acc = bk[t * NB].p;
#pragma unroll 1
      for (int s = 1; s < gb::SLICES; s++) acc = jac_add(acc, bk[gb::lane_of(G2, win, s) * NB].p);
      bk[t * NB].p = acc;
    }
    __syncthreads();
  }
  // tail: segment sums into the second bucket of lanes 0 .. TAIL_SEGS - 1 (dead since the reduction)
  if (t < gb::TAIL_SEGS) {
    const int lo = gb::seg_lo(G2, t), hi = gb::seg_hi(G2, t);
    Jac<F> acc = bk[gb::lane_of(G2, hi - 1, 0) * NB].p;
#pragma unroll 1
    for (int w = hi - 2; w >= lo; w--) {
      acc = jac_dbl(jac_dbl(acc));
      acc = jac_add(acc, bk[gb::lane_of(G2, w, 0) * NB].p);
    }
#pragma unroll 1
    for (int j = gb::seg_shift(G2, t); j > 0; j--) acc = jac_dbl(acc);
    bk[t * NB + 1].p = acc;
  }
  __syncthreads();
#pragma unroll 1
  for (int h = gb::TAIL_SEGS / 2; h > 0; h >>= 1) {
    if (t < h) bk[t * NB + 1].p = jac_add(bk[t * NB + 1].p, bk[(t + h) * NB + 1].p);
    __syncthreads();
  }
  if (t == 0) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&bk[1].p);
    uint32_t* dst = tile_out + (size_t)tile * (sizeof(Jac<F>) / 4);
    for (int i = 0; i < (int)(sizeof(Jac<F>) / 4); i++) dst[i] = src[i];
  }
}

}  // namespace hb

namespace hbl {

template <class F>
static hipError_t group_bucket(hipStream_t s, int ntile, int n, int max_len, const void* pts, const uint32_t* scalars,
                               const uint32_t* perm, const uint32_t* tile_off, const uint32_t* tile_len,
                               void* tile_sums) {
  if (ntile <= 0) return hipSuccess;
  if (max_len < 1 || max_len > (int)GROUP_TILE) return hipErrorInvalidValue;
  constexpr size_t lds = gb::lds_bytes(hb::BucketKind<F>::G2, sizeof(hb::Jac<F>));
  static_assert(lds <= 64 * 1024, "no function attribute needed up to 64 KiB");
  hipLaunchKernelGGL(hb::k_group_bucket<F>, dim3((unsigned)ntile), dim3(gb::THREADS), lds, s, ntile, n,
                     (const uint32_t*)pts, scalars, perm, tile_off, tile_len, (uint32_t*)tile_sums);
  return hipGetLastError();
}

hipError_t group_bucket_g1(hipStream_t s, int ntile, int n, int max_len, const void* pts, const uint32_t* scalars,
                           const uint32_t* perm, const uint32_t* tile_off, const uint32_t* tile_len, void* tile_sums) {
  return group_bucket<hb::Fp>(s, ntile, n, max_len, pts, scalars, perm, tile_off, tile_len, tile_sums);
}
hipError_t group_bucket_g2(hipStream_t s, int ntile, int n, int max_len, const void* pts, const uint32_t* scalars,
                           const uint32_t* perm, const uint32_t* tile_off, const uint32_t* tile_len, void* tile_sums) {
  return group_bucket<hb::Fp2>(s, ntile, n, max_len, pts, scalars, perm, tile_off, tile_len, tile_sums);
}

}  // namespace hbl
