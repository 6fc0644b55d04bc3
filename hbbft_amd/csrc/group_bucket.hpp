// Layout of the bucket form of the grouped random-combination sums (k_group_bucket, k_rlc_bucket.hip):
// the window width and counts, the digits of an item's scalar, the (window, slice) <-> thread map, the
// LDS byte count and the segment plan of the tail.  Shared by the kernel and a CPU checker
// (tests/csrc/group_bucket_check.cpp compiles this header with g++), so no HIP here.
//
// A tile's sum is  sum_w 4^w B_w  with  B_w = sum over the tile's terms of digit_w(term) * point(term):
//   G1: one term per item, the point itself; r (128 bits) is 64 two-bit digits.
//   G2: r = d0 + d1 |x| + d2 |x|^2 (div_x_abs twice; d0, d1 < |x| < 2^64, d2 <= 1) gives three terms:
//       P with d0, -psi(P) with d1 (32 two-bit digits each) and psi^2(P) with d2, which is digit 1 of
//       window 0 and digit 0 of every other window.
#pragma once
#include <cstddef>
#include <cstdint>

#include "endo.hpp"

namespace gb {

constexpr int WINDOW_BITS = 2;                      // digits 0..3
constexpr int NBUCKET = (1 << WINDOW_BITS) - 1;     // a lane's buckets: digits 1, 2, 3
constexpr int SLICES = 1;                           // lanes per window (each sums every SLICES-th term)
constexpr int THREADS = 64;                         // one wave per tile
constexpr int TAIL_SEGS = 8;                        // lanes of the tail, one run of windows each
constexpr size_t LDS_BUDGET = 38 * 1024;            // four workgroups per 160 KiB CU, with room to spare

HB_HD constexpr int windows(bool g2) { return g2 ? 32 : 64; }
HB_HD constexpr int terms_per_item(bool g2) { return g2 ? 3 : 1; }
// items staged per round (one thread each): what fits LDS_BUDGET next to the buckets
HB_HD constexpr int stage_items(bool g2) { return g2 ? 8 : 16; }

// An item's scalar, split once per item.  G1: v[0], v[1] = the low and high 64 bits of r, top = 0.
// G2: v[0] = d0, v[1] = d1, top = d2.
struct Digits {
  uint64_t v[2];
  uint32_t top, pad;
};
HB_HD Digits digits_zero() { return Digits{{0, 0}, 0, 0}; }
HB_HD Digits digits_g1(const uint32_t r[4]) {
  return Digits{{(uint64_t)r[0] | ((uint64_t)r[1] << 32), (uint64_t)r[2] | ((uint64_t)r[3] << 32)}, 0, 0};
}
HB_HD Digits digits_g2(const uint32_t r[4]) {
  uint64_t q[4] = {(uint64_t)r[0] | ((uint64_t)r[1] << 32), (uint64_t)r[2] | ((uint64_t)r[3] << 32), 0, 0};
  Digits d;
  d.v[0] = hb::div_x_abs(q);
  d.v[1] = hb::div_x_abs(q);
  d.top = (uint32_t)q[0];  // <= 1: |x|^2 > 2^127
  d.pad = 0;
  return d;
}
HB_HD Digits digits_of(bool g2, const uint32_t r[4]) { return g2 ? digits_g2(r) : digits_g1(r); }

// Digit of `term` (< terms_per_item) at `window` (< windows)
HB_HD uint32_t digit(const Digits& d, bool g2, int term, int window) {
  if (term == 2) return window == 0 ? d.top : 0;
  const uint64_t v = g2 ? d.v[term] : d.v[window >> 5];
  return (uint32_t)(v >> (WINDOW_BITS * (window & 31))) & 3u;
}

// Thread t < lanes(g2) is lane (window, slice); the other threads of the workgroup only stage.
HB_HD constexpr int lanes(bool g2) { return windows(g2) * SLICES; }
HB_HD constexpr int lane_window(bool g2, int t) { return t % windows(g2); }
HB_HD constexpr int lane_slice(bool g2, int t) { return t / windows(g2); }
HB_HD constexpr int lane_of(bool g2, int window, int slice) { return slice * windows(g2) + window; }

// LDS: the buckets, then one round's staged terms (affine, internal form) and digits.  A bucket is a
// Jacobian point in a slot of a multiple of 16 bytes: the 128-bit LDS accesses stay aligned, and the
// lanes' slots (3 x 176 B apart for G1, 3 x 336 B for G2) start 4 banks apart modulo 64, so the 8 lanes
// that one LDS cycle of a 128-bit access serves touch distinct banks.
HB_HD constexpr size_t slot_bytes(size_t jac_bytes) { return (jac_bytes + 15) / 16 * 16; }
HB_HD constexpr size_t bucket_bytes(bool g2, size_t jac_bytes) {
  return (size_t)lanes(g2) * NBUCKET * slot_bytes(jac_bytes);
}
HB_HD constexpr size_t stage_bytes(bool g2, size_t jac_bytes) {
  return (size_t)stage_items(g2) * ((size_t)terms_per_item(g2) * (jac_bytes / 3 * 2) + sizeof(Digits));
}
HB_HD constexpr size_t lds_bytes(bool g2, size_t jac_bytes) { return bucket_bytes(g2, jac_bytes) + stage_bytes(g2, jac_bytes); }

// Tail: segment s < TAIL_SEGS is the Horner run over the windows [seg_lo, seg_hi) from the top one
// down (two doublings and one addition per step), then seg_shift further doublings (its weight 4^seg_lo);
// the segment sums are added up a tree.
HB_HD constexpr int seg_len(bool g2) { return windows(g2) / TAIL_SEGS; }
HB_HD constexpr int seg_lo(bool g2, int s) { return s * seg_len(g2); }
HB_HD constexpr int seg_hi(bool g2, int s) { return (s + 1) * seg_len(g2); }
HB_HD constexpr int seg_shift(bool g2, int s) { return WINDOW_BITS * seg_lo(g2, s); }

static_assert(windows(false) * WINDOW_BITS == 128 && windows(true) * WINDOW_BITS == 64, "digits cover r, d0 and d1");
static_assert(windows(false) % TAIL_SEGS == 0 && windows(true) % TAIL_SEGS == 0, "whole segments");
static_assert((TAIL_SEGS & (TAIL_SEGS - 1)) == 0 && TAIL_SEGS <= windows(true), "the segment tree halves a power of two");
static_assert(lanes(false) <= THREADS && lanes(true) <= THREADS, "a lane per (window, slice)");
static_assert(stage_items(false) <= THREADS && stage_items(true) <= THREADS, "a thread per staged item");

}  // namespace gb
