// Stand-alone check of hbbft_amd/csrc/group_bucket.hpp (layout of the bucket form of the group sums):
// the digits of a scalar recombine to it (G1: 64 two-bit digits of r; G2: r = d0 + d1 |x| + d2 |x|^2
// with 32 two-bit digits over d0 and d1 and d2 as digit 1 of window 0) and are < 4, the thread map is a
// bijection onto (window, slice), the LDS bytes stay within the stated budget and the tail's segments
// cover every window exactly once with the right weight.  Prints "GB_WINDOWS <g1> <g2>" and
// "group_bucket: 0 bad of <checks>"; exit status 1 on any failure.  tests/test_group_bucket_host.py
// builds it plain and with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <random>
#include <vector>

#include "group_bucket.hpp"

static long g_checks = 0, g_bad = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    g_checks++;                                                  \
    if (!(cond)) {                                               \
      if (g_bad++ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
    }                                                            \
  } while (0)

typedef unsigned __int128 u128;
static const u128 X = (u128)hb::X_ABS;

static void check_scalar(u128 r) {
  const uint32_t w[4] = {(uint32_t)r, (uint32_t)(r >> 32), (uint32_t)(r >> 64), (uint32_t)(r >> 96)};
  // G1: sum_w 4^w digit_w = r
  {
    const gb::Digits d = gb::digits_of(false, w);
    u128 acc = 0;
    for (int win = gb::windows(false) - 1; win >= 0; win--) {
      const uint32_t dig = gb::digit(d, false, 0, win);
      CHECK(dig < 4);
      acc = (acc << gb::WINDOW_BITS) | dig;
    }
    CHECK(acc == r);
  }
  // G2: the three terms' digits give d0, d1, d2 with d0 + d1 |x| + d2 |x|^2 = r
  {
    const gb::Digits d = gb::digits_of(true, w);
    u128 v[3] = {0, 0, 0};
    for (int term = 0; term < gb::terms_per_item(true); term++)
      for (int win = gb::windows(true) - 1; win >= 0; win--) {
        const uint32_t dig = gb::digit(d, true, term, win);
        CHECK(dig < 4);
        v[term] = (v[term] << gb::WINDOW_BITS) | dig;
      }
    CHECK(v[0] < X && v[1] < X && v[2] <= 1);
    CHECK(v[0] == d.v[0] && v[1] == d.v[1] && v[2] == d.top);
    for (int win = 1; win < gb::windows(true); win++) CHECK(gb::digit(d, true, 2, win) == 0);
    // d2 |x|^2 <= r < 2^128, so the sum does not wrap
    CHECK(v[0] + v[1] * X + (v[2] ? X * X : (u128)0) == r);
  }
}

static void check_layout(bool g2, size_t jac_bytes) {
  // thread -> (window, slice) is a bijection of [0, lanes) onto windows x SLICES, inverted by lane_of
  const int nl = gb::lanes(g2), nw = gb::windows(g2);
  CHECK(nl == nw * gb::SLICES && nl <= gb::THREADS);
  std::vector<int> seen((size_t)nl, 0);
  for (int t = 0; t < nl; t++) {
    const int w = gb::lane_window(g2, t), s = gb::lane_slice(g2, t);
    CHECK(w >= 0 && w < nw && s >= 0 && s < gb::SLICES);
    CHECK(gb::lane_of(g2, w, s) == t);
    if (w >= 0 && w < nw && s >= 0 && s < gb::SLICES) seen[(size_t)(s * nw + w)]++;
  }
  for (int k = 0; k < nl; k++) CHECK(seen[(size_t)k] == 1);
  for (int w = 0; w < nw; w++)
    for (int s = 0; s < gb::SLICES; s++) {
      const int t = gb::lane_of(g2, w, s);
      CHECK(t >= 0 && t < nl && gb::lane_window(g2, t) == w && gb::lane_slice(g2, t) == s);
    }
  // LDS
  CHECK(gb::slot_bytes(jac_bytes) >= jac_bytes && gb::slot_bytes(jac_bytes) % 16 == 0 && gb::slot_bytes(jac_bytes) < jac_bytes + 16);
  CHECK(gb::bucket_bytes(g2, jac_bytes) == (size_t)nl * gb::NBUCKET * gb::slot_bytes(jac_bytes));
  CHECK(gb::lds_bytes(g2, jac_bytes) == gb::bucket_bytes(g2, jac_bytes) + gb::stage_bytes(g2, jac_bytes));
  CHECK(gb::lds_bytes(g2, jac_bytes) <= gb::LDS_BUDGET);
  CHECK(gb::LDS_BUDGET <= 64 * 1024);
  CHECK(gb::stage_items(g2) >= 1 && gb::stage_items(g2) <= gb::THREADS);
  // tail: the segments cover every window exactly once, in order; Horner inside a segment and its shift
  // give window w the weight 4^w
  std::vector<int> cover((size_t)nw, 0);
  for (int s = 0; s < gb::TAIL_SEGS; s++) {
    CHECK(gb::seg_lo(g2, s) < gb::seg_hi(g2, s) && gb::seg_hi(g2, s) <= nw);
    if (s) CHECK(gb::seg_lo(g2, s) == gb::seg_hi(g2, s - 1));
    for (int w = gb::seg_lo(g2, s); w < gb::seg_hi(g2, s) && w < nw; w++) {
      cover[(size_t)w]++;
      const int doublings = gb::WINDOW_BITS * (w - gb::seg_lo(g2, s)) + gb::seg_shift(g2, s);
      CHECK(doublings == gb::WINDOW_BITS * w);
    }
  }
  CHECK(gb::seg_lo(g2, 0) == 0 && gb::seg_hi(g2, gb::TAIL_SEGS - 1) == nw);
  for (int w = 0; w < nw; w++) CHECK(cover[(size_t)w] == 1);
}

int main() {
  std::printf("GB_WINDOWS %d %d\n", gb::windows(false), gb::windows(true));
  std::printf("GB_LDS %zu %zu budget %zu\n", gb::lds_bytes(false, sizeof(hb::Jac<hb::Fp>)),
              gb::lds_bytes(true, sizeof(hb::Jac<hb::Fp2>)), gb::LDS_BUDGET);
  const u128 one = 1;
  const u128 special[] = {1, 2, 3, (one << 64) - 1, one << 64, X - 1, X, X + 1, X * X - 1, X * X,
                          one << 126, (u128)3 << 126, ~(u128)0};
  for (u128 r : special) check_scalar(r);
  std::mt19937_64 rng(1701);
  for (int i = 0; i < 10000; i++) {
    const u128 r = ((u128)rng() << 64) | rng();
    check_scalar(r);
  }
  check_layout(false, sizeof(hb::Jac<hb::Fp>));
  check_layout(true, sizeof(hb::Jac<hb::Fp2>));
  std::printf("group_bucket: %ld bad of %ld\n", g_bad, g_checks);
  return g_bad ? 1 : 0;
}
