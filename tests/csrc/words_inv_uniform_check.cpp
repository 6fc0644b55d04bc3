// CPU check of hbbft_amd/csrc/words.hpp's branch-free inverse (INV_UNIFORM, the lane-pair pairing
// kernel's) against the per-divstep form (MODE 0), word for word, over the BLS12-381 base field
// (12 words) and scalar field (8 words): seeded random values, the values around 0 and m, every
// 2^k and 2^k - 1 below m; and y * y^-1 == 1 on the first 200 values.  Built (once plain, once with
// the address and undefined-behaviour sanitizers) and run by tests/test_words_inv_uniform.py.
#include <cstdint>
#include <cstdio>
#include <random>

#include "words.hpp"

template <int N>
static bool mul_is_one(const uint32_t* a, const uint32_t* b, const uint32_t* m) {
  // a * b mod m by shift-and-add (slow, test only)
  uint32_t acc[N + 1] = {0};
  for (int bit = 32 * N - 1; bit >= 0; bit--) {
    uint32_t carry = 0;  // acc <<= 1
    for (int i = 0; i <= N; i++) {
      const uint32_t nc = acc[i] >> 31;
      acc[i] = (acc[i] << 1) | carry;
      carry = nc;
    }
    if ((a[bit >> 5] >> (bit & 31)) & 1) {
      uint64_t c = 0;
      for (int i = 0; i < N; i++) {
        c += (uint64_t)acc[i] + b[i];
        acc[i] = (uint32_t)c;
        c >>= 32;
      }
      acc[N] += (uint32_t)c;
    }
    for (int k = 0; k < 3; k++) {
      if (acc[N] == 0 && !hb::words_geq<N>(acc, m)) break;
      const uint32_t br = hb::words_sub<N>(acc, m);
      acc[N] -= br;
    }
  }
  return acc[N] == 0 && hb::words_is_one<N>(acc);
}

template <int N>
struct Checker {
  const uint32_t* m;
  int count = 0, bad = 0;

  void check(const uint32_t* y) {
    uint32_t r0[N], r4[N];
    hb::words_inv_vartime<N, 0>(y, m, r0);
    hb::words_inv_vartime<N, hb::INV_UNIFORM>(y, m, r4);
    bool same = true, zero = true;
    for (int i = 0; i < N; i++) {
      same = same && r0[i] == r4[i];
      zero = zero && y[i] == 0;
    }
    bool ok = same;
    if (ok && !zero && count < 200) ok = mul_is_one<N>(y, r4, m);
    if (ok && zero)
      for (int i = 0; i < N; i++) ok = ok && r4[i] == 0;
    if (!ok) bad++;
    count++;
  }
  void small(uint32_t v) {
    uint32_t y[N] = {0};
    y[0] = v;
    check(y);
  }
  void below_m(uint32_t d) {  // m - d (d below m's low word)
    uint32_t y[N];
    for (int i = 0; i < N; i++) y[i] = m[i];
    y[0] -= d;
    check(y);
  }
};

template <int N>
static int run(const uint32_t* m, uint32_t topmask, int iters, uint64_t seed, int* count) {
  Checker<N> ck{m};
  std::mt19937_64 rng(seed);
  for (int it = 0; it < iters; it++) {
    uint32_t y[N];
    for (int i = 0; i < N; i++) y[i] = (uint32_t)rng();
    y[N - 1] &= topmask;
    if (!hb::words_geq<N>(y, m)) ck.check(y);  // canonical values only
    else it--;
  }
  ck.small(0);
  ck.small(1);
  ck.small(2);
  ck.below_m(1);
  ck.below_m(2);
  {  // (m + 1) / 2
    uint32_t y[N + 1];
    for (int i = 0; i < N; i++) y[i] = m[i];
    y[N] = 0;
    y[0] += 1;  // m is odd and its low word is not 0xffffffff
    hb::words_shr1<N>(y, 0);
    ck.check(y);
  }
  for (int k = 0; k < 32 * N; k++) {  // 2^k and 2^k - 1, below m
    uint32_t p[N] = {0}, q[N] = {0};
    p[k >> 5] = 1u << (k & 31);
    for (int i = 0; i < (k >> 5); i++) q[i] = 0xffffffffu;
    q[k >> 5] = (1u << (k & 31)) - 1u;
    if (!hb::words_geq<N>(p, m)) ck.check(p);
    if (!hb::words_geq<N>(q, m)) ck.check(q);
  }
  *count = ck.count;
  return ck.bad;
}

int main() {
  const uint32_t P[12] = {0xffffaaab, 0xb9feffff, 0xb153ffff, 0x1eabfffe, 0xf6b0f624, 0x6730d2a0,
                          0xf38512bf, 0x64774b84, 0x434bacd7, 0x4b1ba7b6, 0x397fe69a, 0x1a0111ea};
  const uint32_t R[8] = {0x00000001, 0xffffffff, 0xfffe5bfe, 0x53bda402,
                         0x09a1d805, 0x3339d808, 0x299d7d48, 0x73eda753};
  int np = 0, nr = 0;
  const int bp = run<12>(P, 0x1fffffff, 20000, 11, &np);
  const int br = run<8>(R, 0x7fffffff, 20000, 12, &nr);
  printf("p: %d bad of %d, r: %d bad of %d\n", bp, np, br, nr);
  return (bp || br) ? 1 : 0;
}
