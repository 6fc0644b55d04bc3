// Stand-alone check of hbbft_amd/csrc/group_digits.hpp (the digit forms of a grouped call's scalars): for
// each digit tuple it replays the exact step sequence of the device chain (k_rlc_digits.hip joint_chain:
// the start value, then per step a doubling and the table entry +B, -lambda B or B - lambda B that
// gd::entry names) over the integers mod r, with the bases taken as the scalars they stand for
// (Q -> 1, -psi(Q) -> |x|, lambda = |x|^2), and compares the result with the tuple's residue:
//   X4 / G2: chain 0 on 1 plus chain 1 on |x|        == a0 + a1 |x| + a2 |x|^2 + a3 |x|^3
//   X4 / G1: the one 96-step chain on 1              == the same; its halves are a0 + a1 |x|, a2 + a3 |x| < 2^96
//   X2 / G1: the one 64-step chain on 1              == b0 + b1 |x|^2
// The residues are checked to be below r (no reduction: a tuple is its own canonical residue), the
// running coefficients to stay within the bound the kernel's exceptional-addition argument uses, and
// the zero residue -- what a grouped call rejects or redraws by its all-zero bytes -- to be the all-zero
// tuple only.  Prints "group_digits: 0 bad of <checks>"; exit
// status 1 on any failure.  tests/test_group_digits_host.py builds it plain and with the address and
// undefined-behaviour sanitizers.
#include <cstdio>
#include <random>

#include "group_digits.hpp"

static long g_checks = 0, g_bad = 0;
#define CHECK(cond)                                                                \
  do {                                                                             \
    g_checks++;                                                                    \
    if (!(cond)) {                                                                 \
      if (g_bad++ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
    }                                                                              \
  } while (0)

typedef unsigned __int128 u128;

// 256-bit unsigned integers, four LE u64 words, and arithmetic mod r
struct U256 {
  uint64_t w[4];
};
static U256 u256(uint64_t v) { return U256{{v, 0, 0, 0}}; }
static bool eq(const U256& a, const U256& b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3]; }
static bool lt(const U256& a, const U256& b) {
  for (int i = 3; i >= 0; i--)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
  return false;
}
static U256 add(const U256& a, const U256& b, bool* carry) {
  U256 r;
  u128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (u128)a.w[i] + b.w[i];
    r.w[i] = (uint64_t)c;
    c >>= 64;
  }
  *carry = c != 0;
  return r;
}
static U256 sub(const U256& a, const U256& b) {  // a - b mod 2^256
  U256 r;
  uint64_t borrow = 0;
  for (int i = 0; i < 4; i++) {
    const u128 d = (u128)a.w[i] - b.w[i] - borrow;
    r.w[i] = (uint64_t)d;
    borrow = (uint64_t)(d >> 64) & 1;
  }
  return r;
}
static U256 mul64(const U256& a, uint64_t m, bool* overflow) {
  U256 r;
  u128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (u128)a.w[i] * m;
    r.w[i] = (uint64_t)c;
    c >>= 64;
  }
  *overflow = c != 0;
  return r;
}

static U256 R;  // the group order, from hb::R_W
static U256 addm(const U256& a, const U256& b) {  // a, b < r < 2^255: the sum does not carry
  bool carry;
  U256 s = add(a, b, &carry);
  CHECK(!carry);
  return lt(s, R) ? s : sub(s, R);
}
static U256 subm(const U256& a, const U256& b) {  // a, b < r
  bool carry;
  return lt(a, b) ? sub(add(a, R, &carry), b) : sub(a, b);
}

static U256 XP[4];  // |x|^j

// The device chain on the base b (a residue): acc <- lambda b or 0; per step acc <- 2 acc + entry
static U256 replay(const gd::Chain& c, int steps, const U256& b) {
  const U256 lb = [&] {  // lambda b = |x|^2 b mod r; b is 1 or |x| here, so no reduction is needed
    bool o1, o2;
    U256 t = mul64(b, hb::X_ABS, &o1);
    t = mul64(t, hb::X_ABS, &o2);
    CHECK(!o1 && !o2 && lt(t, R));
    return t;
  }();
  const U256 b_minus_lb = subm(b, lb);
  const U256 minus_lb = subm(u256(0), lb);
  U256 acc = c.lead ? lb : u256(0);
  for (int i = steps - 1; i >= 0; i--) {
    acc = addm(acc, acc);
    const int e = gd::entry(c, i);
    CHECK(e >= 0 && e <= 3);
    if (e == 1) acc = addm(acc, b);
    if (e == 2) acc = addm(acc, minus_lb);
    if (e == 3) acc = addm(acc, b_minus_lb);
  }
  return acc;
}

// The same chain as its integer coefficients: acc = U + V lambda with 0 <= U < 2^steps, 0 <= V <= 2^steps
// at every step (what the kernel's argument against exceptional additions rests on), ending at (u, v)
static void replay_coeffs(const gd::Chain& c, int steps, u128 u, u128 v) {
  u128 U = 0, V = c.lead ? 1 : 0;
  for (int i = steps - 1; i >= 0; i--) {
    U <<= 1;
    V <<= 1;
    const int e = gd::entry(c, i);
    if (e & 1) U += 1;
    if (e & 2) {
      CHECK(V >= 1);  // V never goes negative
      V -= 1;
    }
    const u128 cap = (u128)1 << (steps - i);
    CHECK(U < cap && V <= cap);
    CHECK(!(U == 0 && V == 0) || (!c.lead && e == 0));  // acc = O only above the leading bits
  }
  CHECK(U == u && V == v);
}

static U256 residue4(const uint32_t a[4]) {  // sum a_j |x|^j, checked < r
  U256 s = u256(0);
  for (int j = 0; j < 4; j++) {
    bool o, carry;
    const U256 t = mul64(XP[j], a[j], &o);
    s = add(s, t, &carry);
    CHECK(!o && !carry);
  }
  CHECK(lt(s, R));
  return s;
}

static void check_x4(const uint32_t a[4]) {
  const U256 want = residue4(a);
  // G2: two 32-step chains on Q -> 1 and -psi(Q) -> |x|
  const gd::Chain c0 = gd::chain_x4_g2(a, 0), c1 = gd::chain_x4_g2(a, 1);
  CHECK(eq(addm(replay(c0, gd::steps_g2(), XP[0]), replay(c1, gd::steps_g2(), XP[1])), want));
  replay_coeffs(c0, gd::steps_g2(), a[0], a[2]);
  replay_coeffs(c1, gd::steps_g2(), a[1], a[3]);
  // G1: one 96-step chain on P -> 1 of the halves a0 + a1 |x| and a2 + a3 |x|
  const gd::Chain g = gd::chain_x4_g1(a);
  const u128 h0 = (u128)a[0] + (u128)a[1] * hb::X_ABS, h1 = (u128)a[2] + (u128)a[3] * hb::X_ABS;
  CHECK((h0 >> 96) == 0 && (h1 >> 96) == 0);
  CHECK(g.pos[0] == (uint32_t)h0 && g.pos[1] == (uint32_t)(h0 >> 32) && g.pos[2] == (uint32_t)(h0 >> 64));
  CHECK(gd::steps_g1(gd::FORM_X4) == 96);
  CHECK(eq(replay(g, 96, XP[0]), want));
  replay_coeffs(g, 96, h0, h1);
  CHECK(((a[0] | a[1] | a[2] | a[3]) == 0) == eq(want, u256(0)));  // the zero residue is the all-zero tuple only
}

static void check_x2(uint64_t b0, uint64_t b1) {
  const uint32_t a[4] = {(uint32_t)b0, (uint32_t)(b0 >> 32), (uint32_t)b1, (uint32_t)(b1 >> 32)};
  bool o, carry;
  const U256 want = add(u256(b0), mul64(XP[2], b1, &o), &carry);
  CHECK(!o && !carry && lt(want, R));
  const gd::Chain g = gd::chain_x2_g1(a);
  CHECK(gd::steps_g1(gd::FORM_X2) == 64);
  CHECK(eq(replay(g, 64, XP[0]), want));
  replay_coeffs(g, 64, b0, b1);
  const gd::Chain g2 = gd::chain_g1(gd::FORM_X2, a);
  CHECK(g2.lead == g.lead && g2.pos[0] == g.pos[0] && g2.pos[1] == g.pos[1] && g2.neg[0] == g.neg[0] && g2.neg[1] == g.neg[1]);
  CHECK(((a[0] | a[1] | a[2] | a[3]) == 0) == eq(want, u256(0)));
}

int main() {
  for (int i = 0; i < 4; i++) R.w[i] = (uint64_t)hb::R_W[2 * i] | ((uint64_t)hb::R_W[2 * i + 1] << 32);
  XP[0] = u256(1);
  for (int j = 1; j < 4; j++) {
    bool o;
    XP[j] = mul64(XP[j - 1], hb::X_ABS, &o);
    CHECK(!o);
  }
  {  // r = |x|^4 - |x|^2 + 1
    bool o, carry;
    const U256 x4 = mul64(XP[3], hb::X_ABS, &o);
    CHECK(!o && eq(add(sub(x4, XP[2]), u256(1), &carry), R));
  }
  // every digit in {0, 1, max}, all combinations (this covers the single non-zero digit in each position
  // and the leading-zero high digits); then each position alone with a mid value
  const uint32_t e32[3] = {0u, 1u, 0xffffffffu};
  for (int k = 0; k < 81; k++) {
    const uint32_t a[4] = {e32[k % 3], e32[k / 3 % 3], e32[k / 9 % 3], e32[k / 27]};
    check_x4(a);
  }
  const uint64_t e64[3] = {0ull, 1ull, ~0ull};
  for (int k = 0; k < 9; k++) check_x2(e64[k % 3], e64[k / 3]);
  for (int j = 0; j < 4; j++)
    for (uint32_t v : {2u, 0x80000000u, 0x12345678u}) {
      uint32_t a[4] = {0, 0, 0, 0};
      a[j] = v;
      check_x4(a);
    }
  for (uint64_t v : {2ull, 1ull << 32, 1ull << 63, 0x123456789abcdefull}) {
    check_x2(v, 0);
    check_x2(0, v);
  }
  std::mt19937_64 rng(2201);
  for (int i = 0; i < 10000; i++) {
    const uint64_t lo = rng(), hi = rng();
    uint32_t a[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
    check_x4(a);
    check_x2(lo, hi);
    if (i % 4 == 0) {  // leading-zero high digits and short digits
      a[3] = 0;
      a[2] >>= (i / 4) % 32;
      check_x4(a);
      check_x2(lo, hi >> ((i / 4) % 64));
      check_x2(lo >> ((i / 4) % 64), 0);
    }
  }
  std::printf("group_digits: %ld bad of %ld\n", g_bad, g_checks);
  return g_bad ? 1 : 0;
}
