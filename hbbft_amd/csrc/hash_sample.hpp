// The sampler in front of hash_g2 (threshold_crypto hash_g2 = pairing 0.14 G2::rand over
// ChaChaRng::from_seed(sha3_256(msg))): the ChaCha20 word stream of rand_chacha
// 0.1 consumed through rand 0.4 -- next_u32 = the next key-stream word, next_u64 = two words, low word
// first -- and ff 0.4's Fq::rand / rand's bool on top of it.  Plain functions, no HIP constructs
// beyond the HB_HD qualifier: k_hash.hip runs them one lane per message, and the host includes the
// header too (tests/test_hash_sample_host.py compares the stream with the oracle's).
//
// A stream position is (block, word): the ChaCha block counter and the index (< 16) of the next word
// in that block.  A stream can be reopened at any position from the 32-byte seed alone, which is how
// the sampling kernel carries a message from one round to the next.
#pragma once
#include <stdint.h>

#include "constants.hpp"

#ifndef HB_HD
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define HB_HD __host__ __device__ __forceinline__
#else
#define HB_HD inline
#endif
#endif

namespace hsample {

struct Stream {
  uint32_t key[8];   // the seed as 8 little-endian words
  uint32_t buf[16];  // key stream of block `block` when loaded
  uint64_t block;    // position: block counter ...
  uint32_t word;     // ... and the next word in it, < 16
  bool loaded;
};

HB_HD uint32_t rotl32(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }

#define HS_QR(a, b, c, d)      \
  do {                         \
    a += b; d = rotl32(d ^ a, 16); \
    c += d; b = rotl32(b ^ c, 12); \
    a += b; d = rotl32(d ^ a, 8);  \
    c += d; b = rotl32(b ^ c, 7);  \
  } while (0)

// One ChaCha20 block (20 rounds), rand_chacha 0.1 layout: constants, 8 key words, the 64-bit block
// counter in words 12-13, a zero 64-bit nonce in words 14-15.
HB_HD void chacha20_block(const uint32_t key[8], uint64_t counter, uint32_t out[16]) {
  const uint32_t s0 = 0x61707865u, s1 = 0x3320646eu, s2 = 0x79622d32u, s3 = 0x6b206574u;
  const uint32_t c0 = (uint32_t)counter, c1 = (uint32_t)(counter >> 32);
  uint32_t x0 = s0, x1 = s1, x2 = s2, x3 = s3, x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3], x8 = key[4],
           x9 = key[5], x10 = key[6], x11 = key[7], x12 = c0, x13 = c1, x14 = 0, x15 = 0;
  for (int r = 0; r < 10; r++) {
    HS_QR(x0, x4, x8, x12);
    HS_QR(x1, x5, x9, x13);
    HS_QR(x2, x6, x10, x14);
    HS_QR(x3, x7, x11, x15);
    HS_QR(x0, x5, x10, x15);
    HS_QR(x1, x6, x11, x12);
    HS_QR(x2, x7, x8, x13);
    HS_QR(x3, x4, x9, x14);
  }
  out[0] = x0 + s0;
  out[1] = x1 + s1;
  out[2] = x2 + s2;
  out[3] = x3 + s3;
  out[4] = x4 + key[0];
  out[5] = x5 + key[1];
  out[6] = x6 + key[2];
  out[7] = x7 + key[3];
  out[8] = x8 + key[4];
  out[9] = x9 + key[5];
  out[10] = x10 + key[6];
  out[11] = x11 + key[7];
  out[12] = x12 + c0;
  out[13] = x13 + c1;
  out[14] = x14;
  out[15] = x15;
}
#undef HS_QR

// ChaChaRng::from_seed(seed) moved to position (block, word); (0, 0) is the fresh stream
HB_HD void stream_open(Stream& s, const uint8_t seed[32], uint64_t block = 0, uint32_t word = 0) {
  for (int i = 0; i < 8; i++)
    s.key[i] = (uint32_t)seed[4 * i] | ((uint32_t)seed[4 * i + 1] << 8) | ((uint32_t)seed[4 * i + 2] << 16) |
               ((uint32_t)seed[4 * i + 3] << 24);
  s.block = block;
  s.word = word & 15u;
  s.loaded = false;
}

HB_HD uint32_t next_u32(Stream& s) {
  if (!s.loaded) {
    chacha20_block(s.key, s.block, s.buf);
    s.loaded = true;
  }
  // a select chain instead of a variable index: on the device buf then stays in registers
  uint32_t w = s.buf[0];
  for (int i = 1; i < 16; i++) w = s.word == (uint32_t)i ? s.buf[i] : w;
  if (++s.word == 16) {
    s.word = 0;
    s.block++;
    s.loaded = false;
  }
  return w;
}

HB_HD uint64_t next_u64(Stream& s) {  // low word first
  const uint64_t lo = next_u32(s);
  return lo | ((uint64_t)next_u32(s) << 32);
}

// rand 0.4 bool: gen::<u8>() & 1 == 1 with u8 = next_u32() as u8
HB_HD bool gen_bool(Stream& s) { return (next_u32(s) & 1u) != 0; }

// w (12 little-endian words) >= p
HB_HD bool words_geq_p(const uint32_t w[12]) {
  for (int i = 11; i >= 0; i--)
    if (w[i] != hb::P_W[i]) return w[i] > hb::P_W[i];
  return true;
}

// ff 0.4 Fq::rand: six next_u64 limbs (= twelve stream words, little-endian), the top three bits
// cleared, redrawn while >= p.  The limbs ARE pairing's Montgomery representation (R = 2^384): the
// field element is limbs * 2^-384 mod p (hb::fq_limbs_to_fp in k_hash.hip converts, one product).
// Draws at most max_draws candidates; false when every one was >= p (the stream stands behind the
// last draw), so no caller loops without a bound.  A draw fails with probability 0.187.
HB_HD bool gen_fq(Stream& s, uint32_t w[12], int max_draws = 64) {
  for (int d = 0; d < max_draws; d++) {
    for (int i = 0; i < 12; i++) w[i] = next_u32(s);
    w[11] &= 0xffffffffu >> 3;
    if (!words_geq_p(w)) return true;
  }
  return false;
}

// Step over one candidate of G2::rand -- x = (gen_fq, gen_fq) and the sign flag -- without keeping
// it: the stream stands where drawing the candidate would have left it.  No field work.  false on
// gen_fq's draw failure (the stream then stands behind the failed draws, as gen_fq leaves it).
// k_hash_quad.hip opens a message's stream at its saved position on four lanes and steps lane j over
// j candidates, so that the lanes try the next four side by side.
HB_HD bool skip_candidate(Stream& s, int max_draws = 64) {
  uint32_t w[12];
  if (!gen_fq(s, w, max_draws) || !gen_fq(s, w, max_draws)) return false;
  (void)gen_bool(s);
  return true;
}

}  // namespace hsample
