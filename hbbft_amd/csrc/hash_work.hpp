// What the two device forms of hashing to G2 share (k_hash.hip, one lane per message; k_hash_quad.hip,
// one lane quad): the sampled point's words between the sampler and the clearing kernel, and the
// layout of the work buffer (hbl::hash_work_bytes).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "constants.hpp"

namespace hb {

constexpr int XY_WORDS = 4 * NL;  // a sampled point between the kernels: x.c0, x.c1, y.c0, y.c1 (Montgomery limbs)

}  // namespace hb

namespace hbl {

constexpr int HASH_RETRY_ROUNDS = 2;  // sampler candidates for messages the clearing kernel sent back
struct HashWork {
  uint32_t *counts, *pos, *xy, *list[2], *retry;
};
// one count per round, the retry count and one per retry round, padded to four words
inline size_t hash_count_words(int rounds) { return ((size_t)rounds + 2 + HASH_RETRY_ROUNDS + 3) & ~(size_t)3; }
// counts and pos first: one memset zeroes both
inline HashWork hash_carve(void* work, size_t n, int rounds) {
  HashWork w;
  w.counts = (uint32_t*)work;
  w.pos = w.counts + hash_count_words(rounds);
  w.xy = w.pos + 2 * n;
  w.list[0] = w.xy + (size_t)hb::XY_WORDS * n;
  w.list[1] = w.list[0] + n;
  w.retry = w.list[1] + n;
  return w;
}

}  // namespace hbl
