// Slot allocator of a device-resident G2 set (hbh_g2_set_*): which of the set's `capacity` slots hold
// a prepared point.  Free slots are handed out lowest first, so a released slot is the next one
// reused and a set that never fills stays dense from slot 0.  Plain C++, no HIP: the engine (engine_impl.hpp) keeps one
// per set under the engine lock, tests/test_g2_slots_host.py runs it on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <vector>

struct G2Slots {
  // free: a min-heap of the free slots; live: one bit per slot
  std::vector<uint32_t> free_heap;
  std::vector<uint64_t> live_bits;
  size_t cap = 0, nlive = 0;

  explicit G2Slots(size_t capacity = 0) { reset(capacity); }

  void reset(size_t capacity) {
    cap = capacity;
    nlive = 0;
    live_bits.assign((capacity + 63) / 64, 0);
    free_heap.resize(capacity);
    for (size_t k = 0; k < capacity; k++) free_heap[k] = (uint32_t)k;
    std::make_heap(free_heap.begin(), free_heap.end(), std::greater<uint32_t>());
  }

  size_t capacity() const { return cap; }
  size_t live_count() const { return nlive; }
  size_t free_count() const { return cap - nlive; }
  bool live(uint64_t slot) const { return slot < cap && ((live_bits[slot >> 6] >> (slot & 63)) & 1); }

  // n free slots, lowest first, into out; false (nothing taken) when fewer than n are free
  bool take(size_t n, uint32_t* out) {
    if (n > free_count()) return false;
    for (size_t k = 0; k < n; k++) {
      std::pop_heap(free_heap.begin(), free_heap.end(), std::greater<uint32_t>());
      const uint32_t s = free_heap.back();
      free_heap.pop_back();
      live_bits[s >> 6] |= (uint64_t)1 << (s & 63);
      out[k] = s;
    }
    nlive += n;
    return true;
  }

  // frees n slots; false (nothing freed) when one of them is not live or is named twice
  bool release(size_t n, const uint32_t* slots) {
    for (size_t k = 0; k < n; k++) {
      bool ok = live(slots[k]);
      if (ok) {
        live_bits[slots[k] >> 6] &= ~((uint64_t)1 << (slots[k] & 63));  // marks it: a repeat fails the test above
      } else {
        for (size_t j = 0; j < k; j++) live_bits[slots[j] >> 6] |= (uint64_t)1 << (slots[j] & 63);
        return false;
      }
    }
    for (size_t k = 0; k < n; k++) {
      free_heap.push_back(slots[k]);
      std::push_heap(free_heap.begin(), free_heap.end(), std::greater<uint32_t>());
    }
    nlive -= n;
    return true;
  }
};
