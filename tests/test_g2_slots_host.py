"""The slot allocator of resident G2 sets (hbbft_amd/csrc/g2_slots.hpp, used by hbh_g2_set_add /
hbh_g2_set_release in engine_pairing.hip): a stand-alone host program includes the header and checks

* free slots are handed out lowest first;
* a released slot is the next one reused;
* releasing a slot that is not live, out of range, or named twice in one call is refused and frees
  nothing;
* a full set refuses a request it cannot serve whole and takes nothing.

The program is a plain host executable built with AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hbbft_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "g2_slots.hpp"

static int fails = 0;
#define CHECK(c)                                           \
  do {                                                     \
    if (!(c)) {                                            \
      std::printf("FAIL line %d: %s\n", __LINE__, #c);     \
      fails++;                                             \
    }                                                      \
  } while (0)

int main() {
  {  // lowest free first, size bookkeeping
    G2Slots s(5);
    uint32_t a[5] = {9, 9, 9, 9, 9};
    CHECK(s.capacity() == 5 && s.live_count() == 0 && s.free_count() == 5);
    CHECK(s.take(3, a) && a[0] == 0 && a[1] == 1 && a[2] == 2);
    CHECK(s.live_count() == 3 && s.free_count() == 2);
    CHECK(s.live(0) && s.live(2) && !s.live(3) && !s.live(5) && !s.live(0xffffffffu));
    // reuse after release: the freed slot comes before the never-used ones
    const uint32_t mid = 1;
    CHECK(s.release(1, &mid) && !s.live(1) && s.live_count() == 2);
    uint32_t b[2] = {9, 9};
    CHECK(s.take(2, b) && b[0] == 1 && b[1] == 3);
    // double release refused
    CHECK(s.release(1, &mid) && !s.release(1, &mid) && s.live_count() == 3);
    // a slot named twice in one call, a slot never taken, a slot out of range: nothing is freed
    const uint32_t twice[3] = {0, 2, 0}, never[2] = {0, 4}, far[2] = {2, 5};
    CHECK(!s.release(3, twice) && !s.release(2, never) && !s.release(2, far));
    CHECK(s.live(0) && s.live(2) && s.live(3) && s.live_count() == 3);
    // a full set: a request larger than the room takes nothing, the exact room is served
    uint32_t c[3] = {9, 9, 9};
    CHECK(!s.take(3, c) && c[0] == 9 && s.live_count() == 3);
    CHECK(s.take(2, c) && c[0] == 1 && c[1] == 4 && s.free_count() == 0);
    CHECK(!s.take(1, c) && s.take(0, c));
    const uint32_t all[5] = {4, 0, 3, 1, 2};
    CHECK(s.release(5, all) && s.live_count() == 0);
    CHECK(s.take(5, a) && a[0] == 0 && a[1] == 1 && a[2] == 2 && a[3] == 3 && a[4] == 4);
  }
  {  // across the 64-slot words of the bitmap, in an order that is not the allocation order
    G2Slots s(130);
    std::vector<uint32_t> got(130);
    CHECK(s.take(130, got.data()));
    for (uint32_t k = 0; k < 130; k++) CHECK(got[k] == k);
    const uint32_t rel[4] = {129, 64, 63, 7};
    CHECK(s.release(4, rel) && s.free_count() == 4);
    uint32_t again[4];
    CHECK(s.take(4, again) && again[0] == 7 && again[1] == 63 && again[2] == 64 && again[3] == 129);
  }
  {  // an empty set
    G2Slots s;
    uint32_t x = 9;
    CHECK(s.capacity() == 0 && !s.take(1, &x) && !s.live(0) && !s.release(1, &x));
  }
  if (fails) return 1;
  std::printf("g2_slots OK\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def slots_program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++) to build the slot program")
    d = tmp_path_factory.mktemp("g2_slots")
    src, exe = d / "slots.cpp", d / "slots"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    return str(exe)


def test_slot_allocator(slots_program):
    r = subprocess.run([slots_program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "g2_slots OK" in r.stdout


def test_engine_uses_the_header():
    """The sets of the engine (the struct in engine_impl.hpp, the calls in engine_pairing.hip) allocate
    through the header under test."""
    with open(os.path.join(CSRC, "engine_impl.hpp")) as f:
        text = f.read()
    assert '#include "g2_slots.hpp"' in text
    assert "G2Slots slots" in text
    with open(os.path.join(CSRC, "engine_pairing.hip")) as f:
        text = f.read()
    assert '#include "engine_impl.hpp"' in text
    for use in ("slots.take(", "slots.release(", "slots.live("):
        assert use in text, use
