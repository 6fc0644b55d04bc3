"""The lane layout of the packed cyclotomic-squaring runs (hbbft_amd/csrc/cyc_pack.hpp, used by
k_wave.hpp cyc_run_packed): a stand-alone host program includes the header and checks, for 2 and 3
checks per wave, that

* (check, role, square, component) <-> lane is a bijection onto the 18 * pack active lanes;
* the two components of a value sit on adjacent lanes, component 0 on the even one (the DPP swap of
  the lane-pair arithmetic exchanges exactly these);
* the source lanes of A, B and A + B belong to the lane's own (check, role);
* the partner map is an involution that trades roles 1 and 2 inside one check and fixes role 0;
* no lane of a check ever names a lane of another check, and idle lanes name only themselves.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hbbft_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "cyc_pack.hpp"
using namespace cycpack;

static int fails = 0;
#define CHECK(c)                                                                   \
  do {                                                                             \
    if (!(c)) {                                                                    \
      std::printf("FAIL pack %d lane %d: %s\n", pack, lane, #c);                   \
      fails++;                                                                     \
    }                                                                              \
  } while (0)

// usable in constant expressions: the kernel evaluates the same functions on the device
static_assert(lane_of(2, 1, 2, 1) == 47 && check_of(47) == 2 && role_of(47) == 1 && square_of(47) == 2, "");
static_assert(max_pack() == 3 && active_lanes(3) == 54, "");

int main() {
  for (int pack = 2; pack <= 3; pack++) {
    int lane = -1;
    CHECK(pack <= max_pack() && active_lanes(pack) == 18 * pack && active_lanes(pack) <= WAVE_LANES);
    int seen[WAVE_LANES] = {0};
    for (int c = 0; c < pack; c++)
      for (int role = 0; role < 3; role++)
        for (int j = 0; j < 3; j++)
          for (int h = 0; h < 2; h++) {
            lane = lane_of(c, role, j, h);
            CHECK(lane >= 0 && lane < active_lanes(pack));
            CHECK(lane == 18 * c + 6 * role + 2 * j + h);
            if (lane < 0 || lane >= WAVE_LANES) continue;
            seen[lane]++;
            CHECK(is_active(lane, pack));
            CHECK(check_of(lane) == c && role_of(lane) == role && square_of(lane) == j && comp_of(lane) == h);
          }
    int holders = 0;
    for (lane = 0; lane < WAVE_LANES; lane++) {
      const bool act = lane < 18 * pack;
      CHECK(seen[lane] == (act ? 1 : 0));  // bijection onto the active lanes
      CHECK(is_active(lane, pack) == act);
      if (!act) {  // idle lanes hold nothing and name only themselves
        CHECK(!is_holder(lane, pack));
        CHECK(partner_lane(lane, pack) == lane);
        for (int k = 0; k < 3; k++) CHECK(source_lane(lane, k, pack) == lane);
        continue;
      }
      const int c = check_of(lane), role = role_of(lane), j = square_of(lane), h = comp_of(lane);
      // lane pairs: (even, odd) neighbours, component 0 on the even lane
      CHECK((lane & 1) == h);
      CHECK(lane_of(c, role, j, 1) == lane_of(c, role, j, 0) + 1 && (lane_of(c, role, j, 0) & 1) == 0);
      CHECK(is_holder(lane, pack) == (j < 2));
      holders += is_holder(lane, pack);
      for (int k = 0; k < 3; k++) {
        const int s = source_lane(lane, k, pack);
        CHECK(is_active(s, pack));
        CHECK(check_of(s) == c && role_of(s) == role && square_of(s) == k && comp_of(s) == h);
        CHECK(s == source_lane(lane, 0, pack) + 2 * k);  // the kernel steps by two lanes
      }
      const int p = partner_lane(lane, pack);
      CHECK(is_active(p, pack));
      CHECK(partner_lane(p, pack) == lane);  // involution
      CHECK(check_of(p) == c && square_of(p) == j && comp_of(p) == h);
      CHECK(role_of(p) == (role == 0 ? 0 : 3 - role));
      CHECK((role == 0) == (p == lane));
    }
    lane = -1;
    CHECK(holders == 12 * pack);  // six Fp2 values of two components per check
  }
  if (fails) return 1;
  std::printf("cyc_pack layout OK\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def layout_program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++) to build the layout program")
    d = tmp_path_factory.mktemp("cyc_pack")
    src, exe = d / "layout.cpp", d / "layout"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    return str(exe)


def test_layout_properties(layout_program):
    r = subprocess.run([layout_program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cyc_pack layout OK" in r.stdout


def test_kernel_uses_the_header():
    """The packed run takes its lanes from the header under test, not from a copy of the arithmetic."""
    with open(os.path.join(CSRC, "k_wave.hpp")) as f:
        text = f.read()
    assert '#include "cyc_pack.hpp"' in text
    for fn in ("cycpack::source_lane", "cycpack::partner_lane", "cycpack::check_of", "cycpack::is_holder"):
        assert fn in text, fn
