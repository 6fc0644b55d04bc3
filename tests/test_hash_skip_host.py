"""hsample::skip_candidate (hbbft_amd/csrc/hash_sample.hpp) on the host: the step with which lane j of a
quad of k_hash_sample_quad (k_hash_quad.hip) passes over the j candidates its lower neighbours try.

A stand-alone program includes the header and, for the 64 seeds of tests/test_hash_sample_host.py, opens
the stream, skips j = 0..7 candidates and prints the position it stands at, then draws one more candidate
(gen_fq, gen_fq, gen_bool) there and prints it.  The test compares with oracle.tc.ChaChaRng drawing the
same candidates one by one:

* the position after j skips is the (block, word) the oracle reaches by drawing j candidates;
* the candidate drawn after the skip is the oracle's candidate j + 1;
* the seed set contains sha3(b"hbh-trial-78"), whose stream makes gen_fq redraw, so a skip that counted
  twelve words per gen_fq instead of following the redraws would land elsewhere;
* a skip from a reopened position (the saved position of a later sampler launch) lands where the skip
  from the start does.

The program is built with the address and undefined-behaviour sanitizers: it has its own main, nothing is
loaded into python.
"""
import os
import shutil
import subprocess

import pytest

from oracle import tc
from tests.test_hash_sample_host import consumed, seeds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hbbft_amd", "csrc")
NSKIP = 8

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "hash_sample.hpp"
using namespace hsample;

int main(int argc, char** argv) {
  const int nskip = std::atoi(argv[1]);
  for (int a = 2; a < argc; a++) {
    uint8_t seed[32];
    for (int i = 0; i < 32; i++) {
      unsigned v;
      std::sscanf(argv[a] + 2 * i, "%2x", &v);
      seed[i] = (uint8_t)v;
    }
    uint64_t block1 = 0;  // the position behind the first candidate, where a second launch reopens
    uint32_t word1 = 0;
    for (int j = 0; j < nskip; j++) {
      Stream s;
      stream_open(s, seed);
      bool ok = true;
      for (int k = 0; k < j; k++) ok = ok && skip_candidate(s);
      if (j == 1) {
        block1 = s.block;
        word1 = s.word;
      }
      if (j >= 1) {  // the same place from the saved position, one candidate fewer to skip
        Stream t;
        stream_open(t, seed, block1, word1);
        for (int k = 1; k < j; k++) ok = ok && skip_candidate(t);
        if (t.block != s.block || t.word != s.word) ok = false;
      }
      std::printf("%d %llu %u", ok ? 1 : 0, (unsigned long long)s.block, s.word);
      uint32_t w0[12] = {0}, w1[12] = {0};
      const bool drawn = gen_fq(s, w0) && gen_fq(s, w1);
      const bool greatest = gen_bool(s);
      std::printf(" %d ", drawn ? 1 : 0);
      for (int i = 11; i >= 0; i--) std::printf("%08x", w0[i]);
      std::printf(" ");
      for (int i = 11; i >= 0; i--) std::printf("%08x", w1[i]);
      std::printf(" %d %llu %u\n", greatest ? 1 : 0, (unsigned long long)s.block, s.word);
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def skips(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++) to build the sampler program")
    d = tmp_path_factory.mktemp("hash_skip")
    src, exe = d / "skip.cpp", d / "skip"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe), str(NSKIP)] + [s.hex() for s in seeds()], capture_output=True, text=True, check=True)
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 64 * NSKIP
    return [lines[k * NSKIP:(k + 1) * NSKIP] for k in range(64)]


def test_skip_lands_where_drawing_does(skips):
    rinv = pow(1 << 384, tc.P - 2, tc.P)
    redraws = {}
    for k, (seed, lines) in enumerate(zip(seeds(), skips)):
        rng = tc.ChaChaRng(seed)
        for j, line in enumerate(lines):
            ok, block, word, drawn, l0, l1, greatest, block2, word2 = line.split()
            assert ok == "1" and drawn == "1", (k, j)
            # the oracle has drawn j candidates by now
            assert (int(block), int(word)) == divmod(consumed(rng), 16), (k, j)
            x = (rng.gen_fq(), rng.gen_fq())
            g = rng.gen_bool()
            limbs = (int(l0, 16), int(l1, 16))
            assert all(v < tc.P for v in limbs), (k, j)
            assert tuple(v * rinv % tc.P for v in limbs) == x, (k, j)
            assert int(greatest) == int(g), (k, j)
            assert (int(block2), int(word2)) == divmod(consumed(rng), 16), (k, j)
        redraws[k] = (consumed(rng) - NSKIP * 25) // 12
    # the inputs exercise the redraw loop inside the skipped candidates
    assert redraws[78 - 16] >= 1
    assert sum(redraws.values()) > 64


def test_skip_reports_the_draw_failure(tmp_path):
    """max_draws = 0 stands for 64 draws >= p in a row: skip_candidate returns false, as gen_fq does"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    src, exe = tmp_path / "fail.cpp", tmp_path / "fail"
    src.write_text(r"""
#include <cstdio>
#include "hash_sample.hpp"
int main() {
  uint8_t seed[32] = {1, 2, 3};
  hsample::Stream s;
  hsample::stream_open(s, seed);
  const bool none = hsample::skip_candidate(s, 0);
  const bool one = hsample::skip_candidate(s, 64);
  std::printf("%d %d %llu %u\n", none ? 1 : 0, one ? 1 : 0, (unsigned long long)s.block, s.word);
  return 0;
}
""")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out[:2] == ["0", "1"]
    rng = tc.ChaChaRng(bytes([1, 2, 3]) + bytes(29))
    rng.gen_fq(), rng.gen_fq(), rng.gen_bool()
    assert (int(out[2]), int(out[3])) == divmod(consumed(rng), 16)


def test_kernel_uses_the_helper():
    with open(os.path.join(CSRC, "k_hash_quad.hip")) as f:
        text = f.read()
    assert '#include "hash_sample.hpp"' in text
    for fn in ("hsample::stream_open", "hsample::skip_candidate", "hsample::gen_fq", "hsample::gen_bool", "FQ_RAND_M"):
        assert fn in text, fn
