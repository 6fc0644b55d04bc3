"""The sampler in front of the device form of hash_g2 (hbbft_amd/csrc/hash_sample.hpp, used by
k_hash.hip) on the host: a stand-alone program includes the header and, for 64 seeds, prints 40
draws in the sampler's own order (gen_fq, gen_fq, gen_bool, ...) with the stream position after each.
The test compares every draw and every position with oracle.tc.ChaChaRng:

* gen_fq's limbs are pairing's Montgomery representation, so limbs * 2^-384 mod p is the oracle's value;
* a position is (block, word) = divmod(stream words consumed, 16);
* the seed set contains sha3(b"hbh-trial-78"), whose stream makes gen_fq redraw;
* a stream reopened at a printed position continues with the same words (how the kernel carries a
  message from one sampling round to the next).

The constant that takes gen_fq's limbs into the device field's Montgomery form is checked here too.
"""
import hashlib
import os
import re
import shutil
import subprocess

import pytest

from oracle import tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hbbft_amd", "csrc")
NDRAW = 40

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hash_sample.hpp"
using namespace hsample;

static void draw(Stream& s, int k) {
  if (k % 3 == 2) {
    std::printf("B %d", gen_bool(s) ? 1 : 0);
  } else {
    uint32_t w[12];
    if (!gen_fq(s, w)) std::printf("X");
    std::printf("F ");
    for (int i = 11; i >= 0; i--) std::printf("%08x", w[i]);
  }
  std::printf(" %llu %u\n", (unsigned long long)s.block, s.word);
}

int main(int argc, char** argv) {
  const int ndraw = std::atoi(argv[1]);
  for (int a = 2; a < argc; a++) {
    uint8_t seed[32];
    for (int i = 0; i < 32; i++) {
      unsigned v;
      std::sscanf(argv[a] + 2 * i, "%2x", &v);
      seed[i] = (uint8_t)v;
    }
    Stream s;
    stream_open(s, seed);
    uint64_t block = 0;
    uint32_t word = 0;
    for (int k = 0; k < ndraw; k++) {
      if (k == ndraw / 2) {  // go on from the saved position alone, as the next kernel round does
        Stream t;
        stream_open(t, seed, block, word);
        s = t;
      }
      draw(s, k);
      block = s.block;
      word = s.word;
    }
  }
  return 0;
}
"""


def seeds():
    return [hashlib.sha3_256(b"hbh-trial-%d" % i).digest() for i in range(16, 80)]


@pytest.fixture(scope="module")
def draws(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++) to build the sampler program")
    d = tmp_path_factory.mktemp("hash_sample")
    src, exe = d / "sample.cpp", d / "sample"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe), str(NDRAW)] + [s.hex() for s in seeds()], capture_output=True, text=True, check=True)
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 64 * NDRAW
    return [lines[k * NDRAW:(k + 1) * NDRAW] for k in range(64)]


def consumed(rng):
    """stream words the oracle's generator has handed out"""
    return (rng.counter - 1) * 16 + rng.idx if rng.buf else 0


def test_draws_and_positions_match_the_oracle(draws):
    rinv = pow(1 << 384, tc.P - 2, tc.P)
    redraws = {}
    for k, (seed, lines) in enumerate(zip(seeds(), draws)):
        rng = tc.ChaChaRng(seed)
        nfq = 0
        for j, line in enumerate(lines):
            kind, val, block, word = line.split()
            if j % 3 == 2:
                assert kind == "B" and int(val) == int(rng.gen_bool()), (k, j)
            else:
                nfq += 1
                limbs = int(val, 16)
                assert kind == "F" and limbs < tc.P and limbs >> 381 == 0, (k, j)
                assert limbs * rinv % tc.P == rng.gen_fq(), (k, j)
            assert (int(block), int(word)) == divmod(consumed(rng), 16), (k, j)
        redraws[k] = (consumed(rng) - (NDRAW - nfq) - 12 * nfq) // 12
    # the inputs exercise the redraw loop: a draw is >= p with probability 0.187
    assert redraws[78 - 16] >= 1
    assert sum(redraws.values()) > 64


def test_montgomery_conversion_constant():
    """gen_fq's limbs L stand for L 2^-384; the device field keeps v as v 2^392, so the conversion is one
    Montgomery product (which divides by 2^392) by 2^400 mod p, stored in 28-bit limbs."""
    with open(os.path.join(CSRC, "constants.hpp")) as f:
        m = re.search(r"FQ_RAND_M\[NL\] = \{([^}]*)\}", f.read())
    limbs = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
    assert len(limbs) == 14 and all(l < 1 << 28 for l in limbs)
    c = sum(l << (28 * i) for i, l in enumerate(limbs))
    assert c == pow(2, 400, tc.P)
    L = 0x123456789ABCDEF << 300
    assert L * c * pow(1 << 392, tc.P - 2, tc.P) % tc.P == (L * pow(1 << 384, tc.P - 2, tc.P) % tc.P) * (1 << 392) % tc.P


def test_kernel_uses_the_header():
    with open(os.path.join(CSRC, "k_hash.hip")) as f:
        text = f.read()
    assert '#include "hash_sample.hpp"' in text
    for fn in ("hsample::stream_open", "hsample::gen_fq", "hsample::gen_bool", "FQ_RAND_M"):
        assert fn in text, fn
