// HBH_IMPL_WAVEP: one wave per pairing check, WV_PACK checks per workgroup ("wave, packed", gfx950).
//
// k_wave.hip gives every check a workgroup of one wave.  Two kinds of stage of the final
// exponentiation then run far below the wave's width: the 31 cyclotomic-squaring runs (316 squarings
// held in registers) do useful work on 18 of 64 lanes (3 Fp4 squarings x 3 Fp2 squares x 2
// components), and the one inversion on 2.  They are ~45 % of a check's issue time.
//
// Here a workgroup is WV_PACK waves; wave w runs check blockIdx.x * WV_PACK + w through the same
// 32-pair stage programs (wave_prog.inc) in its own LDS region.  At a cyclotomic-squaring run or the
// inversion the waves meet at a workgroup barrier and ONE wave runs the stage for all WV_PACK checks
// in one instruction stream: 18 lanes per check (cyc_pack.hpp) or one lane pair per check.  The other
// waves wait at the next barrier and issue nothing.  648 k -> 492 k VALU instructions per check (442 k
// at three checks per workgroup, profiles/r08/pmc_wavep.json).
//
// The build parameters and what the A/B runs on the MI355X gave (profiles/r08/README.md; kernel ms
// for 4,096 sign-share checks, k_wave 5.09):
//   WV_PACK 2 / 3      three checks fill 54 lanes but leave two workgroups (6 waves) per CU at 256
//                      VGPRs, two leave four (8 waves, two per SIMD): 5.51 against 7.27-7.37.
//   WV_WAVE_SYNC       outside the packed stages a wave touches only its own region, so a
//                      wavefront-scope fence replaces the workgroup barrier of every stage phase:
//                      neutral without rotation (5.55 / 7.13), -3 % with it (5.16 -> 4.98 in the
//                      closing run).
//   WV_PACK_ROTATE     the packed stages take turns on the workgroup's waves instead of all landing
//                      on wave 0 (whose SIMD was the one every workgroup loaded): 5.55 -> 5.07.
//   WV_PACK_INV        the inversion packed as well: neutral (7.27-7.37 against 7.34), kept.
// As built the form beats k_wave by more than the cells' spread from 1,025 to 1,536 checks (2.46-2.48
// against 2.64-2.78 ms: k_wave needs a second wave on some SIMDs there), which is HBH_IMPL_AUTO's
// range for it (HBH_AUTO_WAVEP_MIN / MAX); it ties at 2,048 and 4,096 checks and loses below 1,025.
#define WV_NS hbsp
#define WV_PROG hbw
#define WV_THREADS 64
#define WV_FULL 0
#define WV_PACKED 1
#ifndef WV_PACK
#define WV_PACK 2
#endif
#ifndef WV_WAVE_SYNC
#define WV_WAVE_SYNC 1
#endif
#ifndef WV_PACK_ROTATE
#define WV_PACK_ROTATE 1
#endif
#include "wave_prog.inc"
#include "k_wave.hpp"

namespace hbl {

int wavep_pack() { return hbsp::WV_NPACK; }

hipError_t wavep_verify(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                        uint8_t* verdict, uint32_t* value_out) {
  if (n <= 0) return hipSuccess;
  if (flags & ~(WAVE_NEG_P2 | WAVE_CONJ_VALUE)) return hipErrorInvalidValue;  // plain checks only
  hbsp::WaveArgs a = {};
  a.n = n;
  const PairSideDesc* d[2] = {&d1, &d2};
  for (int k = 0; k < 2; k++) {
    a.s[k].p = (const uint32_t*)d[k]->p;
    a.s[k].q = (const uint32_t*)d[k]->q;
    a.s[k].lines = (const int4*)d[k]->lines;
    a.s[k].qinf = d[k]->qinf;
    a.s[k].idx = d[k]->idx;
    a.s[k].nq = (uint32_t)d[k]->nq;
  }
  a.flags = flags;
  a.verdict = verdict;
  a.value_out = value_out;
  constexpr int pack = hbsp::WV_NPACK;
  const size_t lds = (size_t)pack * hbsp::WV_REGION * 4;  // == pack * wave_lds_bytes()
  hipLaunchKernelGGL(hbsp::k_wave, dim3((unsigned)((n + pack - 1) / pack)), dim3(64 * pack), lds, s, a);
  return hipGetLastError();
}

}  // namespace hbl
