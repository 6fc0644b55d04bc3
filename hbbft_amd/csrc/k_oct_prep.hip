// Line tables of shared G2 points on lane octos (the TABLE side of every pairing kernel).
//
// The serial 68-step walk of one shared point (63 doublings + 5 additions of |x|) with the lane-octo
// doubling and addition steps (ofp.hpp: 3 and 5 rounds of four Fp2 products), eight lanes per point;
// pair 0 of each octo writes the table (pair_side.hpp line_store), which every verify kernel reads
// unchanged (line_load).
//
// Point j of a launch writes position j of the outputs, or -- the slot-mapped form of a resident G2
// set (hbh_g2_set_add) -- position slot[j], where it also leaves its 48 affine ABI words in qout for
// the kernels that walk a side.
#include "launch.hpp"
#include "pair_side.hpp"
#include "ofp.hpp"

namespace hbs {

__global__ void __launch_bounds__(256, 1) k_oct_prep(int n, const uint32_t* __restrict__ q, int4* __restrict__ lines,
                                                     uint8_t* __restrict__ qinf, const uint32_t* __restrict__ slot,
                                                     uint32_t nslot, uint32_t* __restrict__ qout) {
  const int j = (int)((blockIdx.x * 256u + threadIdx.x) >> 3);
  if (j >= n) return;  // the eight lanes of an octo leave together
  const size_t at = slot ? slot[j] : (uint32_t)j;
  if (slot && at >= nslot) return;  // never write past the set (the host hands out slots < capacity)
  const uint32_t* w = q + (size_t)j * 48;
  const bool inf = lp_both(words_zero(w + (lp_even() ? 0 : 12), 12) && words_zero(w + (lp_even() ? 24 : 36), 12));
  Fp xQ, yQ;
  h_g2_load(w, xQ, yQ);
  if (inf) {
    xQ = h_one();
    yQ = h_one();
  }
  const bool writer = o_idx() == 0;
  if ((threadIdx.x & 7) == 0) qinf[at] = inf ? 1 : 0;
  if (qout) {  // six of the 48 words per lane of the octo
    const int l = (int)(threadIdx.x & 7);
    for (int k = 0; k < 6; k++) qout[at * 48 + 6 * l + k] = w[6 * l + k];
  }
  HJac T{xQ, yQ, h_one()};
  int4* base = lines + line_at(at * PAIR_STEPS);
  int step = 0;
#pragma unroll 1
  for (int b = 62; b >= 0; b--) {
#pragma unroll 1
    for (int add = 0; add < (((hb::X_ABS >> b) & 1) ? 2 : 1); add++) {
      const HLine l = add ? h_add_step_o(T, xQ, yQ) : h_dbl_step_o(T);
      if (writer) line_store(base + (size_t)step * LINE_Q4, l);
      step++;
    }
  }
}

}  // namespace hbs

namespace hbl {

hipError_t oct_prep(hipStream_t s, int n, const void* q, void* lines, uint8_t* qinf, const uint32_t* slot, size_t nslot,
                    void* qout) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(hbs::k_oct_prep, dim3((unsigned)((8 * (size_t)n + 255) / 256)), dim3(256), 0, s, n,
                     (const uint32_t*)q, (int4*)lines, qinf, slot, (uint32_t)nslot, (uint32_t*)qout);
  return hipGetLastError();
}

}  // namespace hbl
