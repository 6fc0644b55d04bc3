// HBH_IMPL_QUAD, generator mode 0 (both P read per check) and the dispatcher (k_quad.hpp).
#define HS_MULFN static __device__ __noinline__
#include "k_quad.hpp"

namespace hbl {

hipError_t quad_verify_g0(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                          uint8_t* verdict, uint32_t* value_out) {
  return lane_launch<QuadKernels, 0>(s, n, d1, d2, flags, verdict, value_out);
}

hipError_t quad_verify(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                       uint8_t* verdict, uint32_t* value_out) {
  if (n <= 0) return hipSuccess;
  const int gen = pair_gen_mode(d1, d2);
  if (gen == 1) return quad_verify_g1(s, n, d1, d2, flags, verdict, value_out);
  if (gen == 2) return quad_verify_g2(s, n, d1, d2, flags, verdict, value_out);
  return quad_verify_g0(s, n, d1, d2, flags, verdict, value_out);
}

}  // namespace hbl
