// HBH_IMPL_OCT, generator mode 0 (both P read per check) and the dispatcher (k_oct.hpp).
#define HS_MULFN static __device__ __noinline__
#include "k_oct.hpp"

namespace hbl {

hipError_t oct_verify_g0(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                          uint8_t* verdict, uint32_t* value_out) {
  return lane_launch<OctKernels, 0>(s, n, d1, d2, flags, verdict, value_out);
}

hipError_t oct_verify(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                       uint8_t* verdict, uint32_t* value_out) {
  if (n <= 0) return hipSuccess;
  const int gen = pair_gen_mode(d1, d2);
  if (gen == 1) return oct_verify_g1(s, n, d1, d2, flags, verdict, value_out);
  if (gen == 2) return oct_verify_g2(s, n, d1, d2, flags, verdict, value_out);
  return oct_verify_g0(s, n, d1, d2, flags, verdict, value_out);
}

}  // namespace hbl
