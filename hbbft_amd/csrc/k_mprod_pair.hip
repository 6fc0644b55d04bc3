// The Miller-product kernel of the batched checks on lane pairs (pair_side.hpp lane_miller_prod): 256
// items per workgroup, one tile per group of HBH_BATCH_GROUP items.  A translation unit of its own, as
// k_mprod_quad.hip and k_mprod_oct.hip, so the parallel build stays balanced.
#define HS_MULFN static __device__ __noinline__
#include "pair_side.hpp"

namespace hbs {

__global__ void __launch_bounds__(256, 2) k_pair_miller_prod(MillerProdArgs a) {
  extern __shared__ uint32_t stash_lds[];
  lane_miller_prod<LanePair>(a, stash_lds);
}

}  // namespace hbs

namespace hbl {

hipError_t pair_miller_prod(hipStream_t s, int ntile, int n, const void* p, const void* q, int tpg, int nf,
                            uint32_t* out) {
  return miller_prod_launch(hbs::k_pair_miller_prod, s, ntile, n, p, q, tpg, nf, out);
}

}  // namespace hbl
