// The Miller-product kernel of the batched checks on lane octos (pair_side.hpp lane_miller_prod): 64
// items per workgroup, four tiles per group of HBH_BATCH_GROUP items.  One wave per SIMD, as k_oct_verify.
#define HS_MULFN static __device__ __noinline__
#include "pair_side.hpp"
#include "ofp.hpp"

namespace hbs {

__global__ void __launch_bounds__(256, 1) k_oct_miller_prod(MillerProdArgs a) {
  extern __shared__ uint32_t stash_lds[];
  lane_miller_prod<LaneOcto>(a, stash_lds);
}

}  // namespace hbs

namespace hbl {

hipError_t oct_miller_prod(hipStream_t s, int ntile, int n, const void* p, const void* q, int tpg, int nf,
                           uint32_t* out) {
  return miller_prod_launch(hbs::k_oct_miller_prod, s, ntile, n, p, q, tpg, nf, out);
}

}  // namespace hbl
