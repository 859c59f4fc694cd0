// k_ec_lagrange: the Lagrange coefficients of reconstruct for the curve groups, one coefficient per lane (ec_lagrange.h has the
// arithmetic and the reason the result equals the host path's byte for byte).  A translation unit of its own: the figures of the
// kernels in verdict_kernels.hip and ec_kernels.hip do not depend on it.
//
// One workgroup of LAGRANGE_WG lanes per tile of ONE list (ec::lagrange_tiles): the four words of its row are read once and are
// wave-uniform, so every loop bound and every barrier below is.  The list's m positions pass through LDS LAGRANGE_STAGE at a
// time; each lane multiplies all of them but its own into its numerator and its denominator.  Nothing at or past first + m is
// read: the next list's positions lie right there.  Lanes past the tile's live count only help to stage.
#include <hip/hip_runtime.h>

#include "ec_consts.h"
#include "ec_lagrange.h"

namespace {

template <class O, bool BE>
__global__ void __launch_bounds__(ec::LAGRANGE_WG)
k_ec_lagrange(const int64_t* __restrict__ positions, const uint32_t* __restrict__ tiles, uint8_t* __restrict__ out) {
  __shared__ int64_t stage[ec::LAGRANGE_STAGE];
  const uint32_t* row = tiles + 4 * (size_t)blockIdx.x;
  const uint32_t first = row[0], m = row[1], c0 = row[2], live = row[3];
  const uint32_t lane = threadIdx.x;
  const bool alive = lane < live;                       // c0 + lane < first + m for these
  const uint32_t i = c0 - first + lane;                 // the lane's index in its list
  const int64_t xi = alive ? positions[(size_t)c0 + lane] : 0;
  ec::LagrangeLane s;
  ec::lagrange_begin(s);
  for (uint32_t base = 0; base < m; base += ec::LAGRANGE_STAGE) {
    const uint32_t cnt = m - base < (uint32_t)ec::LAGRANGE_STAGE ? m - base : (uint32_t)ec::LAGRANGE_STAGE;
    for (uint32_t k = lane; k < cnt; k += ec::LAGRANGE_WG) stage[k] = positions[(size_t)first + base + k];
    __syncthreads();
    if (alive) ec::lagrange_accumulate<O>(s, xi, stage, (int)cnt, (i >= base && i - base < cnt) ? (int)(i - base) : -1);
    __syncthreads();
  }
  if (!alive) return;
  ec::Sc lambda;
  ec::lagrange_finish<O>(lambda, s);
  ec::lagrange_store<BE>(out + 32 * ((size_t)c0 + lane), lambda);
}

}  // namespace

extern "C" int ec_lagrange_launch(int group, const int64_t* positions, const uint32_t* tiles, int ntiles, uint8_t* out, hipStream_t s) {
  if (ntiles <= 0) return 0;
  if (group == 1)
    hipLaunchKernelGGL((k_ec_lagrange<ec::OrderSecp, true>), dim3(ntiles), dim3(ec::LAGRANGE_WG), 0, s, positions, tiles, out);
  else
    hipLaunchKernelGGL((k_ec_lagrange<ec::OrderEd, false>), dim3(ntiles), dim3(ec::LAGRANGE_WG), 0, s, positions, tiles, out);
  return (int)hipGetLastError();
}
