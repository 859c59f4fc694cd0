// Lagrange coefficients at 0 of a position list in the scalar field of a curve group (secp256k1 n, ristretto255 l):
//   lambda_i = prod_{j != i} x_j / (x_j - x_i)  mod n          (participant.rs:1518-1557, 1955-2002)
// as the 32-byte scalar a share is multiplied by.  One coefficient per lane; plain C++ (host + device) so that the very functions
// the kernel body calls (k_ec_lagrange, ec_lagrange_kernels.hip) run on the CPU in tests/ec_lagrange_unit.cpp.
//
// Arithmetic.  Positions are >= 1 and below 2^63, pairwise different, so every factor x_j and |x_j - x_i| is a nonzero 64-bit value
// and a unit mod the prime order (above 2^252): lambda_i is one field element however it is computed, and "order - |lambda|" of the
// host path (capi_scalar.inc, ec_lagrange_scalar) for a negative coefficient is just that element.  Each factor is multiplied in by
// ScalarField::mont_step_u64, acc <- acc d 2^-64.  Starting from 1 the numerator and the denominator of lane i both take exactly
// m - 1 steps (the lane's own index is skipped in both), so
//   num = 2^(-64 (m-1)) prod x_j,   den = 2^(-64 (m-1)) prod |x_j - x_i|,
// and the stray power cancels in num / den.  The quotient: den R by one mont_mul with R^2, its inverse den^-1 R by Fermat
// (inv_mont), then mont_mul(num, den^-1 R) = num / den, reduced and out of the Montgomery domain.  The sign is the parity of the
// negative differences, kept aside; the value is negated mod n when it is odd (never 0 for admissible positions).
// A zero difference (duplicate positions never reach the kernel: the host refuses them first) makes den = 0, inv_mont(0) = 0 and
// the result 0: nothing faults and no loop depends on the data.
#pragma once
#include <stddef.h>

#include <vector>

#include "ec_scalar.h"

namespace ec {

constexpr int LAGRANGE_WG = 64;        // lanes of a workgroup: the coefficients of one tile
constexpr int LAGRANGE_STAGE = 256;    // positions of the list staged through LDS at a time (2 KiB)

struct LagrangeLane {
  Sc num, den;
  bool neg;
};

EC_HD void lagrange_begin(LagrangeLane& s) {
#pragma unroll
  for (int k = 0; k < 8; ++k) s.num.v[k] = s.den.v[k] = k == 0 ? 1u : 0u;
  s.neg = false;
}

// the factors of the positions x[0 .. cnt) except x[skip] (skip < 0: none is the lane's own) into the lane of position xi
template <class O>
EC_HD void lagrange_accumulate(LagrangeLane& s, int64_t xi, const int64_t* x, int cnt, int skip) {
  for (int k = 0; k < cnt; ++k) {
    if (k == skip) continue;
    const uint64_t xj = (uint64_t)x[k];                  // `position as u64`
    ScalarField<O>::mont_step_u64(s.num, xj);
    uint64_t d = xj - (uint64_t)xi;                      // |x_j - x_i| < 2^63: both lie in [1, 2^63)
    const bool below = (int64_t)d < 0;
    if (below) d = 0 - d;
    s.neg ^= below;
    ScalarField<O>::mont_step_u64(s.den, d);
  }
}

// lambda = num / den, negated mod n for an odd number of negative differences
template <class O>
EC_HD void lagrange_finish(Sc& lambda, const LagrangeLane& s) {
  typedef ScalarField<O> F;
  Sc r2, d;
#pragma unroll
  for (int k = 0; k < 8; ++k) r2.v[k] = O::r2(k);
  F::mont_mul(d, s.den, r2);              // den R
  F::inv_mont(d, d);                      // den^-1 R
  F::mont_mul(lambda, s.num, d);          // num den^-1, reduced
  u32 any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) any |= lambda.v[k];
  if (s.neg && any) {
    u64 borrow = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const u64 t = (u64)O::n(k) - lambda.v[k] - borrow;
      lambda.v[k] = (u32)t;
      borrow = (t >> 63) & 1;
    }
  }
}

// 32 bytes in the group's scalar byte order (secp256k1 big-endian, ristretto255 little-endian)
template <bool BE>
EC_HD void lagrange_store(uint8_t* b, const Sc& a) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint8_t* q = BE ? b + 28 - 4 * i : b + 4 * i;
    const u32 v = a.v[i];
    if (BE) { q[0] = (uint8_t)(v >> 24); q[1] = (uint8_t)(v >> 16); q[2] = (uint8_t)(v >> 8); q[3] = (uint8_t)v; }
    else { q[0] = (uint8_t)v; q[1] = (uint8_t)(v >> 8); q[2] = (uint8_t)(v >> 16); q[3] = (uint8_t)(v >> 24); }
  }
}

// The tile table of one launch, in the manner of many::tile_table: a tile is up to LAGRANGE_WG consecutive coefficients of ONE
// list, one workgroup.  Appends {the list's first position, m, the tile's first coefficient, live lanes} for every tile of a list
// of m positions that starts at `first` in the launch's concatenated positions; coefficient c belongs to position c.
inline void lagrange_tiles(size_t first, size_t m, std::vector<uint32_t>& out) {
  for (size_t off = 0; off < m; off += LAGRANGE_WG) {
    const size_t live = m - off < (size_t)LAGRANGE_WG ? m - off : (size_t)LAGRANGE_WG;
    const uint32_t row[4] = {(uint32_t)first, (uint32_t)m, (uint32_t)(first + off), (uint32_t)live};
    out.insert(out.end(), row, row + 4);
  }
}

}  // namespace ec

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// out[32 c ..] = the coefficient of position c for every tile of `tiles` (lagrange_tiles rows, device memory); group 1 =
// secp256k1, 2 = ristretto255.  positions: the launch's lists back to back, device memory.
extern "C" int ec_lagrange_launch(int group, const int64_t* positions, const uint32_t* tiles, int ntiles, uint8_t* out, hipStream_t s);
#endif
