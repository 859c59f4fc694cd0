// Key sets of the curve groups for gfx950 (ec_keyset.h holds the bodies): the per-key comb in HBM and the walk over it.
//   k_*_keyset_build_bases   one key per lane: decode, validity, identity mark, the 65 window bases 16^w y
//   k_*_keyset_build_rows    one (key, window) per lane: the window's eight affine entries, one inversion for the eight
//   k_*_keyset_walk    one share per lane, blockIdx.y = the scalar set (P(i) / w of the dealer): 65 mixed additions
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ec_keyset.h"
#include "ec_kernels.h"

using namespace ec;

namespace {

constexpr int KS_THREADS = 64;

template <class C>
__device__ __forceinline__ void bases_kernel_body(const uint8_t* __restrict__ enc, int count, u32* __restrict__ rows,
                                                  uint8_t* __restrict__ ok, uint8_t* __restrict__ marks) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= count) return;
  keyset_bases_body<C>(enc + (size_t)x * C::ENC_LEN, rows + (size_t)x * KeysetGeom<C>::ROW_WORDS, ok + x, marks + x);
}

template <class C>
__device__ __forceinline__ void rows_kernel_body(int count, u32* __restrict__ rows) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)count * KS_WINDOWS) return;
  keyset_window_body<C>(rows + (size_t)g * KeysetGeom<C>::WINDOW_WORDS);       // (key, window) = (g / 65, g % 65): windows are contiguous
}

// Share x of scalar set blockIdx.y walks the row of key x (the caller passes the rows and marks of key key_offset).
// The loop body is one mixed addition: the WHOLE kernel is 24 KB of code for secp256k1 and 15 KB for ristretto255, inside the
// 64 KB instruction cache with room (dual_win_body's doubling-and-addition body alone is about 50 KB).  Compiler's figures,
// gfx950: 189 VGPRs / 2 waves per SIMD (secp256k1), 160 / 3 (ristretto255), no scratch; an entry arrives as 4 / 6 16-byte loads.
template <class C>
__device__ __forceinline__ void walk_kernel_body(const u32* __restrict__ rows, const uint8_t* __restrict__ marks,
                                                 const uint8_t* __restrict__ k1, const uint8_t* __restrict__ k2, int count,
                                                 u32* __restrict__ out1, u32* __restrict__ out2) {
  const int xi = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = xi < count;
  const int x = live ? xi : count - 1;          // a dead lane walks a live share's row and stores nothing
  const uint8_t* k = (blockIdx.y == 0 ? k1 : k2) + (size_t)x * 32;
  u32* out = blockIdx.y == 0 ? out1 : out2;
  typename C::Point acc;
  keyset_walk_body<C>(acc, rows + (size_t)x * KeysetGeom<C>::ROW_WORDS, marks[x] != 0, k);
  if (live) ks_store_point<C>(out + (size_t)x * C::POINT_WORDS, acc);
}

}  // namespace

#define EC_KEYSET_KERNELS(NAME, CURVE)                                                                                       \
  extern "C" __global__ void __launch_bounds__(KS_THREADS) k_##NAME##_keyset_build_bases(const uint8_t* enc, int count, u32* rows, \
                                                                                   uint8_t* ok, uint8_t* marks) {            \
    bases_kernel_body<CURVE>(enc, count, rows, ok, marks);                                                                   \
  }                                                                                                                          \
  extern "C" __global__ void __launch_bounds__(KS_THREADS) k_##NAME##_keyset_build_rows(int count, u32* rows) {                    \
    rows_kernel_body<CURVE>(count, rows);                                                                                    \
  }                                                                                                                          \
  extern "C" __global__ void __launch_bounds__(KS_THREADS) k_##NAME##_keyset_walk(                                           \
      const u32* rows, const uint8_t* marks, const uint8_t* k1, const uint8_t* k2, int count, u32* out1, u32* out2) {        \
    walk_kernel_body<CURVE>(rows, marks, k1, k2, count, out1, out2);                                                         \
  }

EC_KEYSET_KERNELS(secp, Secp)
EC_KEYSET_KERNELS(rist, Ristretto)

extern "C" size_t ec_keyset_row_words(int group) {
  return group == 1 ? (size_t)KeysetGeom<Secp>::ROW_WORDS : (size_t)KeysetGeom<Ristretto>::ROW_WORDS;
}

// the build of `count` keys (count * 65 must fit an int: the caller chunks); k_*_keyset_build is this pair of launches
extern "C" int ec_launch_keyset_build(int group, const uint8_t* enc, int count, uint32_t* rows, uint8_t* ok, uint8_t* marks,
                                      hipStream_t s) {
  if (count <= 0) return 0;
  const unsigned gb = (unsigned)((count + KS_THREADS - 1) / KS_THREADS);
  const unsigned gr = (unsigned)(((long long)count * KS_WINDOWS + KS_THREADS - 1) / KS_THREADS);
  if (group == 1) {
    hipLaunchKernelGGL(k_secp_keyset_build_bases, dim3(gb), dim3(KS_THREADS), 0, s, enc, count, rows, ok, marks);
    hipLaunchKernelGGL(k_secp_keyset_build_rows, dim3(gr), dim3(KS_THREADS), 0, s, count, rows);
  } else {
    hipLaunchKernelGGL(k_rist_keyset_build_bases, dim3(gb), dim3(KS_THREADS), 0, s, enc, count, rows, ok, marks);
    hipLaunchKernelGGL(k_rist_keyset_build_rows, dim3(gr), dim3(KS_THREADS), 0, s, count, rows);
  }
  return (int)hipGetLastError();
}

// out1[x] = k1[x] * y_x and (k2 != null) out2[x] = k2[x] * y_x in internal coordinates; rows / marks: those of the first key
extern "C" int ec_launch_keyset_walk(int group, const uint32_t* rows, const uint8_t* marks, const uint8_t* k1, const uint8_t* k2,
                                     int count, uint32_t* out1, uint32_t* out2, hipStream_t s) {
  if (count <= 0) return 0;
  const dim3 grid((unsigned)((count + KS_THREADS - 1) / KS_THREADS), k2 != nullptr ? 2 : 1);
  if (group == 1) hipLaunchKernelGGL(k_secp_keyset_walk, grid, dim3(KS_THREADS), 0, s, rows, marks, k1, k2, count, out1, out2);
  else hipLaunchKernelGGL(k_rist_keyset_walk, grid, dim3(KS_THREADS), 0, s, rows, marks, k1, k2, count, out1, out2);
  return (int)hipGetLastError();
}
