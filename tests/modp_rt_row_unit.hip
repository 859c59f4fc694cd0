// Test helper (built by `make examples` into tests/_build/modp_rt_row_unit, run by tests/test_gpu_modp_rt_row_unit.py): ONE
// Montgomery product and ONE squaring of the run-time row layout (mpvss_rs_amd/csrc/bn_row_rt.h: 16 lanes per number) per operand
// pair, at the width named on the command line, compared by the test with Python integers.
//   modp_rt_row_unit <quad lpl: 18 | 27 | 36> <in.bin> <out.bin> <n>
// in.bin : u32 n0inv, L u32 limbs of the modulus N (radix 2^29), then n x 2 x L limbs: a, b      (L = 4 x quad lpl)
// out.bin: n x 2 x L limbs: a*b R^-1, a*a R^-1
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../mpvss_rs_amd/csrc/bn_row_rt.h"

#define CHECK(x)                                                                       \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } \
  } while (0)

using namespace bnrowrt;

template <int QL>
__global__ void __launch_bounds__(64) k_unit(const u32* __restrict__ hdr, const u32* __restrict__ in, u32* __restrict__ out, int count) {
  constexpr int L = 4 * QL, LPL = row_lpl(QL), SLOT = Slot<LPL>::WORDS;
  __shared__ __attribute__((aligned(16))) u32 lds[NUMS_PER_WAVE * SLOT + LDS_PAD];
  const Lane ln = make_lane();
  const int num = threadIdx.x >> 4;
  const int xi = blockIdx.x * NUMS_PER_WAVE + num;
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + num * SLOT;
  const u32 n0inv = hdr[0];
  u32 n[LPL], a[LPL], r[LPL];
  load_lane_limbs<LPL, L>(n, hdr + 1, ln);
  load_lane_limbs<LPL, L>(a, in + ((size_t)x * 2) * L, ln);
  slot_fill_from_global<LPL, L>(slot, in + ((size_t)x * 2 + 1) * L, ln);
  __builtin_amdgcn_wave_barrier();
  mont_mul<LPL, L>(r, a, slot, n, n0inv, ln);
  __builtin_amdgcn_wave_barrier();
  if (live) store_lane_limbs<LPL, L>(out + ((size_t)x * 2) * L, r, ln);
  slot_store<LPL>(slot, a, ln);
  __builtin_amdgcn_wave_barrier();
  mont_mul<LPL, L, true>(r, a, slot, n, n0inv, ln);
  __builtin_amdgcn_wave_barrier();
  if (live) store_lane_limbs<LPL, L>(out + ((size_t)x * 2 + 1) * L, r, ln);
}

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: modp_rt_row_unit lpl in.bin out.bin n\n"); return 1; }
  const int ql = atoi(argv[1]), n = atoi(argv[4]);
  if ((ql != 18 && ql != 27 && ql != 36) || n <= 0) { fprintf(stderr, "lpl is 18, 27 or 36; n >= 1\n"); return 1; }
  const size_t L = 4 * (size_t)ql;
  std::vector<uint32_t> hin(1 + L + (size_t)n * 2 * L), hout((size_t)n * 2 * L);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(hin.data(), 4, hin.size(), f) != hin.size()) { fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
  fclose(f);
  uint32_t *din, *dout;
  CHECK(hipMalloc(&din, hin.size() * 4));
  CHECK(hipMalloc(&dout, hout.size() * 4));
  CHECK(hipMemcpy(din, hin.data(), hin.size() * 4, hipMemcpyHostToDevice));
  const dim3 grid((n + NUMS_PER_WAVE - 1) / NUMS_PER_WAVE);
  if (ql == 18) hipLaunchKernelGGL(k_unit<18>, grid, dim3(64), 0, 0, din, din + 1 + L, dout, n);
  else if (ql == 27) hipLaunchKernelGGL(k_unit<27>, grid, dim3(64), 0, 0, din, din + 1 + L, dout, n);
  else hipLaunchKernelGGL(k_unit<36>, grid, dim3(64), 0, 0, din, din + 1 + L, dout, n);
  CHECK(hipGetLastError());
  CHECK(hipMemcpy(hout.data(), dout, hout.size() * 4, hipMemcpyDeviceToHost));
  f = fopen(argv[3], "wb");
  if (!f || fwrite(hout.data(), 4, hout.size(), f) != hout.size()) { fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
  fclose(f);
  return 0;
}
