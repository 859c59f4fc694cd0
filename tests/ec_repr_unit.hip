// Test helper (built by `make examples` into tests/_build/ec_repr_unit, run by tests/test_gpu_ec_repr.py): the one-lane point
// operations of mpvss_rs_amd/csrc/ec_curves.h on operands given as RAW LIMB WORDS, one case per lane -- the body is
// tests/ec_repr_ops.h, the same that tests/ec_host_shim.cpp compiles for the CPU; the cases (saturated limbs in every position,
// non-canonical identities) and the expected bytes are those of tests/ec_repr_cases.py.
//   ec_repr_unit <1 secp256k1 | 2 ristretto255 | 3 secp256k1 encode_batch<8>> <in.bin> <n> <out.bin>
//     modes 1, 2: in.bin  n x (P, Q) of 30 / 40 u32 words each;  out.bin  n x REPR_SLOTS x 33 / 32 bytes
//     mode 3:     in.bin  n x 8 points of 30 words;               out.bin  n x 8 x 33 bytes
// exit code 0 when the kernel ran and out.bin is written; the comparison is the caller's
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ec_repr_ops.h"

using namespace ec;

#define CHECK(x)                                                                       \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } \
  } while (0)

template <class C>
__global__ void __launch_bounds__(64) k_pairs(const u32* __restrict__ in, int n, uint8_t* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  constexpr int PW = C::POINT_WORDS;
  repr_pair<C>(in + (size_t)i * 2 * PW, in + (size_t)i * 2 * PW + PW, out + (size_t)i * REPR_SLOTS * C::ENC_LEN);
}
__global__ void __launch_bounds__(64) k_batch8(const u32* __restrict__ in, int n, uint8_t* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  repr_batch8(in + (size_t)i * 8 * 30, out + (size_t)i * 8 * 33);
}

int main(int argc, char** argv) {
  if (argc != 5) { fprintf(stderr, "usage: ec_repr_unit <mode> <in.bin> <n> <out.bin>\n"); return 2; }
  const int mode = atoi(argv[1]), n = atoi(argv[3]);
  if (mode < 1 || mode > 3 || n < 1 || n > (1 << 20)) { fprintf(stderr, "bad mode or count\n"); return 2; }
  const size_t in_words = (size_t)n * (mode == 1 ? 60 : mode == 2 ? 80 : 240);
  const size_t out_bytes = (size_t)n * (mode == 1 ? REPR_SLOTS * 33 : mode == 2 ? REPR_SLOTS * 32 : 8 * 33);
  std::vector<u32> in(in_words);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(in.data(), 4, in.size(), f) != in.size()) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
  fclose(f);
  u32* din;
  uint8_t* dout;
  CHECK(hipMalloc(&din, in_words * 4));
  CHECK(hipMalloc(&dout, out_bytes));
  CHECK(hipMemcpy(din, in.data(), in_words * 4, hipMemcpyHostToDevice));
  CHECK(hipMemset(dout, 0xee, out_bytes));
  const dim3 grid((n + 63) / 64), block(64);
  if (mode == 1)
    hipLaunchKernelGGL(k_pairs<Secp>, grid, block, 0, 0, din, n, dout);
  else if (mode == 2)
    hipLaunchKernelGGL(k_pairs<Ristretto>, grid, block, 0, 0, din, n, dout);
  else
    hipLaunchKernelGGL(k_batch8, grid, block, 0, 0, din, n, dout);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<uint8_t> res(out_bytes);
  CHECK(hipMemcpy(res.data(), dout, out_bytes, hipMemcpyDeviceToHost));
  f = fopen(argv[4], "wb");
  if (!f || fwrite(res.data(), 1, res.size(), f) != res.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
  printf("ran %d\n", n);
  return 0;
}
