// Run-time MODP groups of 384-byte elements (moduli of 2049 .. 3072 bits, RFC 3526 group 15 among them): the kernel
// templates of modp_rt_kernels.inc at 27 limbs per lane.  Built with -mllvm -pragma-unroll-threshold=200000 (Makefile): the
// 27 x 27 row loop of a product must be unrolled completely, or its accumulators turn into a dynamically indexed array in
// scratch memory.  modp_rt_kernels.hip, which keeps the compiler's default threshold, reaches these launchers by name.
#include "modp_rt_kernels.h"

#define RT_FN(name) modp_rt27_##name
#define RT_ELSEWHERE(name, lpl, ...)
#define RT_DISPATCH(lpl, KERNEL, ...)                                                          \
  do {                                                                                         \
    if ((lpl) == 27) hipLaunchKernelGGL(KERNEL<27>, __VA_ARGS__);                              \
    else return (int)hipErrorInvalidValue;                                                     \
  } while (0)

#define RT_DISPATCH_FN(lpl, FN, ...) ((lpl) == 27 ? FN<27>(__VA_ARGS__) : (int)hipErrorInvalidValue)

#include "modp_rt_kernels.inc"
