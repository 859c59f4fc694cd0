// Run-time MODP groups of 512-byte elements (moduli of 3073 .. 4096 bits, RFC 3526 group 16 among them): the kernel
// templates of modp_rt_kernels.inc at 36 limbs per lane, the one width at which bn::mont_mul carries a column a second time
// half way down its lane (bn_quad.h, `if constexpr (K > 27)`).  Built with -mllvm -pragma-unroll-threshold=200000 (Makefile)
// like modp_rt_kernels_wide.hip: the 36 x 36 row loop of a product must be unrolled completely, or its accumulators turn into
// a dynamically indexed array in scratch memory.  modp_rt_kernels.hip reaches these launchers by name.
#include "modp_rt_kernels.h"

#define RT_FN(name) modp_rt36_##name
#define RT_ELSEWHERE(name, lpl, ...)
#define RT_DISPATCH(lpl, KERNEL, ...)                                                          \
  do {                                                                                         \
    if ((lpl) == 36) hipLaunchKernelGGL(KERNEL<36>, __VA_ARGS__);                              \
    else return (int)hipErrorInvalidValue;                                                     \
  } while (0)

#define RT_DISPATCH_FN(lpl, FN, ...) ((lpl) == 36 ? FN<36>(__VA_ARGS__) : (int)hipErrorInvalidValue)

#include "modp_rt_kernels.inc"
