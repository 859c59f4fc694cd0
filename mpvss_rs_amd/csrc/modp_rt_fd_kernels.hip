// The forward-difference chain kernel of a run-time MODP group (k_rt_fd_chain, modp_rt_kernels.inc) at 5, 9 and 18 limbs per
// lane.  A unit of its own because of its build flag: sixteen waves of one workgroup leave a wave 128 registers, and at 18
// limbs per lane the product only stays inside them (120, no scratch) with -mllvm -pragma-unroll-threshold=200000 (Makefile);
// under the default threshold it spills 84 bytes per lane.  modp_rt_kernels.o keeps the default, which its own register
// figures depend on, and reaches this launcher by name.
#include "modp_rt_kernels.h"

#define RT_FD_ONLY
#define RT_FN(name) modp_rtfd_##name
#define RT_ELSEWHERE(name, lpl, ...)
#define RT_DISPATCH(lpl, KERNEL, ...) return (int)hipErrorInvalidValue
#define RT_DISPATCH_FN(lpl, FN, ...) \
  ((lpl) == 5 ? FN<5>(__VA_ARGS__) : (lpl) == 9 ? FN<9>(__VA_ARGS__) : (lpl) == 18 ? FN<18>(__VA_ARGS__) : (int)hipErrorInvalidValue)

#include "modp_rt_kernels.inc"
