// Run-time MODP groups of 256-byte elements (moduli of at most 2048 bits): the kernel templates of modp_rt_kernels.inc at
// 5, 9 and 18 limbs per lane, and the launch interface of modp_rt_kernels.h, which hands the wider widths over: 27 limbs per
// lane to modp_rt_kernels_wide.hip and 36 to modp_rt_kernels_4096.hip -- translation units of their own because their row
// loops need another unroll threshold.
#include "modp_rt_kernels.h"

#define RT_FN(name) modp_rt_##name
#define RT_ELSEWHERE(name, lpl, ...)                            \
  if ((lpl) == 27) return modp_rt27_##name((lpl), __VA_ARGS__); \
  if ((lpl) == 36) return modp_rt36_##name((lpl), __VA_ARGS__)
#define RT_DISPATCH(lpl, KERNEL, ...)                                                          \
  do {                                                                                         \
    if ((lpl) == 5) hipLaunchKernelGGL(KERNEL<5>, __VA_ARGS__);                                \
    else if ((lpl) == 9) hipLaunchKernelGGL(KERNEL<9>, __VA_ARGS__);                           \
    else if ((lpl) == 18) hipLaunchKernelGGL(KERNEL<18>, __VA_ARGS__);                         \
    else return (int)hipErrorInvalidValue;                                                     \
  } while (0)

#define RT_FD_ELSEWHERE modp_rtfd_launch_fd_chains
// a host function template of the width: FN<lpl>(args)
#define RT_DISPATCH_FN(lpl, FN, ...) \
  ((lpl) == 5 ? FN<5>(__VA_ARGS__) : (lpl) == 9 ? FN<9>(__VA_ARGS__) : (lpl) == 18 ? FN<18>(__VA_ARGS__) : (int)hipErrorInvalidValue)

#define RT_WIDTH_FREE   // the kernel that has no width (k_rt_spread_challenge) lives in this unit alone

#include "modp_rt_kernels.inc"

// what the host needs to know of a width: none of it launches anything
extern "C" int modp_rt_elem_bytes(int lpl) {
  return lpl == 36 ? Width<36>::EB : lpl == 27 ? Width<27>::EB : (lpl == 5 || lpl == 9 || lpl == 18) ? Width<18>::EB : -1;
}

extern "C" int modp_rt_in_rows(int lpl) {
  return lpl == 5 ? Width<5>::IN_ROWS : lpl == 9 ? Width<9>::IN_ROWS : lpl == 18 ? Width<18>::IN_ROWS : lpl == 27 ? Width<27>::IN_ROWS
         : lpl == 36 ? Width<36>::IN_ROWS : -1;
}

extern "C" size_t modp_rt_comb_bytes(int lpl) {
  return (size_t)rt_comb_rows(lpl) * 16 * 4 * lpl * sizeof(uint32_t);
}

extern "C" size_t modp_rt_twin_scratch_bytes(int lpl, int count) {
  return (size_t)rt_grid(count) * RT_NUMS * 2 * RT_TWIN_BUCKETS * 4 * lpl * sizeof(uint32_t);
}

extern "C" size_t modp_rt_keyset_bytes(int lpl, size_t count) {
  if (lpl != 5 && lpl != 9 && lpl != 18 && lpl != 27 && lpl != 36) return 0;
  return count * (size_t)rt_ks_rows(lpl) * 16 * 4 * lpl * sizeof(uint32_t);
}

extern "C" int modp_rt_fd_max_t(int lpl) { return (lpl == 5 || lpl == 9 || lpl == 18 || lpl == 27 || lpl == 36) ? MODP_RT_FD_MAX_T(lpl) : -1; }

extern "C" size_t modp_rt_fd_park_bytes(int lpl, int t, int S) { return (size_t)S * 2 * (16 * ((t + 15) / 16)) * 4 * lpl * sizeof(uint32_t); }
