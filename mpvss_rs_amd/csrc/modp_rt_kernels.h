// Internal launch interface between the C-ABI layer (capi_modp_rt.inc) and the kernels of a run-time MODP group
// (modp_rt_kernels.hip, modp_rt_kernels_wide.hip, modp_rt_kernels_4096.hip, bn_quad_rt.h).  Every array of limbs holds numbers of L = 4 lpl limbs,
// stride L words; every element, scalar and exponent is a big-endian value of EB = modp_rt_elem_bytes(lpl) bytes, stride EB.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define MODP_RT_MAX_LIMBS 144

/* device image of a group's constants (built by the host from the modulus alone) */
typedef struct modp_rt_consts {
  uint32_t n[MODP_RT_MAX_LIMBS];      /* N, L limbs of 29 bits (zero above) */
  uint32_t kin[MODP_RT_MAX_LIMBS];    /* 2^(29 (IN_ROWS + L)) mod N: an EB-byte input times this, one long product -> x R mod N */
  uint32_t one_m[MODP_RT_MAX_LIMBS];  /* R mod N (Montgomery one) */
  uint32_t one[MODP_RT_MAX_LIMBS];    /* plain 1 (leaves the Montgomery domain) */
  uint32_t n0inv;                     /* -N^-1 mod 2^29 */
  uint32_t lpl;                       /* limbs per lane: 5, 9, 18, 27 or 36 */
  uint32_t qm1_lo, qm1_hi;            /* q - 1 when it is below 2^64 (positions are reduced by it), else 0 */
} modp_rt_consts;

/* Forward differences (k_rt_fd_chain): the largest t a width's workgroup holds -- one level per DPP quad, 16 waves of at most
 * 128 registers at 5 / 9 / 18 limbs per lane, 8 waves of at most 256 at 27, 4 waves (one per SIMD) at 36 -- and the
 * one place that cuts n consecutive
 * positions into S chains (host and device): chain c is [first, first + len), len >= t when n / S >= t; its t seeds start at
 * first + (len - t) / 2. */
#define MODP_RT_FD_MAX_T(lpl) ((lpl) == 36 ? 64 : (lpl) == 27 ? 128 : 256)
static inline __host__ __device__ void modp_rt_fd_chain(int n, int S, int c, int* first, int* len) {
  const long long a = (long long)c * n / S, b = (long long)(c + 1) * n / S;
  *first = (int)a;
  *len = (int)(b - a);
}

/* k_rt_lagrange_terms: steps of a position list staged through LDS at a time (one position more than steps) */
#define MODP_RT_LAGRANGE_STAGE 256

#ifdef __cplusplus
extern "C" {
#endif
/* MODP_RT_FD_MAX_T of a width, -1 for no width */
int modp_rt_fd_max_t(int lpl);
/* HBM scratch of modp_rt_launch_fd_chains: one number per level, chain and direction */
size_t modp_rt_fd_park_bytes(int lpl, int t, int S);
/* bytes of an element / scalar / exponent of a width (256; 384 at 27 limbs per lane, 512 at 36), -1 for no width */
int modp_rt_elem_bytes(int lpl);
/* IN_ROWS of a width (rows of the long product that takes an EB-byte input) */
int modp_rt_in_rows(int lpl);
size_t modp_rt_comb_bytes(int lpl);
size_t modp_rt_twin_scratch_bytes(int lpl, int count);
/* bytes of the rows of `count` keys of a key set: EB / 32 rows of 16 numbers each (0 for no width) */
size_t modp_rt_keyset_bytes(int lpl, size_t count);
#define MODP_RT_FN(name) modp_rt_##name
#include "modp_rt_launchers.h"
#undef MODP_RT_FN
#define MODP_RT_FN(name) modp_rt27_##name
#include "modp_rt_launchers.h"
#undef MODP_RT_FN
#define MODP_RT_FN(name) modp_rt36_##name
#include "modp_rt_launchers.h"
#undef MODP_RT_FN
/* c_out[first + i] = c_box[box] (eb bytes each, eb a multiple of 4) for the live shares i of every tile of
 * modp_rt_launch_commit_eval_tiles' tile table: plain bytes, no width */
int modp_rt_launch_spread_challenge(const uint8_t* c_box, const uint32_t* tiles, int ntiles, int eb, uint8_t* c_out, hipStream_t s);
/* modp_rt_fd_kernels.hip: modp_rt_launch_fd_chains at 5, 9 and 18 limbs per lane */
int modp_rtfd_launch_fd_chains(int lpl, const uint32_t* seeds_m, int t, int n, int S, uint32_t* x_m, uint32_t* park,
                               const modp_rt_consts* cs, hipStream_t s);
/* modp_rt_row_kernels.hip: the row layout (bn_row_rt.h, 16 lanes per number) for small calls at 18, 27 and 36 limbs per lane --
 * any other lpl is hipErrorInvalidValue.  The argument lists of modp_rt_launch_dual_exp, _exp_sets and _comb_exp with a work
 * buffer in place of the results: out_m[x] = the result in Montgomery limbs below 2N, L words each (exp_sets: 2 count numbers,
 * the second set behind the first), which modp_rt_launch_from_mont turns into canonical bytes.  Not here: row variants of the
 * key-set, commit_eval, twin_exp and fd_chain kernels, handles at 5 / 9 limbs per lane, the pair layout. */
int modp_rt_row_launch_dual_exp(int lpl, const uint32_t* tab1, size_t tab1_stride, const uint32_t* tab2, size_t tab2_stride,
                                const uint8_t* e1, size_t e1_stride, const uint8_t* e2, size_t e2_stride, int count, uint32_t* out_m,
                                const modp_rt_consts* cs, hipStream_t s);
int modp_rt_row_launch_exp_sets(int lpl, const uint32_t* tab, size_t tab_stride, const uint8_t* e1, const uint8_t* e2, int count,
                                uint32_t* out_m, const modp_rt_consts* cs, hipStream_t s);
int modp_rt_row_launch_comb_exp(int lpl, const uint32_t* comb, const uint32_t* tab2, size_t tab2_stride, const uint8_t* e1,
                                const uint8_t* e2, size_t e2_stride, int count, uint32_t* out_m, const modp_rt_consts* cs, hipStream_t s);
#ifdef __cplusplus
}
#endif
