// Internal launch interface between the C-ABI layer (capi_modp_rt.inc) and the kernels of a run-time MODP group
// (modp_rt_kernels.hip, bn_quad_rt.h).  Every array of limbs holds numbers of L = 4 lpl limbs, stride L words.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define MODP_RT_MAX_LIMBS 72

/* device image of a group's constants (built by the host from the modulus alone) */
typedef struct modp_rt_consts {
  uint32_t n[MODP_RT_MAX_LIMBS];      /* N, L limbs of 29 bits (zero above) */
  uint32_t kin[MODP_RT_MAX_LIMBS];    /* 2^(29 (IN_ROWS + L)) mod N: a 2048-bit input times this, one long product -> x R mod N */
  uint32_t one_m[MODP_RT_MAX_LIMBS];  /* R mod N (Montgomery one) */
  uint32_t one[MODP_RT_MAX_LIMBS];    /* plain 1 (leaves the Montgomery domain) */
  uint32_t n0inv;                     /* -N^-1 mod 2^29 */
  uint32_t lpl;                       /* limbs per lane: 5, 9 or 18 */
  uint32_t qm1_lo, qm1_hi;            /* q - 1 when it is below 2^64 (positions are reduced by it), else 0 */
} modp_rt_consts;

#ifdef __cplusplus
extern "C" {
#endif
/* IN_ROWS of a width (rows of the long product that takes a 2048-bit input) */
int modp_rt_in_rows(int lpl);
/* out_m[x] = in[x] R mod N (< 2N), any 256-byte big-endian input */
int modp_rt_launch_to_mont(int lpl, const uint8_t* in_be, int count, uint32_t* out_m, const modp_rt_consts* cs, hipStream_t s);
/* tab[x][d] = base[x]^d R mod N, d < 16 (base_stride 0: one base for every x) */
int modp_rt_launch_table(int lpl, const uint8_t* base_be, size_t base_stride, int count, uint32_t* tab, const modp_rt_consts* cs,
                         hipStream_t s);
/* out[x] = B1[x]^e1[x] * B2[x]^e2[x] mod q, canonical 256-byte big-endian; tab1/tab2: 16-entry tables (stride in words, 0 = shared),
   tab2 == NULL: B1^e1 alone; exponent strides in bytes (0 = one exponent for every x) */
int modp_rt_launch_dual_exp(int lpl, const uint32_t* tab1, size_t tab1_stride, const uint32_t* tab2, size_t tab2_stride,
                            const uint8_t* e1, size_t e1_stride, const uint8_t* e2, size_t e2_stride, int count, uint8_t* out,
                            const modp_rt_consts* cs, hipStream_t s);
/* fixed-base comb of one base shared by every share: comb[k][d] = base^(d 16^k) R mod N, k < 512, d < 16 --
   modp_rt_comb_bytes(lpl) bytes (2.25 MiB at 18 limbs per lane, 1.125 MiB at 9, 640 KiB at 5).  The base is a 256-byte value
   of any size on the device. */
size_t modp_rt_comb_bytes(int lpl);
int modp_rt_launch_comb_build(int lpl, const uint8_t* base_be, uint32_t* comb, const modp_rt_consts* cs, hipStream_t s);
/* out[x] = base^e1[x] * B2[x]^e2[x] mod q, canonical: e1 over the comb with no squarings, e2 left to right over B2's 16-entry
   table (tab2 == NULL: base^e1 alone; tab2_stride in words, e2_stride in bytes, 0 = one exponent for every x); e1 n x 256 bytes */
int modp_rt_launch_comb_exp(int lpl, const uint32_t* comb, const uint32_t* tab2, size_t tab2_stride, const uint8_t* e1,
                            const uint8_t* e2, size_t e2_stride, int count, uint8_t* out, const modp_rt_consts* cs, hipStream_t s);
/* out1[x] = B[x]^e1[x], out2[x] = B[x]^e2[x] from the base's one table, two left-to-right exponent sets in one launch
   (gridDim.y = 2); exponents and results n x 256 bytes */
int modp_rt_launch_exp_sets(int lpl, const uint32_t* tab, size_t tab_stride, const uint8_t* e1, const uint8_t* e2, int count,
                            uint8_t* out1, uint8_t* out2, const modp_rt_consts* cs, hipStream_t s);
/* the same two results right to left with shared squarings (k_rt_twin_exp): bases as 256-byte values of any size, `buckets`
   a scratch of modp_rt_twin_scratch_bytes(lpl, count) bytes that holds exponent windows afterwards (the caller zeroes it) */
size_t modp_rt_twin_scratch_bytes(int lpl, int count);
int modp_rt_launch_twin_exp(int lpl, const uint8_t* bases, const uint8_t* e1, const uint8_t* e2, int count, uint32_t* buckets,
                            uint8_t* out1, uint8_t* out2, const modp_rt_consts* cs, hipStream_t s);
/* out[x] = a[x] b[x] mod q, canonical, from a R and b R (modp_rt_launch_to_mont) */
int modp_rt_launch_mul(int lpl, const uint32_t* a_m, const uint32_t* b_m, int count, uint8_t* out, const modp_rt_consts* cs, hipStream_t s);
/* X[x] = Horner in the exponent over the commitments cm_m ([t] numbers in Montgomery form) at i' = positions[x] mod (q-1) */
int modp_rt_launch_commit_eval(int lpl, const uint32_t* cm_m, int t, const int64_t* positions, int count, uint8_t* x_be,
                               const modp_rt_consts* cs, hipStream_t s);
#ifdef __cplusplus
}
#endif
