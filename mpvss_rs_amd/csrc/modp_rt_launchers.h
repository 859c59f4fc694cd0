// The launchers of a run-time MODP group, named by MODP_RT_FN: modp_rt_launch_* (modp_rt_kernels.h; every width) and, for
// modp_rt_kernels.hip alone, modp_rt27_launch_* (modp_rt_kernels_wide.hip; 27 limbs per lane only) and modp_rt36_launch_*
// (modp_rt_kernels_4096.hip; 36 only).  No include guard: it is included once per name.
/* out_m[x] = in[x] R mod N (< 2N), any EB-byte big-endian input */
int MODP_RT_FN(launch_to_mont)(int lpl, const uint8_t* in_be, int count, uint32_t* out_m, const modp_rt_consts* cs, hipStream_t s);
/* tab[x][d] = base[x]^d R mod N, d < 16 (base_stride 0: one base for every x) */
int MODP_RT_FN(launch_table)(int lpl, const uint8_t* base_be, size_t base_stride, int count, uint32_t* tab, const modp_rt_consts* cs,
                         hipStream_t s);
/* out[x] = B1[x]^e1[x] * B2[x]^e2[x] mod q, canonical EB-byte big-endian; tab1/tab2: 16-entry tables (stride in words, 0 = shared),
   tab2 == NULL: B1^e1 alone; exponent strides in bytes (0 = one exponent for every x) */
int MODP_RT_FN(launch_dual_exp)(int lpl, const uint32_t* tab1, size_t tab1_stride, const uint32_t* tab2, size_t tab2_stride,
                            const uint8_t* e1, size_t e1_stride, const uint8_t* e2, size_t e2_stride, int count, uint8_t* out,
                            const modp_rt_consts* cs, hipStream_t s);
/* fixed-base comb of one base shared by every share: comb[k][d] = base^(d 16^k) R mod N, k < 2 EB, d < 16 --
   modp_rt_comb_bytes(lpl) bytes (9.0 MiB at 36 limbs per lane, 5.06 MiB at 27, 2.25 MiB at 18, 1.125 MiB at 9, 640 KiB at 5).  The base is an
   EB-byte value of any size on the device. */
int MODP_RT_FN(launch_comb_build)(int lpl, const uint8_t* base_be, uint32_t* comb, const modp_rt_consts* cs, hipStream_t s);
/* out[x] = base^e1[x] * B2[x]^e2[x] mod q, canonical: e1 over the comb with no squarings, e2 left to right over B2's 16-entry
   table (tab2 == NULL: base^e1 alone; tab2_stride in words, e2_stride in bytes, 0 = one exponent for every x); e1 n x EB bytes */
int MODP_RT_FN(launch_comb_exp)(int lpl, const uint32_t* comb, const uint32_t* tab2, size_t tab2_stride, const uint8_t* e1,
                            const uint8_t* e2, size_t e2_stride, int count, uint8_t* out, const modp_rt_consts* cs, hipStream_t s);
/* out1[x] = B[x]^e1[x], out2[x] = B[x]^e2[x] from the base's one table, two left-to-right exponent sets in one launch
   (gridDim.y = 2); exponents and results n x EB bytes */
int MODP_RT_FN(launch_exp_sets)(int lpl, const uint32_t* tab, size_t tab_stride, const uint8_t* e1, const uint8_t* e2, int count,
                            uint8_t* out1, uint8_t* out2, const modp_rt_consts* cs, hipStream_t s);
/* key set of `count` keys (EB-byte values of any size on the device): ks[key][j][d] = key^(d 2^(256 j)) R mod N, j < EB / 32,
   d < 16 -- modp_rt_keyset_bytes(lpl, count) bytes; count times EB / 32 must fit an int */
int MODP_RT_FN(launch_keyset_build)(int lpl, const uint8_t* keys_be, int count, uint32_t* ks, const modp_rt_consts* cs, hipStream_t s);
/* out_a[x] = key_x^e1a[x] * B2[x]^e2[x] mod q, canonical, over the rows ks[x] of a key set (ks: the rows of the first key) and B2's
   16-entry table (tab2 == NULL: the power of the key alone; tab2_stride in words, e2_stride in bytes, 0 = one exponent for every
   x).  e1b != NULL (tab2 must be NULL): out_b[x] = key_x^e1b[x] as well, a second exponent set in the same launch (gridDim.y = 2) */
int MODP_RT_FN(launch_keyset_exp)(int lpl, const uint32_t* ks, const uint32_t* tab2, size_t tab2_stride, const uint8_t* e1a,
                              const uint8_t* e1b, const uint8_t* e2, size_t e2_stride, int count, uint8_t* out_a, uint8_t* out_b,
                              const modp_rt_consts* cs, hipStream_t s);
/* out[x] = key_(key_of[x])^e1[x] * B2[x]^e2[x] mod q: modp_rt_launch_keyset_exp's first exponent set with the key of every share
   named by its index in the set (ks: the rows of the set's FIRST key; key_of: `count` indices on the device) */
int MODP_RT_FN(launch_keyset_exp_idx)(int lpl, const uint32_t* ks, const uint32_t* key_of, const uint32_t* tab2, size_t tab2_stride,
                                  const uint8_t* e1, const uint8_t* e2, size_t e2_stride, int count, uint8_t* out,
                                  const modp_rt_consts* cs, hipStream_t s);
/* the same two results right to left with shared squarings (k_rt_twin_exp): bases as EB-byte values of any size, `buckets`
   a scratch of modp_rt_twin_scratch_bytes(lpl, count) bytes that holds exponent windows afterwards (the caller zeroes it) */
int MODP_RT_FN(launch_twin_exp)(int lpl, const uint8_t* bases, const uint8_t* e1, const uint8_t* e2, int count, uint32_t* buckets,
                            uint8_t* out1, uint8_t* out2, const modp_rt_consts* cs, hipStream_t s);
/* out[x] = a[x] b[x] mod q, canonical, from a R and b R (modp_rt_launch_to_mont) */
int MODP_RT_FN(launch_mul)(int lpl, const uint32_t* a_m, const uint32_t* b_m, int count, uint8_t* out, const modp_rt_consts* cs, hipStream_t s);
/* out[s] = prod of the factors f_m[first_s .. first_s + m_s) mod q, canonical, one workgroup per segment: f_m numbers in
   Montgomery form (modp_rt_launch_to_mont), segs [nsegs][2] words {first factor, m} on the device, every segment inside f_m */
int MODP_RT_FN(launch_product_segments)(int lpl, const uint32_t* f_m, const uint32_t* segs, int nsegs, uint8_t* out,
                                    const modp_rt_consts* cs, hipStream_t s);
/* X[x] = Horner in the exponent over the commitments cm_m ([t] numbers in Montgomery form) at i' = positions[x] mod (q-1) */
int MODP_RT_FN(launch_commit_eval)(int lpl, const uint32_t* cm_m, int t, const int64_t* positions, int count, uint8_t* x_be,
                               const modp_rt_consts* cs, hipStream_t s);
/* X of a run of boxes in one launch, one workgroup per tile (up to 16 consecutive shares of one box): tiles [ntiles][4] words
   {box, first share in the concatenation, live shares, 0}, boxes [boxes][2] words {first commitment in cm_all_m, t}, cm_all_m the
   commitments of all boxes in Montgomery form, positions and x_be over the concatenated shares */
int MODP_RT_FN(launch_commit_eval_tiles)(int lpl, const uint32_t* cm_all_m, const uint32_t* tiles, int ntiles, const uint32_t* boxes,
                                     const int64_t* positions, uint8_t* x_be, const modp_rt_consts* cs, hipStream_t s);
/* the seeds of the forward differences: Horner in Montgomery form at `count` positions over cm_m (gridDim.y = 0) and over the
   inverted commitments cm_inv_m (1) in one launch; x_m [2][count][L], every number < 2N */
int MODP_RT_FN(launch_commit_eval_mont)(int lpl, const uint32_t* cm_m, const uint32_t* cm_inv_m, int t, const int64_t* positions,
                                    int count, uint32_t* x_m, const modp_rt_consts* cs, hipStream_t s);
/* X in Montgomery limbs, x_m [n][L], at n consecutive positions cut into S chains (modp_rt_fd_chain) from seeds_m [2][S][t][L]:
   one workgroup per chain and direction; park: scratch of modp_rt_fd_park_bytes(lpl, t, S) bytes.  2 <= t <= MODP_RT_FD_MAX_T(lpl), n / S >= t, else hipErrorInvalidValue */
int MODP_RT_FN(launch_fd_chains)(int lpl, const uint32_t* seeds_m, int t, int n, int S, uint32_t* x_m, uint32_t* park,
                             const modp_rt_consts* cs, hipStream_t s);
/* out[x] = canonical EB bytes of x_m[x] (Montgomery limbs < 2N) */
int MODP_RT_FN(launch_from_mont)(int lpl, const uint32_t* x_m, int count, uint8_t* out_be, const modp_rt_consts* cs, hipStream_t s);
/* The scalar ring Z/(q-1) (csq: the device image of the constants of q' = (q-1)/2, odd and >= 3, at the handle's width; every
   value EB big-endian bytes of any size, every result canonical in [0, q-1)).
   out[x] = a[x] b[x] mod (q-1) */
int MODP_RT_FN(launch_modq_mul)(int lpl, const uint8_t* a_be, const uint8_t* b_be, int count, uint8_t* out_be, const modp_rt_consts* csq,
                            hipStream_t s);
/* r[x] = w[x] - alpha[x] c mod (q-1) for one shared c: cneg_be = (-c) mod q' (EB bytes on the device), c_parity = c mod 2 */
int MODP_RT_FN(launch_modq_responses)(int lpl, const uint8_t* w_be, const uint8_t* alpha_be, const uint8_t* cneg_be, int c_parity, int count,
                                  uint8_t* out_be, const modp_rt_consts* csq, hipStream_t s);
/* out[x] = P(positions[x]) mod (q-1): coef_m [t][L] limbs of (a_j mod q') R mod q', 0 <= positions < 2^63, par_even / par_odd the
   parity of P at even / odd positions */
int MODP_RT_FN(launch_modq_poly_eval)(int lpl, const uint32_t* coef_m, int t, const int64_t* positions, int count, int par_even, int par_odd,
                                  uint8_t* out_be, const modp_rt_consts* csq, hipStream_t s);
/* The Lagrange exponents of reconstruct (csq as above).  positions: the launch's position lists back to back; tiles [ntiles][4] words
   {the list's first position, m, the tile's first coefficient, live coefficients (1 .. 16)} on the device, a tile inside one list.
   Workgroup w owns the slots 16 w .. 16 w + 15 of the work arrays: num_m, den_m [16 ntiles][L] limbs below 2 q' (the products of
   the x_j and of the |x_j - x_i|, both times the same power of two), den_be the denominators as canonical EB bytes */
int MODP_RT_FN(launch_lagrange_terms)(int lpl, const int64_t* positions, const uint32_t* tiles, int ntiles, uint32_t* num_m, uint32_t* den_m,
                                  uint8_t* den_be, const modp_rt_consts* csq, hipStream_t s);
/* exps[c] (EB bytes) and flags[c] of every live coefficient c of the tiles from those work arrays and dinv_be = den^(q'-2) (canonical
   EB bytes per slot): flags[c] = 1 iff den dinv = 1 mod q'; exps[c] = num dinv mod q', or 2 q' minus that when neg[c] and it is not 0 */
int MODP_RT_FN(launch_lagrange_finish)(int lpl, const uint32_t* tiles, int ntiles, const uint32_t* num_m, const uint32_t* den_m,
                                   const uint8_t* dinv_be, const uint8_t* neg, uint8_t* exps, uint8_t* flags, const modp_rt_consts* csq,
                                   hipStream_t s);
