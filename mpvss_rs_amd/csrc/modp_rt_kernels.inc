// Kernel templates and launchers of a run-time MODP group: ModpGroup::init(length) of the reference
// (src/groups/modp.rs:72-84) -- any odd modulus q of at most 4096 bits, chosen when the program runs.  Included by the
// three translation units that instantiate them: modp_rt_kernels.hip (5, 9 and 18 limbs per lane, groups of 256-byte
// elements), modp_rt_kernels_wide.hip (27 limbs per lane, groups of 384-byte elements) and modp_rt_kernels_4096.hip (36 limbs
// per lane, groups of 512-byte elements), each of which defines
// RT_FN, RT_DISPATCH, RT_DISPATCH_FN and RT_ELSEWHERE first.  One more unit, modp_rt_fd_kernels.hip (RT_FD_ONLY), holds nothing but
// k_rt_fd_chain at 5, 9 and 18 limbs per lane, which modp_rt_kernels.hip reaches through RT_FD_ELSEWHERE.
//
//   ModpGroup::exp / ::mul                       (src/groups/modp.rs:122-132)      k_rt_dual_exp, k_rt_mul
//   DLEQ verifier commitments a = g1^r h1^c      (src/dleq.rs:66-84)               k_rt_dual_exp (two tables)
//   X_i = prod_j C_j^(i^j mod (q-1))             (src/participant.rs:423-434)      k_rt_commit_eval
//   X_i of the small boxes of a whole round, one launch   (one call per box in the reference)  k_rt_commit_eval_tiles, k_rt_spread_challenge
//   G^s = prod_i S_i^lambda_i of the secrets of a whole round, one launch (src/participant.rs:503-505)   k_rt_product_segments
//   P(i), r_i = w_i - P(i) c, w_i / x_i in Z/(q-1) (src/polynomial.rs:50-58, src/dleq.rs:42-50, modp.rs:180-182)
//                                                                                  k_rt_modq_poly_eval, _responses, _mul
//   y_i^r_i Y_i^c, y_i^P(i), y_i^w_i for long-lived keys    (src/participant.rs:436-447, :219)  k_rt_keyset_bases, _rows, _exp, _exp_idx
//
// Layout and program shape are those of the group-14 kernels (modp_kernels.hip): one number per DPP quad, 16 numbers
// per one-wave workgroup, the second operand of every product staged in LDS, 16-entry window tables in HBM.  The
// product is bn::mont_mul at the widths of bn_quad_rt.h, n0inv a run-time value.
//
// Cost follows the operands: the exponent loops run over the wave's largest exponent (4-bit windows), Horner's squarings
// over the wave's largest reduced position.  Inputs are big-endian values of Width::EB bytes (256; 384 at 27 limbs per lane,
// 512 at 36) of any size: they enter a width by one long product (bnrt::Width::IN_ROWS rows), which reduces them mod q on
// the way into Montgomery form.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bn_quad_rt.h"
#include "modp_rt_kernels.h"

using namespace bnrt;

#define RT_NUMS 16   // numbers per workgroup (one wave)

namespace {

// occupancy of each width: the 18-limb product wants 3 waves per SIMD like the group-14 kernels (135 VGPRs); the
// narrower ones fit more, the 27-limb one (54 accumulator registers) two, the 36-limb one (72) one
template <int LPL> struct Occ { static constexpr int waves = 3; };
template <> struct Occ<9> { static constexpr int waves = 4; };
template <> struct Occ<5> { static constexpr int waves = 6; };
template <> struct Occ<27> { static constexpr int waves = 2; };
template <> struct Occ<36> { static constexpr int waves = 1; };

// a = in R mod N (< 2N) for any EB-byte input: the input's 29-bit limbs go to the LDS slot (IN_ROWS of them), and one
// long product with kin = 2^(29 (IN_ROWS + L)) mod N gives in kin 2^(-29 IN_ROWS) = in R, below N + kin in / 2^(29 IN_ROWS) < 2N.
template <int LPL>
__device__ __forceinline__ void to_mont_in(u32 (&a)[LPL], u32* slot, const uint8_t* __restrict__ in_be, const modp_rt_consts* __restrict__ cs,
                                           const u32 (&n)[LPL], u32 n0inv, const Lane& ln) {
  constexpr int IN_ROWS = Width<LPL>::IN_ROWS;
#pragma unroll
  for (int j = (int)0; j < IN_ROWS; j += 4) {
    const int jj = j + (int)ln.q;
    if (jj < IN_ROWS) slot[jj] = limbs::be_limb<Width<LPL>::EB>(in_be, jj);
  }
  u32 k[LPL];
  load_lane_limbs<LPL>(k, cs->kin, ln);
  __builtin_amdgcn_wave_barrier();
  mont_mul<N0INV_RUNTIME, false, IN_ROWS / LPL>(a, k, slot, n, ln, n0inv);
  __builtin_amdgcn_wave_barrier();
}

// plain almost-normalised value < 2N -> canonical residue as EB big-endian bytes (the slot is scratch)
template <int LPL>
__device__ __forceinline__ void store_canonical(uint8_t* __restrict__ out, const u32 (&a)[LPL], u32* slot,
                                                const modp_rt_consts* __restrict__ cs, const Lane& ln, bool write) {
  constexpr int L = Width<LPL>::L, EB = Width<LPL>::EB, WPL = EB / 16;
  slot_store<LPL>(slot, a, ln);
  __builtin_amdgcn_wave_barrier();
  if (ln.q == 0) limbs::slot_canonicalize<L>(slot, cs->n);
  __builtin_amdgcn_wave_barrier();
  if (write) {
    // lane q emits little-endian 32-bit words WPL q .. WPL q + WPL - 1 (byte-swapped, mirrored position), WPL = 16 words of
    // a 256-byte value, 24 of a 384-byte one; limbs >= L are zero
    u32* out32 = reinterpret_cast<u32*>(out);
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      const int wd = (int)ln.q * WPL + i;
      out32[4 * WPL - 1 - wd] = __builtin_bswap32(limbs::slot_word32<L, EB>(slot, wd));
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// bit length of an EB-byte big-endian number, the maximum over the whole wave (every quad: lane q scans its quarter, bytes
// 64q .. 64q+63 of 256, 96q .. 96q+95 of 384)
template <int EB>
__device__ __forceinline__ int wave_max_bits(const uint8_t* __restrict__ be, const Lane& ln) {
  constexpr int QW = EB / 16;                              // 32-bit words of a quarter
  const uint4* p = reinterpret_cast<const uint4*>(be + (EB / 4) * ln.q);
  int bl = 0;
#pragma unroll
  for (int i = QW / 4 - 1; i >= 0; --i) {
    const uint4 v = p[i];
    const u32 w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 3; k >= 0; --k) {
      const u32 word = __builtin_bswap32(w4[k]);       // big-endian word 4 i + k of this lane's quarter
      if (word != 0) bl = (QW - (4 * i + k)) * 32 - __builtin_clz(word);
    }
  }
  if (bl > 0) bl += (3 - (int)ln.q) * (2 * EB);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int other = __shfl_xor(bl, off);
    bl = other > bl ? other : bl;
  }
  return __builtin_amdgcn_readfirstlane(bl);
}

template <int EB>
__device__ __forceinline__ u32 nibble(const uint8_t* __restrict__ e, int w) {
  const u32 byte = e[EB - 1 - (w >> 1)];
  return (w & 1) ? (byte >> 4) : (byte & 15u);
}

}  // namespace

#define RT_KERNEL(LPL) __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(Occ<LPL>::waves, Occ<LPL>::waves)))
// Horner's kernel holds two slots per number: at 5 limbs per lane its LDS (10 KB per wave) admits 4 waves per SIMD
#define RT_KERNEL_LDS2(LPL) __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(Occ<LPL>::waves < 4 ? Occ<LPL>::waves : 4, Occ<LPL>::waves < 4 ? Occ<LPL>::waves : 4)))

// ---------------------------------------------------------------------------------------
// out_m[x] = in[x] R mod N (commitments into Montgomery form)
// ---------------------------------------------------------------------------------------
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_to_mont(const uint8_t* __restrict__ in_be, int count, u32* __restrict__ out_m,
                                            const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  u32 n[LPL], a[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  to_mont_in<LPL>(a, slot, in_be + (size_t)x * Width<LPL>::EB, cs, n, n0inv, ln);
  if (live) store_lane_limbs<LPL>(out_m + (size_t)x * L, a, ln);
}

// ---------------------------------------------------------------------------------------
// 16-entry window table of each base: tab[x][d] = base^d R mod N
// ---------------------------------------------------------------------------------------
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_table(const uint8_t* __restrict__ base_be, size_t base_stride, int count, u32* __restrict__ tab,
                                          const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  u32 n[LPL], b[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  to_mont_in<LPL>(b, slot, base_be + (size_t)x * base_stride, cs, n, n0inv, ln);
  u32* my = tab + (size_t)x * 16 * L;
  load_lane_limbs<LPL>(acc, cs->one_m, ln);
  if (live) store_lane_limbs<LPL>(my, acc, ln);
  if (live) store_lane_limbs<LPL>(my + L, b, ln);
  slot_store<LPL>(slot, b, ln);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int k = 0; k < LPL; ++k) acc[k] = b[k];
  for (int e = 2; e < 16; ++e) {
    mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
    if (live) store_lane_limbs<LPL>(my + (size_t)e * L, acc, ln);
  }
}

// ---------------------------------------------------------------------------------------
// out[x] = B1^e1 * B2^e2 mod q (B2 absent when tab2 is null), fixed 4-bit windows from the wave's highest one,
// squarings shared.  One Montgomery-product site: every step only chooses its LDS operand (own copy = square, a table
// entry, plain 1 at the end).
// ---------------------------------------------------------------------------------------
template <int LPL>
__device__ __forceinline__ void rt_dual_exp_body(u32* lds, const u32* __restrict__ tab1, size_t tab1_stride, const u32* __restrict__ tab2,
                                                 size_t tab2_stride, const uint8_t* __restrict__ e1_be, size_t e1_stride,
                                                 const uint8_t* __restrict__ e2_be, size_t e2_stride, int count,
                                                 uint8_t* __restrict__ out_be, const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT;
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  const bool has2 = tab2 != nullptr;
  const u32* t1 = tab1 + (size_t)x * tab1_stride;
  const u32* t2 = has2 ? tab2 + (size_t)x * tab2_stride : t1;
  const uint8_t* e1 = e1_be + (size_t)x * e1_stride;
  const uint8_t* e2 = has2 ? e2_be + (size_t)x * e2_stride : e1;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  int nb = wave_max_bits<Width<LPL>::EB>(e1, ln);
  if (has2) {
    const int nb2 = wave_max_bits<Width<LPL>::EB>(e2, ln);
    nb = nb2 > nb ? nb2 : nb;
  }
  const int nw = (nb + 3) >> 2;
  // steps: 0..3 square, 4 times tab1[d1], 5 times tab2[d2], 6 next window, 7 final (times plain 1)
  int w = nw - 1, s;
  if (nw == 0) {
    load_lane_limbs<LPL>(acc, cs->one_m, ln);
    s = 7;
  } else {
    load_lane_limbs<LPL>(acc, t1 + (size_t)nibble<Width<LPL>::EB>(e1, w) * L, ln);
    s = has2 ? 5 : 6;
  }
  while (true) {
    if (s == 6) {
      if (w == 0) {
        s = 7;
      } else {
        --w;
        s = 0;
      }
    }
    if (s == 7) {
      slot_fill_from_global<LPL>(slot, cs->one, ln);
    } else if (s < 4) {
      slot_store<LPL>(slot, acc, ln);
    } else {
      const u32 d = nibble<Width<LPL>::EB>(s == 4 ? e1 : e2, w);
      slot_fill_from_global<LPL>(slot, (s == 4 ? t1 : t2) + (size_t)d * L, ln);
    }
    __builtin_amdgcn_wave_barrier();
    if (s < 4) mont_mul<N0INV_RUNTIME, true>(acc, acc, slot, n, ln, n0inv);
    else mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
    __builtin_amdgcn_wave_barrier();
    if (s == 7) break;
    ++s;
    if (s == 5 && !has2) s = 6;
  }
  store_canonical<LPL>(out_be + (size_t)x * Width<LPL>::EB, acc, slot, cs, ln, live);
}

template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_dual_exp(const u32* __restrict__ tab1, size_t tab1_stride, const u32* __restrict__ tab2,
                                             size_t tab2_stride, const uint8_t* __restrict__ e1_be, size_t e1_stride,
                                             const uint8_t* __restrict__ e2_be, size_t e2_stride, int count,
                                             uint8_t* __restrict__ out_be, const modp_rt_consts* __restrict__ cs) {
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * Width<LPL>::SLOT];
  rt_dual_exp_body<LPL>(lds, tab1, tab1_stride, tab2, tab2_stride, e1_be, e1_stride, e2_be, e2_stride, count, out_be, cs);
}

// ---------------------------------------------------------------------------------------
// Fixed-base comb of ONE base shared by every share: comb[k][d] = base^(d 16^k) R mod N, k = 0..ROWS-1, d = 0..15, entry 0 =
// R mod N.  Always ROWS = Width::COMB_ROWS rows (512, or 768 at the wide width): any exponent of EB bytes stays exact.  The
// counterpart of group 14's k_modp_comb_bases /
// k_modp_comb_rows at a run-time width.
//   k_rt_comb_bases (one workgroup, its first quad writes): the base enters through to_mont_in like a table base (a base
//                   >= q is reduced, one that is 0 mod q gives rows of zeros); comb[k][1] = comb[k-1][1]^16, a row base
//                   every four squarings, and entry 0 of every row
//   k_rt_comb_rows  (one number per row k): comb[k][d] = comb[k][d-1] comb[k][1] for d = 2..15
// ---------------------------------------------------------------------------------------
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_comb_bases(const uint8_t* __restrict__ base_be, u32* __restrict__ comb,
                                               const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT, ROWS = Width<LPL>::COMB_ROWS;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const bool writer = (blockIdx.x == 0) && (threadIdx.x < 4);
  const u32 n0inv = cs->n0inv;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  load_lane_limbs<LPL>(acc, cs->one_m, ln);
  if (writer) {
#pragma nounroll
    for (int k = 0; k < ROWS; ++k) store_lane_limbs<LPL>(comb + (size_t)k * 16 * L, acc, ln);
  }
  to_mont_in<LPL>(acc, slot, base_be, cs, n, n0inv, ln);
#pragma nounroll
  for (int op = 0; op <= (ROWS - 1) * 4; ++op) {
    if (writer && (op & 3) == 0) store_lane_limbs<LPL>(comb + ((size_t)(op >> 2) * 16 + 1) * L, acc, ln);
    if (op == (ROWS - 1) * 4) break;
    slot_store<LPL>(slot, acc, ln);
    __builtin_amdgcn_wave_barrier();
    mont_mul<N0INV_RUNTIME, true>(acc, acc, slot, n, ln, n0inv);
    __builtin_amdgcn_wave_barrier();
  }
}

template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_comb_rows(u32* __restrict__ comb, const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT, ROWS = Width<LPL>::COMB_ROWS;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < ROWS;
  const int k = live ? xi : ROWS - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  u32* row = comb + (size_t)k * 16 * L;
  load_lane_limbs<LPL>(acc, row + L, ln);
  slot_store<LPL>(slot, acc, ln);
  __builtin_amdgcn_wave_barrier();
#pragma nounroll
  for (int d = 2; d < 16; ++d) {
    mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
    if (live) store_lane_limbs<LPL>(row + (size_t)d * L, acc, ln);
  }
}

// ---------------------------------------------------------------------------------------
// out[x] = base^e1[x] (* B2[x]^e2[x] when tab2 is not null) over the comb of the shared base: no squaring for e1 at all.
//   phase A (tab2 only): B2^e2 left to right, 4-bit windows over B2's 16-entry table from the wave's highest set bit of e2
//                        (e2_stride 0: one exponent for every x)
//   phase B            : acc *= comb[k][nibble(e1, k)] for k = 0 .. nw1-1, nw1 from the wave's longest e1; a window whose digit
//                        is 0 in all 16 numbers of the wave is skipped, otherwise a lane with digit 0 multiplies by entry 0
//   then times plain 1.  Without tab2 and with every e1 of the wave 0 the result is 1.
// One Montgomery-product site as in rt_dual_exp_body: every step only chooses its LDS operand.  The comb index is an exponent
// digit, so the gather address follows the exponent, as the nibble-indexed table reads of k_rt_dual_exp do.
// Full-width e1 at 2048 bits: 512 comb products + 1 exit = 513 Montgomery operations (tests/test_modp_rt_comb_model.py); at
// 3072 bits, 768 + 1 = 769 (tests/test_modp_rt_wide_model.py).
// ---------------------------------------------------------------------------------------
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_comb_exp(const u32* __restrict__ comb, const u32* __restrict__ tab2, size_t tab2_stride,
                                             const uint8_t* __restrict__ e1_be, const uint8_t* __restrict__ e2_be, size_t e2_stride,
                                             int count, uint8_t* __restrict__ out_be, const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  const bool has2 = tab2 != nullptr;
  const uint8_t* e1 = e1_be + (size_t)x * Width<LPL>::EB;
  const uint8_t* e2 = has2 ? e2_be + (size_t)x * e2_stride : e1;
  const u32* t2 = has2 ? tab2 + (size_t)x * tab2_stride : comb;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  const int nw1 = (wave_max_bits<Width<LPL>::EB>(e1, ln) + 3) >> 2;                 // <= Width::COMB_ROWS
  const int nw2 = has2 ? (wave_max_bits<Width<LPL>::EB>(e2, ln) + 3) >> 2 : 0;
  // steps: 0..3 square, 4 times tab2[d2], 5 next window of e2, 6 times comb[k][d1], 7 final (times plain 1)
  int w = nw2 - 1, k = 0, s;
  if (nw2 == 0) {
    load_lane_limbs<LPL>(acc, cs->one_m, ln);
    s = 6;
  } else {
    load_lane_limbs<LPL>(acc, t2 + (size_t)nibble<Width<LPL>::EB>(e2, w) * L, ln);
    s = 5;
  }
  while (true) {
    if (s == 5) {
      if (w == 0) {
        s = 6;
      } else {
        --w;
        s = 0;
      }
    }
    if (s == 6) {
      while (k < nw1 && __builtin_amdgcn_ballot_w64(nibble<Width<LPL>::EB>(e1, k) != 0) == 0) ++k;
      if (k == nw1) s = 7;
    }
    if (s == 7) {
      slot_fill_from_global<LPL>(slot, cs->one, ln);
    } else if (s < 4) {
      slot_store<LPL>(slot, acc, ln);
    } else if (s == 4) {
      slot_fill_from_global<LPL>(slot, t2 + (size_t)nibble<Width<LPL>::EB>(e2, w) * L, ln);
    } else {
      slot_fill_from_global<LPL>(slot, comb + ((size_t)k * 16 + nibble<Width<LPL>::EB>(e1, k)) * L, ln);
      ++k;
    }
    __builtin_amdgcn_wave_barrier();
    if (s < 4) mont_mul<N0INV_RUNTIME, true>(acc, acc, slot, n, ln, n0inv);
    else mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
    __builtin_amdgcn_wave_barrier();
    if (s == 7) break;
    if (s < 5) ++s;
  }
  store_canonical<LPL>(out_be + (size_t)x * Width<LPL>::EB, acc, slot, cs, ln, live);
}

// ---------------------------------------------------------------------------------------
// Two powers of each base in ONE launch: out1[x] = B[x]^e1[x] (blockIdx.y = 0), out2[x] = B[x]^e2[x] (blockIdx.y = 1), both
// left to right over the base's one 16-entry table.  The form for a batch that does not fill the chip: twice the
// workgroups of one k_rt_dual_exp launch, each with the short chain of a single exponentiation.
// ---------------------------------------------------------------------------------------
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_exp_sets(const u32* __restrict__ tab, size_t tab_stride, const uint8_t* __restrict__ e1_be,
                                             const uint8_t* __restrict__ e2_be, int count, uint8_t* __restrict__ out1_be,
                                             uint8_t* __restrict__ out2_be, const modp_rt_consts* __restrict__ cs) {
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * Width<LPL>::SLOT];
  const bool second = blockIdx.y != 0;
  rt_dual_exp_body<LPL>(lds, tab, tab_stride, nullptr, 0, second ? e2_be : e1_be, Width<LPL>::EB, nullptr, 0, count, second ? out2_be : out1_be, cs);
}

// ---------------------------------------------------------------------------------------
// Key sets: per-key row tables for full-width powers of long-lived public keys (the counterpart of group 14's key sets at a
// run-time width).  ks[key][j][d] = y^(d 2^(256 j)) R mod N, j < J = Width::KS_ROWS = EB / 32 (8 rows, 12 at the wide width),
// d < 16, entry 0 = R mod N: always J rows, so any EB-byte exponent stays exact, as the comb's 2 EB rows do.
//   k_rt_keyset_bases (one key per quad): the key enters through to_mont_in like a table base (a key >= q is reduced, one that
//                     is 0 mod q gives rows of zeros beside entry 0); one chain of 256 (J - 1) squarings, entry 1 of row j
//                     stored every 256 of them, and entry 0 of every row
//   k_rt_keyset_rows  (one number per (key, row)): d = 2..15, as k_rt_comb_rows fills the comb's rows
// 1 + 256 (J - 1) + 14 J operations per key: 1 905 at 256 bytes, 2 985 at 384 (tests/test_modp_rt_keyset_model.py).
// ---------------------------------------------------------------------------------------
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_keyset_bases(const uint8_t* __restrict__ keys_be, int count, u32* __restrict__ ks,
                                                 const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT, J = Width<LPL>::KS_ROWS;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  u32* my = ks + (size_t)x * J * 16 * L;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  load_lane_limbs<LPL>(acc, cs->one_m, ln);
  if (live) {
#pragma nounroll
    for (int j = 0; j < J; ++j) store_lane_limbs<LPL>(my + (size_t)j * 16 * L, acc, ln);
  }
  to_mont_in<LPL>(acc, slot, keys_be + (size_t)x * Width<LPL>::EB, cs, n, n0inv, ln);
#pragma nounroll
  for (int op = 0; op <= (J - 1) * 256; ++op) {
    if (live && (op & 255) == 0) store_lane_limbs<LPL>(my + ((size_t)(op >> 8) * 16 + 1) * L, acc, ln);
    if (op == (J - 1) * 256) break;
    slot_store<LPL>(slot, acc, ln);
    __builtin_amdgcn_wave_barrier();
    mont_mul<N0INV_RUNTIME, true>(acc, acc, slot, n, ln, n0inv);
    __builtin_amdgcn_wave_barrier();
  }
}

// k_rt_comb_rows over a run-time number of rows.  A body of its own: k_rt_comb_rows with the count made an argument allocates
// other registers at 18 limbs per lane (114 instead of 118), and existing instances keep their figures.
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_keyset_rows(u32* __restrict__ ks, int nrows, const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < nrows;
  const int k = live ? xi : nrows - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  u32* row = ks + (size_t)k * 16 * L;
  load_lane_limbs<LPL>(acc, row + L, ln);
  slot_store<LPL>(slot, acc, ln);
  __builtin_amdgcn_wave_barrier();
#pragma nounroll
  for (int d = 2; d < 16; ++d) {
    mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
    if (live) store_lane_limbs<LPL>(row + (size_t)d * L, acc, ln);
  }
}

// ---------------------------------------------------------------------------------------
// out[x] = y_x^e1[x] (* B2[x]^e2[x] when tab2 is not null) over the rows ks[x] of a key set: Straus over the key's J rows and
// B2's 16-entry table, 4-bit windows, 63 x 4 squarings for a full-width e1 instead of 2 044.  blockIdx.y selects an exponent set:
// 0 is (e1a, out_a), 1 is (e1b, out_b) -- the dealer's two powers of one key in one launch (gridDim.y = 2, no tab2), as
// k_rt_exp_sets does.
//   W = max(ceil(min(bits(e1), 256) / 4), ceil(bits(e2) / 4)) over the wave.  For w = W-1 .. 0: four squarings (none while the
//   accumulator is still one); for w < 64 one product per row j by ks[j][nibble(e1, 64 j + w)], rows above the wave's longest e1
//   left out and a row whose digit is 0 in all 16 numbers of the wave skipped (otherwise a lane with digit 0 multiplies by entry
//   0); then the product by tab2[nibble(e2, w)] while w is below the wave's longest e2.  Windows of e2 above 64 run before the
//   rows join, so any EB-byte e2 stays exact.  Then times plain 1.
// One Montgomery-product site as in rt_dual_exp_body: every step only chooses its LDS operand.  The row index is an exponent
// digit, so the gather address follows the exponent, as the comb's does; the table is per share, so no gather is shared.
// Full-width e1 with a 256-bit e2 at 2048 bits: 252 squarings + 512 row products + 64 products by B2 + 1 exit = 829 (844 with
// B2's table; tests/test_modp_rt_keyset_model.py).
// ---------------------------------------------------------------------------------------
//   rows, x, live : the rows of this quad's key, the share it works on and whether it stores its result -- the entry decides
//                   which key a share takes: the x-th of the rows it was given (k_rt_keyset_exp) or the one an index names
//                   (k_rt_keyset_exp_idx)
template <int LPL>
__device__ __forceinline__ void rt_keyset_exp_body(u32* lds, const u32* __restrict__ rows, int x, bool live, const u32* __restrict__ tab2,
                                                   size_t tab2_stride, const uint8_t* __restrict__ e1a_be,
                                                   const uint8_t* __restrict__ e1b_be, const uint8_t* __restrict__ e2_be,
                                                   size_t e2_stride, uint8_t* __restrict__ out_a, uint8_t* __restrict__ out_b,
                                                   const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT, EB = Width<LPL>::EB, J = Width<LPL>::KS_ROWS;
  const Lane ln = make_lane();
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  const bool second = blockIdx.y != 0;
  const bool has2 = tab2 != nullptr;
  const uint8_t* e1 = (second ? e1b_be : e1a_be) + (size_t)x * EB;
  const uint8_t* e2 = has2 ? e2_be + (size_t)x * e2_stride : e1;
  const u32* t2 = has2 ? tab2 + (size_t)x * tab2_stride : rows;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  const int nb1 = wave_max_bits<EB>(e1, ln);
  const int jl = (nb1 + 255) >> 8;                                     // rows the wave's longest e1 reaches, <= J
  const int nw2 = has2 ? (wave_max_bits<EB>(e2, ln) + 3) >> 2 : 0;
  const int nw1 = ((nb1 < 256 ? nb1 : 256) + 3) >> 2;
  const int nw = nw1 > nw2 ? nw1 : nw2;
  // steps: 0..3 square, 4 + j times ks[j][d1], 4 + J times tab2[d2], 5 + J next window, 6 + J final (times plain 1)
  constexpr int S_TAB2 = 4 + J, S_NEXT = 5 + J, S_FINAL = 6 + J;
  int w = nw - 1, s = nw == 0 ? S_FINAL : 4;
  bool one = true;                                                     // the accumulator is still R mod N (wave-uniform)
  load_lane_limbs<LPL>(acc, cs->one_m, ln);
  while (true) {
    while (s != S_FINAL) {                                             // the next step that has work
      if (s == S_NEXT) {
        if (w == 0) {
          s = S_FINAL;
        } else {
          --w;
          s = one ? 4 : 0;
        }
      } else if (s < 4) {
        break;
      } else if (s < S_TAB2) {
        const int j = s - 4;
        if (w < 64 && j < jl && __builtin_amdgcn_ballot_w64(nibble<EB>(e1, 64 * j + w) != 0) != 0) break;
        s = (w < 64 && j + 1 < jl) ? s + 1 : S_TAB2;
      } else {
        if (w < nw2) break;
        s = S_NEXT;
      }
    }
    if (s == S_FINAL) {
      slot_fill_from_global<LPL>(slot, cs->one, ln);
    } else if (s < 4) {
      slot_store<LPL>(slot, acc, ln);
    } else if (s < S_TAB2) {
      const int j = s - 4;
      slot_fill_from_global<LPL>(slot, rows + ((size_t)j * 16 + nibble<EB>(e1, 64 * j + w)) * L, ln);
    } else {
      slot_fill_from_global<LPL>(slot, t2 + (size_t)nibble<EB>(e2, w) * L, ln);
    }
    __builtin_amdgcn_wave_barrier();
    if (s < 4) mont_mul<N0INV_RUNTIME, true>(acc, acc, slot, n, ln, n0inv);
    else mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
    __builtin_amdgcn_wave_barrier();
    if (s == S_FINAL) break;
    if (s >= 4) one = false;
    ++s;
  }
  store_canonical<LPL>((second ? out_b : out_a) + (size_t)x * EB, acc, slot, cs, ln, live);
}

template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_keyset_exp(const u32* __restrict__ ks, const u32* __restrict__ tab2, size_t tab2_stride,
                                               const uint8_t* __restrict__ e1a_be, const uint8_t* __restrict__ e1b_be,
                                               const uint8_t* __restrict__ e2_be, size_t e2_stride, int count,
                                               uint8_t* __restrict__ out_a, uint8_t* __restrict__ out_b,
                                               const modp_rt_consts* __restrict__ cs) {
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * Width<LPL>::SLOT];
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  rt_keyset_exp_body<LPL>(lds, ks + (size_t)x * Width<LPL>::KS_ROWS * 16 * Width<LPL>::L, x, live, tab2, tab2_stride, e1a_be, e1b_be, e2_be,
                          e2_stride, out_a, out_b, cs);
}

// The same over keys named one by one: share x takes the rows of key key_of[x] of the set (ks: the rows of the set's first key).
// The shares of a run of boxes do not walk the set's rows consecutively (capi_modp_rt.inc, "Many boxes in one call").
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_keyset_exp_idx(const u32* __restrict__ ks, const u32* __restrict__ key_of, const u32* __restrict__ tab2,
                                                   size_t tab2_stride, const uint8_t* __restrict__ e1_be,
                                                   const uint8_t* __restrict__ e2_be, size_t e2_stride, int count,
                                                   uint8_t* __restrict__ out, const modp_rt_consts* __restrict__ cs) {
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * Width<LPL>::SLOT];
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  rt_keyset_exp_body<LPL>(lds, ks + (size_t)key_of[x] * Width<LPL>::KS_ROWS * 16 * Width<LPL>::L, x, live, tab2, tab2_stride, e1_be, nullptr,
                          e2_be, e2_stride, out, nullptr, cs);
}

// ---------------------------------------------------------------------------------------
// K_e[d] = prod over the windows k of exponent e with digit d of B^(16^k), for both exponents of each base with the squarings
// shared: right to left over fixed 4-bit windows.  The running power P_k = B^(16^k) is computed once and multiplied into
// bucket K_e[d] of each exponent whose k-th digit is d != 0; k_rt_twin_combine then forms
//   B^e = prod_d K_e[d]^d = prod_{j=1..15} (K_e[15] K_e[14] .. K_e[j]).
// The counterpart of group 14's k_modp_twin_exp_buckets / k_modp_bucket_combine at a run-time width.  A quad only ever
// touches its own buckets, and every lane reads back exactly the words it wrote (load_lane_limbs / store_lane_limbs).
//   buckets : HBM scratch, [16 gridDim.x][2][15][L] words (dead quads of the last workgroup have buckets of their own);
//             bucket contents tell exponent windows: the caller zeroes the scratch afterwards.
// Per window: one LDS copy of P_k serves both bucket products AND the first of the four squarings, and P_k comes back from
// it afterwards, so the kernel holds one number in registers like k_rt_dual_exp.  A bucket product is skipped when the
// digit is 0 in all 16 numbers of the wave; the window loop runs to the wave's highest set bit over both exponents.
// Worst case at 2048 bits: 1 entry + 2044 squarings + 1024 bucket products + 2 (28 combine + 1 exit) = 3127 Montgomery
// operations for both results (tests/test_modp_rt_twin_model.py); at 3072 bits 1 + 3068 + 1536 + 56 + 2 = 4663
// (tests/test_modp_rt_wide_model.py).
// ---------------------------------------------------------------------------------------
#define RT_TWIN_BUCKETS 15
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_twin_exp(const uint8_t* __restrict__ base_be, const uint8_t* __restrict__ e1_be,
                                             const uint8_t* __restrict__ e2_be, int count, u32* __restrict__ buckets,
                                             const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  const uint8_t* e1 = e1_be + (size_t)x * Width<LPL>::EB;
  const uint8_t* e2 = e2_be + (size_t)x * Width<LPL>::EB;
  u32* mine = buckets + (size_t)xi * 2 * RT_TWIN_BUCKETS * L;        // xi, not x: a dead quad works on scratch of its own
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  load_lane_limbs<LPL>(acc, cs->one_m, ln);
#pragma nounroll
  for (int b = 0; b < 2 * RT_TWIN_BUCKETS; ++b) store_lane_limbs<LPL>(mine + (size_t)b * L, acc, ln);
  to_mont_in<LPL>(acc, slot, base_be + (size_t)x * Width<LPL>::EB, cs, n, n0inv, ln);
  int nb = wave_max_bits<Width<LPL>::EB>(e1, ln);
  {
    const int nb2 = wave_max_bits<Width<LPL>::EB>(e2, ln);
    nb = nb2 > nb ? nb2 : nb;
  }
  const int nw = (nb + 3) >> 2;
  for (int w = 0; w < nw; ++w) {
    slot_store<LPL>(slot, acc, ln);
    __builtin_amdgcn_wave_barrier();
#pragma nounroll
    for (int e = 0; e < 2; ++e) {
      const u32 d = nibble<Width<LPL>::EB>(e ? e2 : e1, w);
      if (__builtin_amdgcn_ballot_w64(d != 0) == 0) continue;
      u32* bk = mine + (size_t)(e * RT_TWIN_BUCKETS + (d ? d - 1 : 0)) * L;
      load_lane_limbs<LPL>(acc, bk, ln);
      mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
      if (d != 0) store_lane_limbs<LPL>(bk, acc, ln);
    }
    if (w + 1 == nw) break;
    slot_load<LPL>(acc, slot, ln);               // P_k back from its LDS copy: the window phase holds one number in registers
#pragma nounroll
    for (int sq = 0; sq < 4; ++sq) {
      if (sq) {
        __builtin_amdgcn_wave_barrier();
        slot_store<LPL>(slot, acc, ln);
        __builtin_amdgcn_wave_barrier();
      }
      mont_mul<N0INV_RUNTIME, true>(acc, acc, slot, n, ln, n0inv);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// Combine step of k_rt_twin_exp, blockIdx.y = exponent: out[x] = prod_d K[d]^d by the running-product rule.  One number in
// registers: acc = running product S = K[15] .. K[j]; the product T of the running products lives in K[15]'s own words
// (T starts as K[15]).  A pair of steps for each j = 14 .. 1: S *= K[j]; T *= S with S parked in the LDS slot meanwhile.
// Last step: T times plain 1.  28 + 1 products.
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_twin_combine(u32* __restrict__ buckets, int count, uint8_t* __restrict__ out1_be,
                                                 uint8_t* __restrict__ out2_be, const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  u32* my = buckets + ((size_t)xi * 2 + blockIdx.y) * RT_TWIN_BUCKETS * L;
  u32* tprod = my + (size_t)(RT_TWIN_BUCKETS - 1) * L;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  load_lane_limbs<LPL>(acc, tprod, ln);
  constexpr int LAST = 2 * (RT_TWIN_BUCKETS - 1);
#pragma nounroll
  for (int step = 0; step <= LAST; ++step) {
    __builtin_amdgcn_wave_barrier();
    if (step == LAST) {
      load_lane_limbs<LPL>(acc, tprod, ln);
      slot_fill_from_global<LPL>(slot, cs->one, ln);
    } else if (!(step & 1)) {
      slot_fill_from_global<LPL>(slot, my + (size_t)(RT_TWIN_BUCKETS - 2 - (step >> 1)) * L, ln);
    } else {
      slot_store<LPL>(slot, acc, ln);
      load_lane_limbs<LPL>(acc, tprod, ln);
    }
    __builtin_amdgcn_wave_barrier();
    mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
    if (step & 1) {
      store_lane_limbs<LPL>(tprod, acc, ln);
      __builtin_amdgcn_wave_barrier();
      slot_load<LPL>(acc, slot, ln);
    }
  }
  __builtin_amdgcn_wave_barrier();
  store_canonical<LPL>((blockIdx.y ? out2_be : out1_be) + (size_t)x * Width<LPL>::EB, acc, slot, cs, ln, live);
}

// ---------------------------------------------------------------------------------------
// out[x] = a[x] b[x] mod q from a R and b R (k_rt_to_mont): a b R, times plain 1
// ---------------------------------------------------------------------------------------
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_mul(const u32* __restrict__ a_m, const u32* __restrict__ b_m, int count,
                                        uint8_t* __restrict__ out_be, const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  load_lane_limbs<LPL>(acc, a_m + (size_t)x * L, ln);
#pragma nounroll
  for (int step = 0; step < 2; ++step) {
    slot_fill_from_global<LPL>(slot, step == 0 ? b_m + (size_t)x * L : cs->one, ln);
    __builtin_amdgcn_wave_barrier();
    mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
    __builtin_amdgcn_wave_barrier();
  }
  store_canonical<LPL>(out_be + (size_t)x * Width<LPL>::EB, acc, slot, cs, ln, live);
}

// ---------------------------------------------------------------------------------------
// out[s] = prod of the factors first_s .. first_s + m_s - 1 mod q, one segment of a dense array of factors per workgroup: the
// secrets of a whole round in one launch (capi_modp_rt.inc, "Many secrets in one call"), where one secret alone takes
// ceil(log2 m) rounds of k_rt_to_mont and k_rt_mul.
//   f_m  : the factors of every segment, concatenated, in Montgomery form (k_rt_to_mont)
//   segs : [gridDim.x] of {first factor of the segment, m}
// Quad k starts from R mod N and multiplies in the factors first + k, first + k + 16, ..: ceil(m / 16) trips, the same for the
// whole wave, a quad with no factor in a trip multiplying by R mod N.  The 16 partial products are then folded through the quads'
// LDS slots in four rounds (strides 8, 4, 2, 1): every quad stores its product, a wave barrier, and quad k < stride multiplies
// by the slot of quad k + stride.  Every quad takes every step: one outside a round's lower half multiplies by its own stored
// value, a number below 2N like every other, and nobody reads its result.  Quad 0 leaves the Montgomery domain by plain 1.  The
// order of the products is free -- the result is the canonical residue, hence the bytes of the pairwise rounds.
// ceil(m / 16) + 4 + 1 Montgomery operations, one product site (every step only chooses its LDS operand).
// ---------------------------------------------------------------------------------------
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_product_segments(const u32* __restrict__ f_m, const uint2* __restrict__ segs,
                                                     uint8_t* __restrict__ out_be, const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int quad = threadIdx.x >> 2;
  u32* slot = lds + quad * SLOT;
  const uint2 seg = segs[blockIdx.x];
  const int m = (int)seg.y;
  const u32* mine = f_m + (size_t)seg.x * L;
  const u32 n0inv = cs->n0inv;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  load_lane_limbs<LPL>(acc, cs->one_m, ln);
  // steps: 0 .. trips-1 times a factor (or R mod N), trips .. trips+3 a fold round, trips+4 final (times plain 1)
  const int trips = (m + RT_NUMS - 1) / RT_NUMS;
#pragma nounroll
  for (int s = 0; s <= trips + 4; ++s) {
    const u32* b = slot;
    if (s < trips) {
      const int k = s * RT_NUMS + quad;
      slot_fill_from_global<LPL>(slot, k < m ? mine + (size_t)k * L : cs->one_m, ln);
    } else if (s < trips + 4) {
      const int stride = (RT_NUMS / 2) >> (s - trips);
      slot_store<LPL>(slot, acc, ln);
      if (quad < stride) b = lds + (quad + stride) * SLOT;
    } else {
      slot_fill_from_global<LPL>(slot, cs->one, ln);
    }
    __builtin_amdgcn_wave_barrier();
    mont_mul<N0INV_RUNTIME>(acc, acc, b, n, ln, n0inv);
    __builtin_amdgcn_wave_barrier();
  }
  store_canonical<LPL>(out_be + (size_t)blockIdx.x * Width<LPL>::EB, acc, slot, cs, ln, quad == 0);
}

// ---------------------------------------------------------------------------------------
// X_i by Horner's rule in the exponent, X = (..((C_{t-1})^i' C_{t-2})^i' ..)^i' C_0 with i' = i mod (q-1).
// For a safe prime q this is the reference's prod_j C_j^(i^j mod (q-1)) for every input: for a unit C_j the
// exponents agree mod q-1 (Fermat); a C_j = 0 mod q gives 0 on both sides when i' > 0 (every i'^j >= 1) and when
// i' = 0 the reference's exponents i^j mod (q-1) of j >= 1 are 0 too, so both sides are C_0.
//   cm : [t][L] commitments in Montgomery form;  squarings run over the wave's largest i'.
// LDS per wave: operand slot + saved-base slot per number, one slot with R mod N.
//   MONT: the result leaves as Montgomery limbs x_m[x][L] (< 2N, no exit product) -- the seeds of the forward differences
// ---------------------------------------------------------------------------------------
//   x, live : the share this quad works on and whether it stores its result (a dead quad is clamped to a live share by the
//             caller); cm and t are wave-uniform, so one workgroup may serve a box of its own (k_rt_commit_eval_tiles)
template <int LPL, bool MONT>
__device__ __forceinline__ void rt_commit_eval_body(u32* lds, const u32* __restrict__ cm, int t, const int64_t* __restrict__ positions,
                                                    int x, bool live, uint8_t* __restrict__ x_be, u32* __restrict__ x_m,
                                                    const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT;
  const Lane ln = make_lane();
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  u32* bslot = lds + (RT_NUMS + (threadIdx.x >> 2)) * SLOT;
  u32* oneslot = lds + 2 * RT_NUMS * SLOT;
  const u32 n0inv = cs->n0inv;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  if (threadIdx.x < 4) slot_fill_from_global<LPL>(oneslot, cs->one_m, ln);
  const u64 qm1 = ((u64)cs->qm1_hi << 32) | cs->qm1_lo;
  u64 pos = (u64)positions[x];
  if (qm1 != 0) pos %= qm1;
  int nb = (pos == 0) ? 0 : 64 - __builtin_clzll(pos);
#pragma unroll
  for (int off = 32; off >= 4; off >>= 1) {
    const int other = __shfl_xor(nb, off);
    nb = other > nb ? other : nb;
  }
  nb = __builtin_amdgcn_readfirstlane(nb);
  __builtin_amdgcn_wave_barrier();

  load_lane_limbs<LPL>(acc, cm + (size_t)(t - 1) * L, ln);
  //   for j = t-2 .. 0:   base = acc; acc = topbit ? base : one
  //                       for bit = nb-2 .. 0: SQUARE; CONDMUL (by base or one, skipped if no lane needs it)
  //                       CMUL (by C_j)
  //   FINAL (by plain 1)
  enum { K_SQUARE, K_CONDMUL, K_CMUL, K_FINAL };
  int j = t - 2, bit = 0, kind = K_FINAL;
  auto begin_coefficient = [&]() {
    if (nb == 0) {   // every i' of the wave is 0: acc^0 = 1
      load_lane_limbs<LPL>(acc, cs->one_m, ln);
      kind = K_CMUL;
      return;
    }
    slot_store<LPL>(bslot, acc, ln);
    if (!((pos >> (nb - 1)) & 1)) load_lane_limbs<LPL>(acc, cs->one_m, ln);
    bit = nb - 2;
    kind = (bit >= 0) ? K_SQUARE : K_CMUL;
  };
  if (j >= 0) begin_coefficient();
  while (true) {
    const u32* bptr = slot;
    bool skip = false;
    if (kind == K_SQUARE) {
      slot_store<LPL>(slot, acc, ln);
    } else if (kind == K_CONDMUL) {
      const bool mine = (pos >> bit) & 1;
      skip = __builtin_amdgcn_ballot_w64(mine) == 0;
      bptr = mine ? bslot : oneslot;
    } else if (kind == K_CMUL) {
      slot_fill_from_global<LPL>(slot, cm + (size_t)j * L, ln);
    } else {
      if (MONT) break;                                  // keep the Montgomery form
      slot_fill_from_global<LPL>(slot, cs->one, ln);
    }
    if (!skip) {
      __builtin_amdgcn_wave_barrier();
      if (kind == K_SQUARE) mont_mul<N0INV_RUNTIME, true>(acc, acc, slot, n, ln, n0inv);
      else mont_mul<N0INV_RUNTIME>(acc, acc, bptr, n, ln, n0inv);
      __builtin_amdgcn_wave_barrier();
    }
    if (kind == K_FINAL) break;
    if (kind == K_SQUARE) {
      kind = K_CONDMUL;
    } else if (kind == K_CONDMUL) {
      --bit;
      kind = (bit >= 0) ? K_SQUARE : K_CMUL;
    } else {
      --j;
      if (j >= 0) begin_coefficient(); else kind = K_FINAL;
    }
  }
  if (MONT) {
    if (live) store_lane_limbs<LPL>(x_m + (size_t)x * L, acc, ln);
    return;
  }
  store_canonical<LPL>(x_be + (size_t)x * Width<LPL>::EB, acc, slot, cs, ln, live);
}

template <int LPL>
__global__ void RT_KERNEL_LDS2(LPL) k_rt_commit_eval(const u32* __restrict__ cm, int t, const int64_t* __restrict__ positions, int count,
                                                uint8_t* __restrict__ x_be, const modp_rt_consts* __restrict__ cs) {
  __shared__ __attribute__((aligned(16))) u32 lds[(2 * RT_NUMS + 1) * Width<LPL>::SLOT];
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  rt_commit_eval_body<LPL, false>(lds, cm, t, positions, live ? xi : count - 1, live, x_be, nullptr, cs);
}

// X of a whole run of boxes in one launch (capi_modp_rt.inc, "Many boxes in one call"): workgroup w serves tile w, up to
// RT_NUMS consecutive shares of ONE box, so the commitments and t of that box are wave-uniform.
//   tiles  : [gridDim.x] of {box, first share of the tile in the run's concatenation, live shares (1 .. RT_NUMS), 0}
//   boxes  : [boxes of the run] of {index of the box's first commitment in cm_all, t}
//   cm_all : the commitments of every box of the run, concatenated, in Montgomery form
// Quads at or beyond the tile's live count are dead lanes, clamped to the tile's last share.
template <int LPL>
__global__ void RT_KERNEL_LDS2(LPL) k_rt_commit_eval_tiles(const u32* __restrict__ cm_all, const uint4* __restrict__ tiles,
                                                      const uint2* __restrict__ boxes, const int64_t* __restrict__ positions,
                                                      uint8_t* __restrict__ x_be, const modp_rt_consts* __restrict__ cs) {
  __shared__ __attribute__((aligned(16))) u32 lds[(2 * RT_NUMS + 1) * Width<LPL>::SLOT];
  const uint4 tile = tiles[blockIdx.x];
  const uint2 box = boxes[tile.x];
  const int quad = threadIdx.x >> 2;
  const bool live = quad < (int)tile.z;
  rt_commit_eval_body<LPL, false>(lds, cm_all + (size_t)box.x * Width<LPL>::L, (int)box.y, positions,
                                  (int)tile.y + (live ? quad : (int)tile.z - 1), live, x_be, nullptr, cs);
}

// Horner in Montgomery form over two sets of commitments in one launch: blockIdx.y = 0 evaluates cm (X at the seed positions),
// 1 evaluates cm_inv, the inverted commitments (X^-1 there).  x_m: [2][count][L].
template <int LPL>
__global__ void RT_KERNEL_LDS2(LPL) k_rt_commit_eval_mont(const u32* __restrict__ cm, const u32* __restrict__ cm_inv, int t,
                                                     const int64_t* __restrict__ positions, int count, u32* __restrict__ x_m,
                                                     const modp_rt_consts* __restrict__ cs) {
  __shared__ __attribute__((aligned(16))) u32 lds[(2 * RT_NUMS + 1) * Width<LPL>::SLOT];
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  rt_commit_eval_body<LPL, true>(lds, blockIdx.y ? cm_inv : cm, t, positions, live ? xi : count - 1, live, nullptr,
                                 x_m + (size_t)blockIdx.y * count * Width<LPL>::L, cs);
}

// ---------------------------------------------------------------------------------------
// Forward differences in the exponent (consecutive positions p0 .. p0+n-1 only; the recurrences of modp_kernels.hip).
// X(i) = prod_j C_j^(i^j) has a polynomial of degree t-1 in the exponent, so with D_0 = X and D_k(c) = D_{k-1}(c+1) / D_{k-1}(c)
//   D_k(c+1) = D_k(c) D_{k+1}(c)  for k < t-1,   D_{t-1} constant:
// t-1 products per share.  The n positions are cut into S contiguous chains (modp_rt_fd_chain); chain c has t seeds in its
// middle, X and X^-1 there by k_rt_commit_eval_mont, and is served by two workgroups: blockIdx.y = 0 steps forward from the
// first seed, 1 backward from the last -- which is the forward scheme over the seeds in reverse order, since Y(j) = X(last - j)
// has a polynomial of the same degree.  A workgroup holds level k in DPP quad k (t <= 16 waves x 16 quads), D in registers,
// each level's operand in its LDS slot, and waits for nothing but its own barrier.
//   table : quad k starts from G_0[k] = X(seed k), H_0[k] = X^-1(seed k); level l = 1 .. t-1 updates the quads k >= l in place,
//           G_l[k] = G_{l-1}[k] H_{l-1}[k-1],  H_l[k] = H_{l-1}[k] G_{l-1}[k-1]
//           (G_l[k] = E_l[k-l], H_l[k] = F_l[k-l] of E_l[k] = E_{l-1}[k+1] F_{l-1}[k], F_l[k] = F_{l-1}[k+1] E_{l-1}[k]); a quad is
//           frozen from level k+1 on, holding E_k[0] = D_k.  Over the reversed seeds the same rule leaves E_k[t-1-k] in quad k
//           for even k and F_k[t-1-k] for odd k: the backward state.  2 (t-1)(t)/2 products, two barriers per level.
//           park: [S][2][16 waves][L] words of HBM scratch.
//   step  : D_k <- D_k D_{k+1}; every quad reads the copy of D_{k+1} its neighbour stored BEFORE the barrier (two slot
//           buffers taken in turn: one barrier per step).  The top level and the idle quads multiply by R mod N.  The first
//           t-1 steps walk over the seeds; from step t on quad 0 stores X in Montgomery limbs, until the chain's edge.
//   x_m   : [n][L]; the forward workgroup also stores the seeds' own X.  k_rt_from_mont makes the canonical bytes.
// LDS: (2 x 16 waves + 1) slots of L words, dynamic.  FdOcc<LPL>::waves = largest workgroup = t_max / 16.
// ---------------------------------------------------------------------------------------
template <int LPL> struct FdOcc { static constexpr int waves = MODP_RT_FD_MAX_T(LPL) / 16; };

template <int LPL>
__global__ void __launch_bounds__(64 * FdOcc<LPL>::waves) k_rt_fd_chain(const u32* __restrict__ seeds_m, int t, int n, int S,
                                                                        u32* __restrict__ x_m, u32* park, const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L;
  extern __shared__ __attribute__((aligned(16))) u32 fd_lds[];
  const Lane ln = make_lane();
  const int k = threadIdx.x >> 2;                        // this quad's level
  const int tp = blockDim.x >> 2;                        // levels of the workgroup, >= t
  const int c = blockIdx.x;
  const bool back = blockIdx.y != 0;
  u32* bufa = fd_lds;
  u32* bufb = fd_lds + (size_t)tp * L;
  u32* oneslot = fd_lds + (size_t)2 * tp * L;
  const u32 n0inv = cs->n0inv;
  int first, len;
  modp_rt_fd_chain(n, S, c, &first, &len);
  const int seed0 = first + (len - t) / 2;               // index (within the n positions) of the chain's first seed
  u32 nn[LPL], g[LPL];
  load_lane_limbs<LPL>(nn, cs->n, ln);
  if (threadIdx.x < 4) slot_fill_from_global<LPL>(oneslot, cs->one_m, ln);
  const bool act = k < t;
  u32* mypark = park + (((size_t)c * 2 + blockIdx.y) * tp + k) * L;
  {
    const int sk = back ? t - 1 - k : k;
    const u32* sx = act ? seeds_m + ((size_t)c * t + sk) * L : cs->one_m;
    const u32* si = act ? sx + (size_t)S * t * L : cs->one_m;
    load_lane_limbs<LPL>(g, si, ln);
    slot_store<LPL>(bufb + (size_t)k * L, g, ln);
    load_lane_limbs<LPL>(g, sx, ln);
    slot_store<LPL>(bufa + (size_t)k * L, g, ln);
    if (act && !back) store_lane_limbs<LPL>(x_m + (size_t)(seed0 + k) * L, g, ln);
  }
  __syncthreads();
  // Between two levels G lives in bufa and H in bufb.  A level forms H' first and parks it in the quad's own words of `park`
  // (HBM; every lane reads back what it wrote), then G', so that one number at a time is in registers beside the modulus and
  // the accumulators; both go to the slots once every quad has read the old ones.
  const int wave_top = (k | 15);                         // highest level of this wave
  for (int l = 1; l < t; ++l) {
    const bool upd = act && k >= l;
    if (wave_top >= l) {                                 // wave-uniform: a wave of frozen quads only keeps the barriers
#pragma nounroll
      for (int half = 0; half < 2; ++half) {             // H' = H G[k-1], then G' = G H[k-1]: one product site
        const u32* own = half ? bufa : bufb;
        const u32* other = half ? bufb : bufa;
        slot_load<LPL>(g, own + (size_t)k * L, ln);
        mont_mul<N0INV_RUNTIME>(g, g, upd ? other + (size_t)(k - 1) * L : oneslot, nn, ln, n0inv);
        if (half == 0) store_lane_limbs<LPL>(mypark, g, ln);
      }
    }
    __syncthreads();
    if (wave_top >= l) {
      slot_store<LPL>(bufa + (size_t)k * L, g, ln);
      load_lane_limbs<LPL>(g, mypark, ln);
      slot_store<LPL>(bufb + (size_t)k * L, g, ln);
    }
    __syncthreads();
  }
  slot_load<LPL>(g, bufa + (size_t)k * L, ln);
  __syncthreads();
  // g = D_k of this direction
  const int m = back ? seed0 - first : first + len - (seed0 + t);      // shares this direction has to produce
  const int steps = m > 0 ? t - 1 + m : 0;
  const bool reads_next = k + 1 < t;
  for (int i = 1; i <= steps; ++i) {
    u32* buf = (i & 1) ? bufb : bufa;
    slot_store<LPL>(buf + (size_t)k * L, g, ln);
    __syncthreads();
    mont_mul<N0INV_RUNTIME>(g, g, reads_next ? buf + (size_t)(k + 1) * L : oneslot, nn, ln, n0inv);
    if (k == 0 && i >= t) {
      const int idx = back ? seed0 + t - 1 - i : seed0 + i;            // in [first, first + len) by the choice of `steps`
      store_lane_limbs<LPL>(x_m + (size_t)idx * L, g, ln);
    }
  }
}

// out[x] = canonical bytes of x_m[x] (Montgomery limbs < 2N): times plain 1
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_from_mont(const u32* __restrict__ x_m, int count, uint8_t* __restrict__ out_be,
                                              const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  load_lane_limbs<LPL>(acc, x_m + (size_t)x * L, ln);
  slot_fill_from_global<LPL>(slot, cs->one, ln);
  __builtin_amdgcn_wave_barrier();
  mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
  __builtin_amdgcn_wave_barrier();
  store_canonical<LPL>(out_be + (size_t)x * Width<LPL>::EB, acc, slot, cs, ln, live);
}

// =======================================================================================
// The scalar ring Z/(q-1) of a run-time group on the device: the dealer's P(i), the responses r_i = w_i - P(i) c and the
// participant's e2_i = w_i / x_i (src/polynomial.rs:50-58, src/dleq.rs:42-50, src/groups/modp.rs:180-182).  The decomposition
// is group 14's (k_modq_* in modp_kernels.hip): for odd q' = (q-1)/2, Z/(q-1) = Z/2 x Z/q'; a scalar is its residue mod q' --
// in the Montgomery machinery above with `cs` the constants of q', built at the handle's own width (q' has one bit fewer than
// q: R > 8 q') -- and its parity, and it is lifted to [0, q-1) when it is written.  Every input is an EB-byte value of any size:
// it enters through to_mont_in, which reduces it mod q'; reducing mod the even q - 1 preserves its parity, so the parity is read
// from the input's last byte.  Bounds and operation counts: tests/test_modp_rt_scalar_model.py.
// =======================================================================================

// a += b limb by limb, carries inside the lane and one hand-over to the next lane: almost normalised again.  The sums here stay
// below 4 q' < R / 2, so the top lane has no carry-out.
template <int LPL>
__device__ __forceinline__ void add_limbs(u32 (&a)[LPL], const u32 (&b)[LPL], const Lane& ln) {
  u32 c = 0;
#pragma unroll
  for (int k = 0; k < LPL; ++k) {
    const u32 v = a[k] + b[k] + c;
    a[k] = v & MASK;
    c = v >> W;
  }
  a[0] += bn::quad_from_prev(c) & ln.not_low;
}

// The lane for one more to_mont_in in the same kernel.  to_mont_in reads its input as some hundred byte loads at offsets that
// depend on the lane's place in the quad; a second input would share those 64-bit offsets with the first, and the compiler
// keeps all of them alive across the product in between and spills them.  An opaque copy of the place makes it form them again.
__device__ __forceinline__ Lane lane_again(const Lane& ln) {
  Lane l2 = ln;
  asm volatile("" : "+v"(l2.q));
  return l2;
}

// store_canonical against q' with a parity: the residue v in [0, q') leaves as the one number in [0, 2 q') = [0, q-1) of that
// parity, v or v + q' (q' is odd, so adding it flips the low bit); quad lane 0 does the lifting (limbs::slot_canonicalize)
template <int LPL>
__device__ __forceinline__ void store_canonical_lift(uint8_t* __restrict__ out, const u32 (&a)[LPL], u32* slot,
                                                     const modp_rt_consts* __restrict__ cs, const Lane& ln, bool write, int parity) {
  constexpr int L = Width<LPL>::L, EB = Width<LPL>::EB, WPL = EB / 16;
  slot_store<LPL>(slot, a, ln);
  __builtin_amdgcn_wave_barrier();
  if (ln.q == 0) limbs::slot_canonicalize<L>(slot, cs->n, parity);
  __builtin_amdgcn_wave_barrier();
  if (write) {
    u32* out32 = reinterpret_cast<u32*>(out);
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      const int wd = (int)ln.q * WPL + i;
      out32[4 * WPL - 1 - wd] = __builtin_bswap32(limbs::slot_word32<L, EB>(slot, wd));
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------------------
// out[x] = a[x] b[x] mod (q-1).  Steps: a R; b R; a R b R R^-1 = a b R; times plain 1.  2 entry products + 1 + 1 exit.
// Parity: that of the integer product.
// ---------------------------------------------------------------------------------------
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_modq_mul(const uint8_t* __restrict__ a_be, const uint8_t* __restrict__ b_be, int count,
                                             uint8_t* __restrict__ out_be, const modp_rt_consts* __restrict__ cs) {
  constexpr int SLOT = Width<LPL>::SLOT, EB = Width<LPL>::EB;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  const uint8_t* pa = a_be + (size_t)x * EB;
  const uint8_t* pb = b_be + (size_t)x * EB;
  const int parity = (int)(pa[EB - 1] & pb[EB - 1] & 1u);
  u32 n[LPL], acc[LPL], v[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  to_mont_in<LPL>(acc, slot, pa, cs, n, n0inv, ln);
  to_mont_in<LPL>(v, slot, pb, cs, n, n0inv, lane_again(ln));
  slot_store<LPL>(slot, v, ln);
#pragma nounroll
  for (int step = 0; step < 2; ++step) {
    if (step == 1) slot_fill_from_global<LPL>(slot, cs->one, ln);
    __builtin_amdgcn_wave_barrier();
    mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
    __builtin_amdgcn_wave_barrier();
  }
  store_canonical_lift<LPL>(out_be + (size_t)x * EB, acc, slot, cs, ln, live, parity);
}

// ---------------------------------------------------------------------------------------
// r[x] = w[x] - alpha[x] c mod (q-1) for one shared c.
//   cneg_be : (-c) mod q' as EB big-endian bytes (device), c_parity = c mod 2
// Steps: (-c) R; alpha R and (-c) R alpha R R^-1 = -alpha c R (< 2 q'); w R (< 2 q'), added in the Montgomery domain (< 4 q' < R),
// times plain 1 (back below 2 q').  3 entry products + 1 + 1 exit.  Parity: w ^ (alpha & c) in the lowest bit.
// ---------------------------------------------------------------------------------------
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_modq_responses(const uint8_t* __restrict__ w_be, const uint8_t* __restrict__ alpha_be,
                                                   const uint8_t* __restrict__ cneg_be, int c_parity, int count,
                                                   uint8_t* __restrict__ out_be, const modp_rt_consts* __restrict__ cs) {
  constexpr int SLOT = Width<LPL>::SLOT, EB = Width<LPL>::EB;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  const uint8_t* pw = w_be + (size_t)x * EB;
  const uint8_t* pal = alpha_be + (size_t)x * EB;
  const int parity = (int)((pw[EB - 1] ^ (pal[EB - 1] & (uint8_t)c_parity)) & 1u);
  u32 n[LPL], acc[LPL], v[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  to_mont_in<LPL>(acc, slot, cneg_be, cs, n, n0inv, ln);
  to_mont_in<LPL>(v, slot, pal, cs, n, n0inv, lane_again(ln));
  slot_store<LPL>(slot, v, ln);
  __builtin_amdgcn_wave_barrier();
  mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);           // -alpha c R
  __builtin_amdgcn_wave_barrier();
  to_mont_in<LPL>(v, slot, pw, cs, n, n0inv, lane_again(ln));
  add_limbs<LPL>(acc, v, ln);                                      // (w - alpha c) R, < 4 q'
  slot_fill_from_global<LPL>(slot, cs->one, ln);
  __builtin_amdgcn_wave_barrier();
  mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
  __builtin_amdgcn_wave_barrier();
  store_canonical_lift<LPL>(out_be + (size_t)x * EB, acc, slot, cs, ln, live, parity);
}

// ---------------------------------------------------------------------------------------
// out[x] = P(positions[x]) mod (q-1), P = sum_j a_j X^j, by Horner's rule in Montgomery form.
//   coef_m      : [t][L] limbs of (a_j mod q') R mod q' (canonical; the dealer's secret, staged and wiped by the caller)
//   positions   : 0 <= i < 2^63, used as integers: three limbs, which enter Montgomery form by the long product of to_mont_in
//   par_even/odd: parity of P at even / odd positions (a_0, resp. the XOR of all a_j)
// acc <- acc iR R^-1 + a_j R with a normalising add: acc < 4 q' before every product (a product of a < 4 q' and b < 2 q' is
// below q' + 8 q'^2 / R < 2 q'), t - 1 products per share, 1 entry and 1 exit.  One product site in the loop: the last round
// multiplies by plain 1 and adds nothing.
// ---------------------------------------------------------------------------------------
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_modq_poly_eval(const u32* __restrict__ coef_m, int t, const int64_t* __restrict__ positions, int count,
                                                   int par_even, int par_odd, uint8_t* __restrict__ out_be,
                                                   const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT, EB = Width<LPL>::EB, IN_ROWS = Width<LPL>::IN_ROWS;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const int xi = blockIdx.x * RT_NUMS + (threadIdx.x >> 2);
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + (threadIdx.x >> 2) * SLOT;
  const u32 n0inv = cs->n0inv;
  const u64 pos = (u64)positions[x];
  u32 n[LPL], acc[LPL], v[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  // i R mod q' (< 2 q'), left in the slot for the whole loop
#pragma unroll
  for (int j = 0; j < IN_ROWS; j += 4) {
    const int jj = j + (int)ln.q;
    if (jj < IN_ROWS) slot[jj] = jj < 3 ? (u32)(pos >> (W * jj)) & MASK : 0u;
  }
  load_lane_limbs<LPL>(v, cs->kin, ln);
  __builtin_amdgcn_wave_barrier();
  mont_mul<N0INV_RUNTIME, false, IN_ROWS / LPL>(acc, v, slot, n, ln, n0inv);
  __builtin_amdgcn_wave_barrier();
  slot_store<LPL>(slot, acc, ln);
  load_lane_limbs<LPL>(acc, coef_m + (size_t)(t - 1) * L, ln);
#pragma nounroll
  for (int j = t - 2; j >= -1; --j) {
    if (j < 0) slot_fill_from_global<LPL>(slot, cs->one, ln);
    __builtin_amdgcn_wave_barrier();
    mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);
    __builtin_amdgcn_wave_barrier();
    if (j >= 0) {
      load_lane_limbs<LPL>(v, coef_m + (size_t)j * L, ln);
      add_limbs<LPL>(acc, v, ln);
    }
  }
  store_canonical_lift<LPL>(out_be + (size_t)x * EB, acc, slot, cs, ln, live, (pos & 1) ? par_odd : par_even);
}

// =======================================================================================
// The Lagrange exponents of reconstruct on the device (capi_modp_rt.inc, "Lagrange exponents on the device"): for a list of m
// positions, |lambda_i| = prod_{j != i} x_j / prod_{j != i} |x_j - x_i| mod q', written as the exponent the host writes
// (rt_lagrange_exponent).  `cs` is the image of the constants of q' throughout.  Three steps, all on tiles of up to RT_NUMS
// coefficients of ONE list (rows {the list's first position, m, the tile's first coefficient, live quads}; workgroup w of a launch
// serves row w and owns the slots 16 w .. 16 w + 15 of the launch's work arrays, dead quads included):
//   k_rt_lagrange_terms   numerator and denominator of every coefficient, the denominator also as canonical bytes;
//   k_rt_table + k_rt_dual_exp with the one exponent q' - 2 over those bytes: den^(q'-2), the inverse when q' is prime (Fermat);
//   k_rt_lagrange_finish  checks den den^-1 = 1, forms the magnitude and stores the exponent.
// Bounds, the cancellation and the product counts: tests/test_modp_rt_lagrange_model.py.
// =======================================================================================

// Quad i starts both accumulators from R mod q' and takes m - 1 steps: step j multiplies x_jj into the numerator and |x_jj - x_i|
// into the denominator, jj = j for j < i and j + 1 from there on (its own index is skipped, every quad of the wave takes the same
// number of steps).  A factor is below 2^63: three 29-bit limbs in an operand of LPL limbs, one quarter product
// (bn::mont_mul<.., OUTER = 1>) -- acc <- acc f 2^(-29 LPL), below q' + 2 q' 2^87 / 2^(29 LPL) < 2 q'.  Both accumulators carry
// the same stray 2^(-29 LPL (m-1)): it cancels in the quotient.  The list's positions pass through LDS MODP_RT_LAGRANGE_STAGE
// steps at a time (one position more than steps: the shifted index); nothing at or past first + m is read.  Loop bounds and
// barriers are wave-uniform; a dead quad works on the tile's last live coefficient and writes a slot nobody reads back.
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_lagrange_terms(const int64_t* __restrict__ positions, const uint4* __restrict__ tiles,
                                                   u32* __restrict__ num_m, u32* __restrict__ den_m, uint8_t* __restrict__ den_be,
                                                   const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT, EB = Width<LPL>::EB, STAGE = MODP_RT_LAGRANGE_STAGE;
  static_assert(2 * LPL + LPL + 1 <= SLOT, "two operands of LPL limbs (and the prefetched word after each) in one slot");
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  __shared__ int64_t stage[STAGE + 1];
  const Lane ln = make_lane();
  const uint4 tile = tiles[blockIdx.x];
  const u32 first = tile.x, m = tile.y, live = tile.w;
  const int quad = threadIdx.x >> 2;
  const u32 i = tile.z - first + ((u32)quad < live ? (u32)quad : live - 1);      // this quad's index in its list, < m
  const size_t sl = (size_t)blockIdx.x * RT_NUMS + quad;
  u32* slot = lds + quad * SLOT;
  u32* opn = slot;
  u32* opd = slot + 2 * LPL;
  const u32 n0inv = cs->n0inv;
  const u64 xi = (u64)positions[(size_t)first + i];
  u32 n[LPL], num[LPL], den[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
#pragma unroll
  for (int k = 0; k < LPL; ++k) num[k] = 0;
  slot_store<LPL>(slot, num, ln);                        // limbs 3 .. LPL of both operands stay 0
  load_lane_limbs<LPL>(num, cs->one_m, ln);
#pragma unroll
  for (int k = 0; k < LPL; ++k) den[k] = num[k];
  const u32 steps = m - 1;
  for (u32 base = 0; base < steps; base += STAGE) {
    const u32 cnt = steps - base < (u32)STAGE ? steps - base : (u32)STAGE;
    for (u32 k = threadIdx.x; k <= cnt; k += 64) stage[k] = positions[(size_t)first + base + k];   // base + cnt <= m - 1
    __syncthreads();
#pragma nounroll
    for (u32 k = 0; k < cnt; ++k) {
      const u64 xj = (u64)stage[k + (base + k >= i ? 1u : 0u)];
      u64 d = xj - xi;                                   // |x_j - x_i| < 2^63: both lie in [1, 2^63)
      if ((int64_t)d < 0) d = 0 - d;
      if (ln.q < 3) {
        opn[ln.q] = (u32)(xj >> (W * ln.q)) & MASK;
        opd[ln.q] = (u32)(d >> (W * ln.q)) & MASK;
      }
      __builtin_amdgcn_wave_barrier();
      mont_mul<N0INV_RUNTIME, false, 1>(num, num, opn, n, ln, n0inv);
      mont_mul<N0INV_RUNTIME, false, 1>(den, den, opd, n, ln, n0inv);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
  }
  store_lane_limbs<LPL>(num_m + sl * L, num, ln);
  store_lane_limbs<LPL>(den_m + sl * L, den, ln);
  store_canonical<LPL>(den_be + sl * EB, den, slot, cs, ln, true);
}

// store_canonical_lift with a sign instead of a parity: the residue mag in [0, q') leaves as the exponent the host writes, mag
// itself, or (q - 1) - mag = 2 q' - mag for a negative coefficient of nonzero magnitude (the residue -mag mod q', plus q')
template <int LPL>
__device__ __forceinline__ void store_canonical_signed(uint8_t* __restrict__ out, const u32 (&a)[LPL], u32* slot,
                                                       const modp_rt_consts* __restrict__ cs, const Lane& ln, bool write, bool negative) {
  constexpr int L = Width<LPL>::L, EB = Width<LPL>::EB, WPL = EB / 16;
  slot_store<LPL>(slot, a, ln);
  __builtin_amdgcn_wave_barrier();
  if (ln.q == 0) {
    limbs::slot_canonicalize<L>(slot, cs->n);
    u32 any = 0;
#pragma nounroll
    for (int j = 0; j < L; ++j) any |= slot[j];
    if (negative && any) {
      int64_t c = 0;
#pragma nounroll
      for (int j = 0; j < L; ++j) {
        const int64_t t = 2 * (int64_t)cs->n[j] - (int64_t)slot[j] + c;
        slot[j] = (u32)t & MASK;
        c = t >> W;
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  if (write) {
    u32* out32 = reinterpret_cast<u32*>(out);
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      const int wd = (int)ln.q * WPL + i;
      out32[4 * WPL - 1 - wd] = __builtin_bswap32(limbs::slot_word32<L, EB>(slot, wd));
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// exps[c] and flags[c] of every live coefficient c of the tiles from the work arrays of k_rt_lagrange_terms and dinv = den^(q'-2):
// dinv R by the entry product, then den dinv (the check) and num dinv (the magnitude; the stray power has cancelled), both out of
// the Montgomery domain.  flags[c] = 1 iff den dinv is 1 mod q': then dinv IS the inverse, whatever q' is; a denominator that is 0
// mod a small q', or a composite q' where Fermat's power is no inverse, gives 0 and the host recomputes the list.  1 entry
// product + 2.  neg[c]: the sign of coefficient c (host: the parity of the rank of x_i in its sorted list).
template <int LPL>
__global__ void RT_KERNEL(LPL) k_rt_lagrange_finish(const uint4* __restrict__ tiles, const u32* __restrict__ num_m,
                                                    const u32* __restrict__ den_m, const uint8_t* __restrict__ dinv_be,
                                                    const uint8_t* __restrict__ neg, uint8_t* __restrict__ exps, uint8_t* __restrict__ flags,
                                                    const modp_rt_consts* __restrict__ cs) {
  constexpr int L = Width<LPL>::L, SLOT = Width<LPL>::SLOT, EB = Width<LPL>::EB;
  __shared__ __attribute__((aligned(16))) u32 lds[RT_NUMS * SLOT];
  const Lane ln = make_lane();
  const uint4 tile = tiles[blockIdx.x];
  const int quad = threadIdx.x >> 2;
  const bool live = (u32)quad < tile.w;
  const size_t c = (size_t)tile.z + (live ? (u32)quad : tile.w - 1);
  const size_t sl = (size_t)blockIdx.x * RT_NUMS + quad;
  u32* slot = lds + quad * SLOT;
  const u32 n0inv = cs->n0inv;
  u32 n[LPL], acc[LPL], v[LPL];
  load_lane_limbs<LPL>(n, cs->n, ln);
  to_mont_in<LPL>(v, slot, dinv_be + sl * EB, cs, n, n0inv, ln);
  slot_store<LPL>(slot, v, ln);
  load_lane_limbs<LPL>(acc, den_m + sl * L, ln);
  load_lane_limbs<LPL>(v, num_m + sl * L, ln);
  __builtin_amdgcn_wave_barrier();
  mont_mul<N0INV_RUNTIME>(acc, acc, slot, n, ln, n0inv);           // den dinv
  mont_mul<N0INV_RUNTIME>(v, v, slot, n, ln, n0inv);               // num dinv
  __builtin_amdgcn_wave_barrier();
  slot_store<LPL>(slot, acc, ln);
  __builtin_amdgcn_wave_barrier();
  if (ln.q == 0) {
    limbs::slot_canonicalize<L>(slot, cs->n);
    u32 rest = slot[0] ^ 1u;
#pragma nounroll
    for (int j = 1; j < L; ++j) rest |= slot[j];
    if (live) flags[c] = rest == 0 ? 1 : 0;
  }
  __builtin_amdgcn_wave_barrier();
  store_canonical_signed<LPL>(exps + c * EB, v, slot, cs, ln, live, neg[c] != 0);
}

// ---------------------------------------------------------------------------------------
// launchers: RT_FN names them (modp_rt_launch_* here, modp_rt27_launch_* in the wide unit, modp_rt36_launch_* in the 4096-bit one), RT_DISPATCH launches the
// instance of a width this unit holds, RT_ELSEWHERE hands a width of another unit over to it
// ---------------------------------------------------------------------------------------
static inline int rt_grid(int count) { return (count + RT_NUMS - 1) / RT_NUMS; }
// rows of a width's comb and of one key of a key set (Width::COMB_ROWS, Width::KS_ROWS follow EB alone)
static inline int rt_comb_rows(int lpl) { return lpl == 36 ? Width<36>::COMB_ROWS : lpl == 27 ? Width<27>::COMB_ROWS : Width<18>::COMB_ROWS; }
static inline int rt_ks_rows(int lpl) { return lpl == 36 ? Width<36>::KS_ROWS : lpl == 27 ? Width<27>::KS_ROWS : Width<18>::KS_ROWS; }

#ifdef RT_WIDTH_FREE
// ---------------------------------------------------------------------------------------
// The challenge of each box of a run, written to every share of the box: c_out[first + i] = c_box[box] for the live shares i of
// tile blockIdx.x (the tile table of k_rt_commit_eval_tiles).  Plain bytes moved as 32-bit words, eb a multiple of 4: no width,
// so the unit that defines RT_WIDTH_FREE holds the one instance.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_rt_spread_challenge(const u32* __restrict__ c_box, const uint4* __restrict__ tiles, int eb,
                                                            u32* __restrict__ c_out) {
  const uint4 tile = tiles[blockIdx.x];
  const int words = eb / 4, total = (int)tile.z * words;
  const u32* src = c_box + (size_t)tile.x * words;
  u32* dst = c_out + (size_t)tile.y * words;
  for (int i = threadIdx.x; i < total; i += 64) dst[i] = src[i % words];
}

extern "C" int modp_rt_launch_spread_challenge(const uint8_t* c_box, const uint32_t* tiles, int ntiles, int eb, uint8_t* c_out,
                                               hipStream_t s) {
  if (ntiles <= 0) return 0;
  if (eb <= 0 || (eb & 3)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rt_spread_challenge, dim3(ntiles), dim3(64), 0, s, reinterpret_cast<const u32*>(c_box),
                     reinterpret_cast<const uint4*>(tiles), eb, reinterpret_cast<u32*>(c_out));
  return (int)hipGetLastError();
}
#endif  // RT_WIDTH_FREE

#ifndef RT_FD_ONLY
extern "C" int RT_FN(launch_to_mont)(int lpl, const uint8_t* in_be, int count, uint32_t* out_m, const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_to_mont, lpl, in_be, count, out_m, cs, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_to_mont, dim3(rt_grid(count)), dim3(64), 0, s, in_be, count, out_m, cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_table)(int lpl, const uint8_t* base_be, size_t base_stride, int count, uint32_t* tab,
                                   const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_table, lpl, base_be, base_stride, count, tab, cs, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_table, dim3(rt_grid(count)), dim3(64), 0, s, base_be, base_stride, count, tab, cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_dual_exp)(int lpl, const uint32_t* tab1, size_t tab1_stride, const uint32_t* tab2, size_t tab2_stride,
                                      const uint8_t* e1, size_t e1_stride, const uint8_t* e2, size_t e2_stride, int count, uint8_t* out,
                                      const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_dual_exp, lpl, tab1, tab1_stride, tab2, tab2_stride, e1, e1_stride, e2, e2_stride, count, out, cs, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_dual_exp, dim3(rt_grid(count)), dim3(64), 0, s, tab1, tab1_stride, tab2, tab2_stride, e1, e1_stride, e2,
              e2_stride, count, out, cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_comb_build)(int lpl, const uint8_t* base_be, uint32_t* comb, const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_comb_build, lpl, base_be, comb, cs, s);
  RT_DISPATCH(lpl, k_rt_comb_bases, dim3(1), dim3(64), 0, s, base_be, comb, cs);
  RT_DISPATCH(lpl, k_rt_comb_rows, dim3(rt_grid(rt_comb_rows(lpl))), dim3(64), 0, s, comb, cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_comb_exp)(int lpl, const uint32_t* comb, const uint32_t* tab2, size_t tab2_stride, const uint8_t* e1,
                                      const uint8_t* e2, size_t e2_stride, int count, uint8_t* out, const modp_rt_consts* cs,
                                      hipStream_t s) {
  RT_ELSEWHERE(launch_comb_exp, lpl, comb, tab2, tab2_stride, e1, e2, e2_stride, count, out, cs, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_comb_exp, dim3(rt_grid(count)), dim3(64), 0, s, comb, tab2, tab2_stride, e1, e2, e2_stride, count, out, cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_exp_sets)(int lpl, const uint32_t* tab, size_t tab_stride, const uint8_t* e1, const uint8_t* e2, int count,
                                      uint8_t* out1, uint8_t* out2, const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_exp_sets, lpl, tab, tab_stride, e1, e2, count, out1, out2, cs, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_exp_sets, dim3(rt_grid(count), 2), dim3(64), 0, s, tab, tab_stride, e1, e2, count, out1, out2, cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_keyset_build)(int lpl, const uint8_t* keys_be, int count, uint32_t* ks, const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_keyset_build, lpl, keys_be, count, ks, cs, s);
  if (count <= 0) return 0;
  const int nrows = count * rt_ks_rows(lpl);
  RT_DISPATCH(lpl, k_rt_keyset_bases, dim3(rt_grid(count)), dim3(64), 0, s, keys_be, count, ks, cs);
  RT_DISPATCH(lpl, k_rt_keyset_rows, dim3(rt_grid(nrows)), dim3(64), 0, s, ks, nrows, cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_keyset_exp)(int lpl, const uint32_t* ks, const uint32_t* tab2, size_t tab2_stride, const uint8_t* e1a,
                                        const uint8_t* e1b, const uint8_t* e2, size_t e2_stride, int count, uint8_t* out_a,
                                        uint8_t* out_b, const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_keyset_exp, lpl, ks, tab2, tab2_stride, e1a, e1b, e2, e2_stride, count, out_a, out_b, cs, s);
  if (count <= 0) return 0;
  if (e1b && tab2) return (int)hipErrorInvalidValue;       // the second exponent set is for powers of the key alone
  RT_DISPATCH(lpl, k_rt_keyset_exp, dim3(rt_grid(count), e1b ? 2 : 1), dim3(64), 0, s, ks, tab2, tab2_stride, e1a, e1b, e2, e2_stride,
              count, out_a, out_b, cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_keyset_exp_idx)(int lpl, const uint32_t* ks, const uint32_t* key_of, const uint32_t* tab2, size_t tab2_stride,
                                            const uint8_t* e1, const uint8_t* e2, size_t e2_stride, int count, uint8_t* out,
                                            const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_keyset_exp_idx, lpl, ks, key_of, tab2, tab2_stride, e1, e2, e2_stride, count, out, cs, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_keyset_exp_idx, dim3(rt_grid(count)), dim3(64), 0, s, ks, key_of, tab2, tab2_stride, e1, e2, e2_stride, count, out,
              cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_twin_exp)(int lpl, const uint8_t* bases, const uint8_t* e1, const uint8_t* e2, int count, uint32_t* buckets,
                                      uint8_t* out1, uint8_t* out2, const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_twin_exp, lpl, bases, e1, e2, count, buckets, out1, out2, cs, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_twin_exp, dim3(rt_grid(count)), dim3(64), 0, s, bases, e1, e2, count, buckets, cs);
  RT_DISPATCH(lpl, k_rt_twin_combine, dim3(rt_grid(count), 2), dim3(64), 0, s, buckets, count, out1, out2, cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_mul)(int lpl, const uint32_t* a, const uint32_t* b, int count, uint8_t* out, const modp_rt_consts* cs,
                                 hipStream_t s) {
  RT_ELSEWHERE(launch_mul, lpl, a, b, count, out, cs, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_mul, dim3(rt_grid(count)), dim3(64), 0, s, a, b, count, out, cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_product_segments)(int lpl, const uint32_t* f_m, const uint32_t* segs, int nsegs, uint8_t* out,
                                              const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_product_segments, lpl, f_m, segs, nsegs, out, cs, s);
  if (nsegs <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_product_segments, dim3(nsegs), dim3(64), 0, s, f_m, reinterpret_cast<const uint2*>(segs), out, cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_commit_eval)(int lpl, const uint32_t* cm_m, int t, const int64_t* positions, int count, uint8_t* x_be,
                                         const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_commit_eval, lpl, cm_m, t, positions, count, x_be, cs, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_commit_eval, dim3(rt_grid(count)), dim3(64), 0, s, cm_m, t, positions, count, x_be, cs);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_commit_eval_tiles)(int lpl, const uint32_t* cm_all_m, const uint32_t* tiles, int ntiles, const uint32_t* boxes,
                                               const int64_t* positions, uint8_t* x_be, const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_commit_eval_tiles, lpl, cm_all_m, tiles, ntiles, boxes, positions, x_be, cs, s);
  if (ntiles <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_commit_eval_tiles, dim3(ntiles), dim3(64), 0, s, cm_all_m, reinterpret_cast<const uint4*>(tiles),
              reinterpret_cast<const uint2*>(boxes), positions, x_be, cs);
  return (int)hipGetLastError();
}

// Seeds of the forward differences: X (and, from the inverted commitments, X^-1) at `count` positions, Montgomery limbs,
// x_m [2][count][L]
extern "C" int RT_FN(launch_commit_eval_mont)(int lpl, const uint32_t* cm_m, const uint32_t* cm_inv_m, int t, const int64_t* positions,
                                              int count, uint32_t* x_m, const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_commit_eval_mont, lpl, cm_m, cm_inv_m, t, positions, count, x_m, cs, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_commit_eval_mont, dim3(rt_grid(count), 2), dim3(64), 0, s, cm_m, cm_inv_m, t, positions, count, x_m, cs);
  return (int)hipGetLastError();
}

#endif  // RT_FD_ONLY

#ifndef RT_FD_ELSEWHERE
template <int LPL>
static int rt_fd_launch(const uint32_t* seeds_m, int t, int n, int S, uint32_t* x_m, uint32_t* park, const modp_rt_consts* cs, hipStream_t s) {
  const int waves = (t + 15) / 16;
  const size_t lds = ((size_t)2 * 16 * waves + 1) * Width<LPL>::L * sizeof(u32);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rt_fd_chain<LPL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_rt_fd_chain<LPL>, dim3(S, 2), dim3(64 * waves), lds, s, seeds_m, t, n, S, x_m, park, cs);
  return (int)hipGetLastError();
}

// X in Montgomery limbs at all n consecutive positions from the seeds of S chains (seeds_m [2][S][t][L], chain geometry
// modp_rt_fd_chain); park: scratch of modp_rt_fd_park_bytes(lpl, t, S) bytes: 2 <= t <= modp_rt_fd_max_t(lpl), 1 <= S, S t <= n
extern "C" int RT_FN(launch_fd_chains)(int lpl, const uint32_t* seeds_m, int t, int n, int S, uint32_t* x_m, uint32_t* park,
                                       const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_fd_chains, lpl, seeds_m, t, n, S, x_m, park, cs, s);
  if (t < 2 || t > MODP_RT_FD_MAX_T(lpl) || S < 1 || n / S < t) return (int)hipErrorInvalidValue;
  return RT_DISPATCH_FN(lpl, rt_fd_launch, seeds_m, t, n, S, x_m, park, cs, s);
}

#else
// this unit's widths of k_rt_fd_chain live in a unit of their own (modp_rt_fd_kernels.hip: another unroll threshold)
extern "C" int RT_FN(launch_fd_chains)(int lpl, const uint32_t* seeds_m, int t, int n, int S, uint32_t* x_m, uint32_t* park,
                                       const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_fd_chains, lpl, seeds_m, t, n, S, x_m, park, cs, s);
  return RT_FD_ELSEWHERE(lpl, seeds_m, t, n, S, x_m, park, cs, s);
}
#endif  // RT_FD_ELSEWHERE

#ifndef RT_FD_ONLY
extern "C" int RT_FN(launch_from_mont)(int lpl, const uint32_t* x_m, int count, uint8_t* out_be, const modp_rt_consts* cs, hipStream_t s) {
  RT_ELSEWHERE(launch_from_mont, lpl, x_m, count, out_be, cs, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_from_mont, dim3(rt_grid(count)), dim3(64), 0, s, x_m, count, out_be, cs);
  return (int)hipGetLastError();
}

// the scalar ring Z/(q-1): csq is the device image of the constants of q' = (q-1)/2
extern "C" int RT_FN(launch_modq_mul)(int lpl, const uint8_t* a_be, const uint8_t* b_be, int count, uint8_t* out_be,
                                      const modp_rt_consts* csq, hipStream_t s) {
  RT_ELSEWHERE(launch_modq_mul, lpl, a_be, b_be, count, out_be, csq, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_modq_mul, dim3(rt_grid(count)), dim3(64), 0, s, a_be, b_be, count, out_be, csq);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_modq_responses)(int lpl, const uint8_t* w_be, const uint8_t* alpha_be, const uint8_t* cneg_be, int c_parity,
                                            int count, uint8_t* out_be, const modp_rt_consts* csq, hipStream_t s) {
  RT_ELSEWHERE(launch_modq_responses, lpl, w_be, alpha_be, cneg_be, c_parity, count, out_be, csq, s);
  if (count <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_modq_responses, dim3(rt_grid(count)), dim3(64), 0, s, w_be, alpha_be, cneg_be, c_parity, count, out_be, csq);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_modq_poly_eval)(int lpl, const uint32_t* coef_m, int t, const int64_t* positions, int count, int par_even,
                                            int par_odd, uint8_t* out_be, const modp_rt_consts* csq, hipStream_t s) {
  RT_ELSEWHERE(launch_modq_poly_eval, lpl, coef_m, t, positions, count, par_even, par_odd, out_be, csq, s);
  if (count <= 0 || t <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_modq_poly_eval, dim3(rt_grid(count)), dim3(64), 0, s, coef_m, t, positions, count, par_even, par_odd, out_be, csq);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_lagrange_terms)(int lpl, const int64_t* positions, const uint32_t* tiles, int ntiles, uint32_t* num_m,
                                            uint32_t* den_m, uint8_t* den_be, const modp_rt_consts* csq, hipStream_t s) {
  RT_ELSEWHERE(launch_lagrange_terms, lpl, positions, tiles, ntiles, num_m, den_m, den_be, csq, s);
  if (ntiles <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_lagrange_terms, dim3(ntiles), dim3(64), 0, s, positions, reinterpret_cast<const uint4*>(tiles), num_m, den_m, den_be,
              csq);
  return (int)hipGetLastError();
}

extern "C" int RT_FN(launch_lagrange_finish)(int lpl, const uint32_t* tiles, int ntiles, const uint32_t* num_m, const uint32_t* den_m,
                                             const uint8_t* dinv_be, const uint8_t* neg, uint8_t* exps, uint8_t* flags,
                                             const modp_rt_consts* csq, hipStream_t s) {
  RT_ELSEWHERE(launch_lagrange_finish, lpl, tiles, ntiles, num_m, den_m, dinv_be, neg, exps, flags, csq, s);
  if (ntiles <= 0) return 0;
  RT_DISPATCH(lpl, k_rt_lagrange_finish, dim3(ntiles), dim3(64), 0, s, reinterpret_cast<const uint4*>(tiles), num_m, den_m, dinv_be, neg,
              exps, flags, csq);
  return (int)hipGetLastError();
}
#endif  // RT_FD_ONLY
