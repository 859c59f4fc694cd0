// Montgomery arithmetic of a RUN-TIME modulus in the "row" layout of bn_row.h: one number over the 16 lanes of a DPP row, four
// numbers per wavefront -- for the small calls of a run-time MODP group (mpvss_modp_group_*), which are the latency of one
// number's chain of products.  bn_row.h hard-codes group 14 (L = 72, 5 limb slots per lane, its N0INV); this is its
// counterpart at the three wide quad widths of bn_quad_rt.h:
//
//   handle                        quad LPL    L    row LPL   lanes x slots   tail rows (L mod row LPL)
//   256 B, 1043 .. 2048 bits         18       72      5           80                 2
//   384 B                            27      108      7          112                 3
//   512 B                            36      144      9          144                 0
//
// The limb form in HBM (L words of 29 bits) and the Montgomery domain R = 2^(29 L) are those of the quad layout: a product of
// the same operands in [0, 2N) is the same integer (a b + m N) / R, so tables, combs and results pass between the layouts as
// they lie.  Handles at 5 and 9 limbs per lane (moduli up to 1042 bits) keep the quad layout: their chains are short.
//
// Same CIOS row as bn_row.h::row_step; n0inv = -N^-1 mod 2^29 is a VGPR value (one more v_mul_lo_u32 per row, as
// bn::mont_mul<N0INV_RUNTIME> has it).  The loop over groups of LPL rows stays rolled; the rows of a group come from a
// compile-time recursion (Rows<>), so that no accumulator index is a run-time value.
//
// Column bound: a column is carried once per LPL rows and collects at most 2 LPL product units in between, in the product and
// in the squaring alike (its rows visit k >= RR only and the doubled limb counts two), each below 2^58.01: below 2^62.18 at
// LPL = 9 with the carry that came in, so no second carry at any of the three widths.  tests/test_modp_rt_row_model.py runs the
// same integer pipeline with a run-time n0inv: largest accumulator 2^60.44 / 2^60.93 / 2^61.30 at LPL 5 / 7 / 9 with every limb
// at 2^29 - 1 + 2^9, 2^61.06 / 2^61.51 / 2^61.98 with a mixed vector whose rows reach m near 2^29.
//
// Out of scope here: handles at 5 / 9 limbs per lane, the pair / MFMA layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "modp_limbs.h"

namespace bnrowrt {

using limbs::MASK;
using limbs::u32;
using limbs::u64;
using limbs::W;

constexpr int LANES = 16;
constexpr int NUMS_PER_WAVE = 4;

// row limb slots per lane of a quad width (0: the width has no row layout)
constexpr int row_lpl(int quad_lpl) { return quad_lpl == 18 ? 5 : quad_lpl == 27 ? 7 : quad_lpl == 36 ? 9 : 0; }

// LDS words of one number's operand slot: 16 lanes x LPL (words >= L are zero)
template <int LPL> struct Slot { static constexpr int WORDS = LANES * LPL; };
// the product reads one word past a slot when L is a multiple of LPL (the prefetch of a row that does not exist): the LDS
// array of a kernel is NUMS_PER_WAVE slots plus this
constexpr int LDS_PAD = 4;

constexpr int DPP_ROW_BCAST0 = 0x150;   // row_newbcast:0
constexpr int DPP_ROW_SHL1 = 0x101;     // lane l reads lane l+1 of its row (lane 15: 0)
constexpr int DPP_ROW_SHR1 = 0x111;     // lane l reads lane l-1 of its row (lane 0: 0)

__device__ __forceinline__ u32 row_bcast0(u32 v) { return (u32)__builtin_amdgcn_mov_dpp((int)v, DPP_ROW_BCAST0, 0xf, 0xf, true); }
__device__ __forceinline__ u32 row_from_next(u32 v) { return (u32)__builtin_amdgcn_mov_dpp((int)v, DPP_ROW_SHL1, 0xf, 0xf, true); }
__device__ __forceinline__ u32 row_from_prev(u32 v) { return (u32)__builtin_amdgcn_mov_dpp((int)v, DPP_ROW_SHR1, 0xf, 0xf, true); }

struct Lane {
  u32 l;         // lane index inside the row, 0..15
  u32 mask29;    // 2^29 - 1 (limbs::MASK) in a VGPR, opaque (keeps "broadcast & mask" one v_and_b32_dpp; see bn_quad.h)
};

__device__ __forceinline__ Lane make_lane() {
  Lane ln;
  ln.l = threadIdx.x & 15;
  ln.mask29 = MASK;
  asm volatile("" : "+v"(ln.mask29));
  return ln;
}

// one row of the product: T (rotated by RR: local position k lives in T[(k + RR) % LPL]) += a * bi + m * n, then retire
template <int LPL, bool SQ, int RR>
__device__ __forceinline__ void row_step(u64 (&T)[LPL], const u32 (&a)[LPL], const u32 (&n)[LPL], u32 bi, u32 n0inv, const Lane& ln) {
  if (SQ) {
    // b is a itself: row r = LPL o + RR visits only the local positions k >= RR, k > RR with the doubled limb (bn_row.h: every
    // pair of limbs is then counted exactly twice, every square once, by the same instructions in all lanes)
    const u32 bi2 = bi << 1;
#pragma unroll
    for (int k = RR; k < LPL; ++k) T[(k + RR) % LPL] += (u64)a[k] * (k > RR ? bi2 : bi);
  } else {
#pragma unroll
    for (int k = 0; k < LPL; ++k) T[(k + RR) % LPL] += (u64)a[k] * bi;
  }
  const u32 m = row_bcast0((u32)T[RR] * n0inv) & ln.mask29;
#pragma unroll
  for (int k = 0; k < LPL; ++k) T[(k + RR) % LPL] += (u64)m * n[k];
  const u64 ret = T[RR];
  T[(RR + 1) % LPL] += ret >> W;
  T[RR] = (u64)(row_from_next((u32)ret) & ln.mask29);      // lane 15 reads 0 (bound_ctrl): a fresh zero column at the top
#pragma unroll
  for (int k = 0; k < LPL; ++k) asm volatile("" : "+v"(T[k]));      // pin the row-wise order (bn_quad.h)
}

// rows RR .. END - 1 of one group: bo points at the group's first limb of b, bnext holds bo[RR] and leaves as bo[END]
template <int LPL, bool SQ, int RR, int END>
struct Rows {
  static __device__ __forceinline__ void run(u64 (&T)[LPL], const u32 (&a)[LPL], const u32 (&n)[LPL], const u32* bo, u32& bnext,
                                             u32 n0inv, const Lane& ln) {
    const u32 bi = bnext;
    bnext = bo[RR + 1];
    row_step<LPL, SQ, RR>(T, a, n, bi, n0inv, ln);
    Rows<LPL, SQ, RR + 1, END>::run(T, a, n, bo, bnext, n0inv, ln);
  }
};
template <int LPL, bool SQ, int END>
struct Rows<LPL, SQ, END, END> {
  static __device__ __forceinline__ void run(u64 (&)[LPL], const u32 (&)[LPL], const u32 (&)[LPL], const u32*, u32&, u32, const Lane&) {}
};

// r = a * b * R^-1 (mod N), R = 2^(29 L), almost normalised and < 2N when a, b < 2N.
//   a, n : this lane's LPL limb slots (registers);  b : LDS pointer to the L limbs of the second operand of THIS number (the
//   word b[L] is read and not used: Slot / LDS_PAD).  SQ: b must be (an LDS copy of) a itself.
template <int LPL, int L, bool SQ = false>
__device__ __forceinline__ void mont_mul(u32 (&r)[LPL], const u32 (&a)[LPL], const u32* __restrict__ b, const u32 (&n)[LPL], u32 n0inv,
                                         const Lane& ln) {
  constexpr int FULL_GROUPS = L / LPL, TAIL_ROWS = L % LPL;
  static_assert(L <= LANES * LPL, "a number fits the row's 16 LPL limb slots");
  u64 T[LPL];
#pragma unroll
  for (int k = 0; k < LPL; ++k) T[k] = 0;
  u32 bnext = b[0];
#pragma nounroll
  for (int o = 0; o < FULL_GROUPS; ++o) Rows<LPL, SQ, 0, LPL>::run(T, a, n, b + o * LPL, bnext, n0inv, ln);
  Rows<LPL, SQ, 0, TAIL_ROWS>::run(T, a, n, b + FULL_GROUPS * LPL, bnext, n0inv, ln);
  // local position k now lives in T[(k + TAIL_ROWS) % LPL].  Pass 1: carry-propagate inside the lane
  u64 c = 0;
#pragma unroll
  for (int k = 0; k < LPL; ++k) {
    const u64 v = T[(k + TAIL_ROWS) % LPL] + c;
    r[k] = (u32)v & MASK;
    c = v >> W;
  }
  // pass 2: the lane's carry-out (< 2^37) goes to the next lane, one more local step
  const u32 cl = row_from_prev((u32)c);
  const u32 ch = row_from_prev((u32)(c >> 32));
  const u64 v = (u64)r[0] + (((u64)ch << 32) | cl);
  r[0] = (u32)v & MASK;
  r[1] += (u32)(v >> W);
}

// ---- operand slots (16 LPL words per number) and the L-word limb form in HBM ----------------------------------------
template <int LPL>
__device__ __forceinline__ void slot_store(u32* slot, const u32 (&a)[LPL], const Lane& ln) {
#pragma unroll
  for (int k = 0; k < LPL; ++k) slot[ln.l * LPL + k] = a[k];
}

// this lane's limb slots of a number in limb form (L words; slots beyond are zero)
template <int LPL, int L>
__device__ __forceinline__ void load_lane_limbs(u32 (&a)[LPL], const u32* __restrict__ g, const Lane& ln) {
#pragma unroll
  for (int k = 0; k < LPL; ++k) {
    const int j = (int)ln.l * LPL + k;
    a[k] = j < L ? g[j < L ? j : 0] : 0u;
  }
}

template <int LPL, int L>
__device__ __forceinline__ void store_lane_limbs(u32* __restrict__ g, const u32 (&a)[LPL], const Lane& ln) {
#pragma unroll
  for (int k = 0; k < LPL; ++k) {
    const int j = (int)ln.l * LPL + k;
    if (j < L) g[j] = a[k];
  }
}

// L words global -> the number's LDS slot (words >= L zeroed): 16 lanes x LPL words
template <int LPL, int L>
__device__ __forceinline__ void slot_fill_from_global(u32* slot, const u32* __restrict__ g, const Lane& ln) {
#pragma unroll
  for (int k = 0; k < LPL; ++k) {
    const int j = (int)ln.l * LPL + k;
    slot[j] = j < L ? g[j < L ? j : 0] : 0u;
  }
}

}  // namespace bnrowrt
