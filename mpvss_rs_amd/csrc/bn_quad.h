// 2048-bit Montgomery arithmetic for gfx950, "quad" layout: one number is spread over the
// four lanes of a DPP quad (16 numbers per 64-lane wavefront).
//
// Representation
//   radix 2^29, L = 72 limbs (capacity 2088 bits, R = 2^2088), lane q of the quad owns limbs
//   18q .. 18q+17 in registers.  Limbs are "almost normalised": every limb <= 2^29 - 1 + 2^9.
//   Values are kept in [0, 2N) (R > 4N, so no conditional subtraction inside a chain).
//
// Why this shape (measured on MI355X, profiles/r01_ubench_valu_issue_rates.txt):
//   * v_mad_u64_u32 issues at one wave-instruction per ~2.07 ns per SIMD, but a carry-producing add
//     (v_add_co/v_addc) costs the same, so a radix-2^32 schoolbook row (1 mad + 1 addc per product) is
//     ~1.85x the cost of a row whose products are accumulated carry-free in 64-bit column accumulators
//     (1 mad per product).  The radix is the largest for which that works: every column passes the lowest
//     position of a lane every 18 rows and is carried there, so it collects at most 36 products < 2^58 in
//     between (< 2^63.2, tests/test_limb_model.py); 2^30 would overflow.
//   * a whole 2048-bit operand per lane (64+ VGPRs per operand, 3-4 live) does not fit 3 waves per SIMD,
//     a quarter of one (18 limbs) does.
//   * quad_perm DPP moves data between the four lanes at full VALU rate (no LDS round trip).
//
// Montgomery product (CIOS, one b-limb per step, accumulators shift one limb per step):
//   the second operand is read limb by limb from LDS (all four lanes read the same word ->
//   broadcast, 16 distinct banks per half-wave -> conflict free).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "modp_limbs.h"

namespace bn {

using limbs::L;
using limbs::MASK;
using limbs::u32;
using limbs::u64;
using limbs::W;

constexpr int LPL = 18;              // limbs per lane
constexpr int NUMS_PER_WAVE = 16;
constexpr int SLOT_WORDS = 72;       // LDS words per number operand slot (288 B = 18 x 16 B)

// quad_perm selectors: dpp_ctrl = p0 | p1<<2 | p2<<4 | p3<<6
constexpr int QP_BCAST0 = 0x00;                          // every lane reads lane 0
constexpr int QP_DOWN = 1 | (2 << 2) | (3 << 4) | (3 << 6);  // lane q reads lane q+1 (lane 3 reads itself)
constexpr int QP_UP = 0 | (0 << 2) | (1 << 4) | (2 << 6);    // lane q reads lane q-1 (lane 0 reads itself)

__device__ __forceinline__ u32 quad_bcast0(u32 v) {
  return (u32)__builtin_amdgcn_mov_dpp((int)v, QP_BCAST0, 0xf, 0xf, true);
}
__device__ __forceinline__ u32 quad_from_next(u32 v) {
  return (u32)__builtin_amdgcn_mov_dpp((int)v, QP_DOWN, 0xf, 0xf, true);
}
__device__ __forceinline__ u32 quad_from_prev(u32 v) {
  return (u32)__builtin_amdgcn_mov_dpp((int)v, QP_UP, 0xf, 0xf, true);
}

struct Lane {
  u32 q;         // lane index inside the quad, 0..3
  u32 not_top;   // all ones unless q == 3
  u32 top28;     // 2^W - 1 unless q == 3 (then 0): "take the low limb of the lane above"
  u32 low01;     // 1 iff q == 0, else 0
  u32 not_low;   // all ones unless q == 0
  u32 mask28;    // 2^W - 1 in a VGPR (lets the compiler fuse "broadcast & mask" into one v_and_b32_dpp)
  u32 one;       // 1 in a VGPR, opaque: "x * one" stays a v_mad_u64_u32 (a 64-bit add would be two carry instructions)
  u32 eight;     // 8 likewise: "hi * eight" must not become a 64-bit shift-and-add
};

__device__ __forceinline__ Lane make_lane() {
  Lane ln;
  ln.q = threadIdx.x & 3;
  ln.not_top = (ln.q != 3) ? 0xffffffffu : 0u;
  ln.top28 = (ln.q != 3) ? MASK : 0u;
  ln.low01 = (ln.q == 0) ? 1u : 0u;
  ln.not_low = (ln.q != 0) ? 0xffffffffu : 0u;
  // Opaque to the optimiser: otherwise `x & mask` becomes v_cndmask_b32 on an SGPR-pair condition,
  // which issues ~4x slower than v_and_b32 on gfx950 (profiles/r01_ubench_valu_issue_rates.txt).
  ln.mask28 = MASK;
  ln.one = 1u;
  ln.eight = 8u;
  asm volatile("" : "+v"(ln.not_top), "+v"(ln.top28), "+v"(ln.low01), "+v"(ln.not_low), "+v"(ln.mask28), "+v"(ln.one),
               "+v"(ln.eight));
  return ln;
}

// r = a * b * R^-1 (mod N), R = 2^(29 * 4 K); result almost normalised and < 2N when a, b < 2N.
//   a     : this lane's K limbs of the first operand (registers); K = 18 for a 2048-bit number, bn_quad_rt.h adds 5, 9, 27 and 36
//   b     : LDS pointer to the limbs of the second operand of THIS number (a slot of at least 4 K words)
//   n     : this lane's K limbs of the modulus (registers)
//   N0INV : -N^-1 mod 2^29 when the modulus is a compile-time one; 1 for the RFC 3526 prime (N = -1 mod 2^64), the multiply
//           folds away.  N0INV_RUNTIME: the value comes as the last argument (a VGPR), one more v_mul_lo_u32 per row.
//
// One step (one limb b_i of b), per lane: K mads a[k]*b_i, m from lane 0's lowest column,
// K mads m*n[k]; lane 0's lowest column is then 0 mod 2^29 and retires.  Every lane carries the upper bits
// of its lowest column into its next column and hands the low 29 bits to the lane below (lane 3 starts a
// fresh zero column).  Column accumulators stay below 2^64 (at most K steps x 2 products < 2^58.01 between two
// carries of a column, whatever OUTER is; checked for worst-case limbs in tests/test_limb_model.py and, for every
// instantiated width with a run-time n0inv, in tests/test_modp_rt_model.py).
//
// SQ = true: b must be (an LDS copy of) a itself.  Row r = K o + rr then only visits the local positions k >= rr:
// k > rr with the doubled limb 2 a_r, k == rr with a_r itself.  Every pair {r, j}, r != j, is then counted exactly
// twice -- once doubled in the row of the limb with the smaller local index, or once in each of the two rows when the
// local indices are equal -- and every square once, in all four lanes by the same instructions: 9.5 instead of 18
// mads per row for the a*a half, 24 % fewer mads per squaring.  (Needs an even number of limbs per lane only in
// the sense that the rule is lane-independent; bounds: tests/test_limb_model.py.)
// OUTER: the product has K OUTER rows and divides by 2^(29 K OUTER), result < N + a b / 2^(29 K OUTER).
//   OUTER < 4: only the low K OUTER limbs of b take part -- the scalar-ring kernels multiply by small numbers this way (a
//              quarter of a product per Horner step);
//   OUTER > 4: b has K OUTER limbs, which is how a 2048-bit input enters a narrower width (bn_quad_rt.h).
constexpr u32 N0INV_RUNTIME = 0;     // (an n0inv is odd)
template <u32 N0INV, bool SQ = false, int OUTER = 4, int K>
__device__ __forceinline__ void mont_mul(u32 (&r)[K], const u32 (&a)[K], const u32* __restrict__ b, const u32 (&n)[K],
                                         const Lane& ln, u32 n0inv = N0INV) {
  static_assert(!SQ || OUTER == 4, "a squaring has 4 K rows");
  constexpr int B_LAST = (OUTER > 4 ? OUTER : 4) * K - 1;   // the prefetch stays inside the slot
  u64 T[K];
#pragma unroll
  for (int k = 0; k < K; ++k) T[k] = 0;
  u32 bnext = b[0];   // software prefetch of the next b limb (one LDS read in flight)
#pragma nounroll
  for (int o = 0; o < OUTER; ++o) {
#pragma unroll
    for (int rr = 0; rr < K; ++rr) {
      // local position k lives in T[(k + rr) % K]
      const u32 bi = bnext;
      {
        const int nxt = o * K + rr + 1;
        bnext = b[nxt <= B_LAST ? nxt : B_LAST];
      }
      if (SQ) {
        const u32 bi2 = bi << 1;
#pragma unroll
        for (int k = rr; k < K; ++k) T[(k + rr) % K] += (u64)a[k] * (k > rr ? bi2 : bi);
      } else {
#pragma unroll
        for (int k = 0; k < K; ++k) T[(k + rr) % K] += (u64)a[k] * bi;
      }
      const u32 m = quad_bcast0((u32)T[rr] * (N0INV != N0INV_RUNTIME ? N0INV : n0inv)) & ln.mask28;
#pragma unroll
      for (int k = 0; k < K; ++k) T[(k + rr) % K] += (u64)m * n[k];
      // K > 27 (bn_quad_rt.h, 36 limbs per lane): 2 K products pass 2^64, so a column is also carried half way down the lane.
      // The column at local position K / 2 moves its upper bits into the column above it (same weight) and keeps its low
      // W bits: between two carries a column then collects at most 36 products and two carry-ins in a product, and in a
      // squaring, whose doubled limbs fall unevenly over a column's life, at most 54 products' worth -- the bound of K = 27
      // (tests/test_modp_rt_4096_model.py).  In-lane, compile-time indices under the full unroll; no narrower instantiation
      // sees it.
      if constexpr (K > 27) {
        const u64 mid = T[(K / 2 + rr) % K];
        T[(K / 2 + 1 + rr) % K] += mid >> W;
        T[(K / 2 + rr) % K] = (u64)((u32)mid & MASK);
      }
      // Every lane moves the upper bits of its lowest column into its next column (same weight) and hands the
      // low 28 bits to the lane below, whose fresh top column they become; lane 0's lowest column is 0 mod 2^W
      // by construction and retires.  No lane-dependent arithmetic: one shift, one 64-bit add, one v_and_b32_dpp.
      {
        const u64 ret = T[rr];
        T[(rr + 1) % K] += ret >> W;
        T[rr] = (u64)(quad_from_next((u32)ret) & ln.top28);
      }
      // Pin the row-wise order: without this LLVM reassociates the 19-fold unrolled body into a
      // column-wise (product-scanning) form that keeps every b_i and m_i of the block live and
      // no longer fits 128 VGPRs (4 waves/SIMD).  The empty asm makes each accumulator opaque.
#ifndef MODP_NO_PIN
#pragma unroll
      for (int k = 0; k < K; ++k) asm volatile("" : "+v"(T[k]));
#endif
    }
  }
  // whole groups of K rows, so local position k is back in T[k].
  // pass 1: carry-propagate inside the lane
  u64 c = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const u64 v = T[k] + c;
    r[k] = (u32)v & MASK;
    c = v >> W;
  }
  // pass 2: hand the lane's carry-out (< 2^37, at K = 36 too: tests/test_modp_rt_4096_model.py) to the next lane, one more local step
  const u32 cl = quad_from_prev((u32)c) & ln.not_low;
  const u32 ch = quad_from_prev((u32)(c >> 32)) & ln.not_low;
  const u64 v = (u64)r[0] + (((u64)ch << 32) | cl);
  r[0] = (u32)v & MASK;
  r[1] += (u32)(v >> W);
}

// r = a^2 R^-1 (mod N); `self` = LDS slot holding a copy of a
template <u32 N0INV>
__device__ __forceinline__ void mont_sqr(u32 (&r)[LPL], const u32 (&a)[LPL], const u32* __restrict__ self,
                                         const u32 (&n)[LPL], const Lane& ln) {
  mont_mul<N0INV, true>(r, a, self, n, ln);
}

// ---- lane and operand slot helpers (one wave = 16 numbers; K limbs per lane, 4 K words per number) -------------

// this lane's K limbs of a number in global memory
template <int K>
__device__ __forceinline__ void load_lane_limbs(u32 (&a)[K], const u32* __restrict__ g, const Lane& ln) {
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = g[ln.q * K + k];
}

template <int K>
__device__ __forceinline__ void store_lane_limbs(u32* __restrict__ g, const u32 (&a)[K], const Lane& ln) {
#pragma unroll
  for (int k = 0; k < K; ++k) g[ln.q * K + k] = a[k];
}

// store this lane's K limbs into the number's LDS slot
template <int K>
__device__ __forceinline__ void slot_store(u32* slot, const u32 (&a)[K], const Lane& ln) {
#pragma unroll
  for (int k = 0; k < K; ++k) slot[ln.q * K + k] = a[k];
}

template <int K>
__device__ __forceinline__ void slot_load(u32 (&a)[K], const u32* slot, const Lane& ln) {
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = slot[ln.q * K + k];
}

// copy the 4 K words of a number global -> LDS slot with 16-byte accesses: chunk c (0 .. K-1) is handled by lane c & 3
template <int K = LPL>
__device__ __forceinline__ void slot_fill_from_global(u32* slot, const u32* __restrict__ g, const Lane& ln) {
  const uint4* g4 = reinterpret_cast<const uint4*>(g);
  uint4* s4 = reinterpret_cast<uint4*>(slot);
#pragma unroll
  for (int c = 0; c < (K + 3) / 4; ++c) {
    const int idx = c * 4 + (int)ln.q;
    if (idx < K) s4[idx] = g4[idx];
  }
}

}  // namespace bn
