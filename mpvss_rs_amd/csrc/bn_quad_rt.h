// Montgomery arithmetic of a RUN-TIME modulus (any odd N of at most 2086 bits) in the quad layout of bn_quad.h:
// one number over the four lanes of a DPP quad, radix 2^29, lazy column accumulation, values kept in [0, 2N).
//
// What differs from bn_quad.h (which stays the RFC 3526 group-14 product):
//   * the width is a template parameter: LPL limbs per lane, L = 4 LPL limbs, R = 2^(29 L).  The library instantiates
//     LPL = 5, 9, 18 (capacities 580, 1044, 2088 bits); a modulus takes the smallest width with bits(N) <= 29 L - 2, so
//     that R > 4N keeps the lazy [0, 2N) invariant with no conditional subtraction inside a chain.
//   * n0inv = -N^-1 mod 2^29 is an argument (a VGPR value), not a template constant: one more v_mul_lo_u32 per row.
//   * the number of rows is a template parameter too: ROWS > L multiplies by a b of ROWS limbs and divides by
//     2^(29 ROWS).  That is how a 2048-bit input enters a narrower width (rt_to_mont): one long product with a host
//     constant reduces it mod N and converts it to Montgomery form at once.
//
// Column bound: every column passes the lowest position of its lane every LPL rows and is carried there, so it collects
// at most 2 LPL products < 2^58.01 between two carries, whatever ROWS is -- 36 at LPL = 18 as in bn_quad.h, fewer below
// (tests/test_modp_rt_model.py checks this for each instantiated width with worst-case limbs and a run-time n0inv).
#pragma once
#include "bn_quad.h"

namespace bnrt {

using bn::Lane;
using bn::make_lane;
using bn::MASK;
using bn::u32;
using bn::u64;
using bn::W;

// the width's constants; IN_ROWS: rows of the long product that takes a whole 2048-bit input (72 limbs, padded to a
// multiple of LPL so that the accumulators end where they started)
template <int LPL>
struct Width {
  static constexpr int L = 4 * LPL;
  static constexpr int IN_ROWS = LPL * ((72 + LPL - 1) / LPL);
  static constexpr int SLOT = ((IN_ROWS > L ? IN_ROWS : L) + 3) & ~3;   // LDS words of one operand slot (16-byte multiple)
  static constexpr int CAP_BITS = 29 * L - 2;                            // largest modulus this width takes
};

// r = a * b * 2^(-29 ROWS) (mod N), almost normalised, < N + a b / 2^(29 ROWS) (< 2N for a, b < 2N and ROWS = L).
//   a : this lane's LPL limbs (registers);  b : LDS, ROWS limbs of THIS number;  n : this lane's LPL limbs of N
// Same step as bn::mont_mul: LPL mads a[k] b_i, m from lane 0's lowest column, LPL mads m n[k], retire / hand down.
// SQ: b is a copy of a (ROWS == L), the a*a half visits only local positions k >= rr (bn_quad.h explains the count).
template <int LPL, bool SQ = false, int ROWS = 4 * LPL>
__device__ __forceinline__ void mont_mul(u32 (&r)[LPL], const u32 (&a)[LPL], const u32* __restrict__ b, const u32 (&n)[LPL],
                                         u32 n0inv, const Lane& ln) {
  static_assert(ROWS % LPL == 0, "the accumulators must end where they started");
  static_assert(!SQ || ROWS == 4 * LPL, "a squaring has L rows");
  u64 T[LPL];
#pragma unroll
  for (int k = 0; k < LPL; ++k) T[k] = 0;
  u32 bnext = b[0];
#pragma nounroll
  for (int o = 0; o < ROWS / LPL; ++o) {
#pragma unroll
    for (int rr = 0; rr < LPL; ++rr) {
      const u32 bi = bnext;
      {
        const int nxt = o * LPL + rr + 1;
        bnext = b[nxt < ROWS ? nxt : ROWS - 1];
      }
      if (SQ) {
        const u32 bi2 = bi << 1;
#pragma unroll
        for (int k = rr; k < LPL; ++k) T[(k + rr) % LPL] += (u64)a[k] * (k > rr ? bi2 : bi);
      } else {
#pragma unroll
        for (int k = 0; k < LPL; ++k) T[(k + rr) % LPL] += (u64)a[k] * bi;
      }
      const u32 m = bn::quad_bcast0((u32)T[rr] * n0inv) & ln.mask28;
#pragma unroll
      for (int k = 0; k < LPL; ++k) T[(k + rr) % LPL] += (u64)m * n[k];
      {
        const u64 ret = T[rr];
        T[(rr + 1) % LPL] += ret >> W;
        T[rr] = (u64)(bn::quad_from_next((u32)ret) & ln.top28);
      }
      // keep the row-wise order (see bn_quad.h: otherwise LLVM turns the unrolled body column-wise and runs out of VGPRs)
#pragma unroll
      for (int k = 0; k < LPL; ++k) asm volatile("" : "+v"(T[k]));
    }
  }
  u64 c = 0;
#pragma unroll
  for (int k = 0; k < LPL; ++k) {
    const u64 v = T[k] + c;
    r[k] = (u32)v & MASK;
    c = v >> W;
  }
  const u32 cl = bn::quad_from_prev((u32)c) & ln.not_low;
  const u32 ch = bn::quad_from_prev((u32)(c >> 32)) & ln.not_low;
  const u64 v = (u64)r[0] + (((u64)ch << 32) | cl);
  r[0] = (u32)v & MASK;
  r[1] += (u32)(v >> W);
}

template <int LPL>
__device__ __forceinline__ void slot_store(u32* slot, const u32 (&a)[LPL], const Lane& ln) {
#pragma unroll
  for (int k = 0; k < LPL; ++k) slot[ln.q * LPL + k] = a[k];
}

template <int LPL>
__device__ __forceinline__ void lane_load(u32 (&a)[LPL], const u32* __restrict__ g, const Lane& ln) {
#pragma unroll
  for (int k = 0; k < LPL; ++k) a[k] = g[ln.q * LPL + k];
}

template <int LPL>
__device__ __forceinline__ void lane_store(u32* __restrict__ g, const u32 (&a)[LPL], const Lane& ln) {
#pragma unroll
  for (int k = 0; k < LPL; ++k) g[ln.q * LPL + k] = a[k];
}

// L words global -> LDS slot with 16-byte accesses (L is a multiple of 4), chunk c by lane c & 3
template <int LPL>
__device__ __forceinline__ void slot_fill(u32* slot, const u32* __restrict__ g, const Lane& ln) {
  constexpr int CH = 4 * LPL / 4;   // 16-byte chunks of a number
  const uint4* g4 = reinterpret_cast<const uint4*>(g);
  uint4* s4 = reinterpret_cast<uint4*>(slot);
#pragma unroll
  for (int c = 0; c < (CH + 3) / 4; ++c) {
    const int idx = c * 4 + (int)ln.q;
    if (idx < CH) s4[idx] = g4[idx];
  }
}

}  // namespace bnrt
