// Montgomery arithmetic of a RUN-TIME modulus (any odd N of at most 4096 bits) in the quad layout of bn_quad.h:
// one number over the four lanes of a DPP quad, radix 2^29, lazy column accumulation, values kept in [0, 2N).
//
// The product, the lane and the slot helpers are bn_quad.h's own templates (one body for every width).  What is run-time here:
//   * the width: K = LPL limbs per lane, L = 4 LPL limbs, R = 2^(29 L).  The library instantiates LPL = 5, 9, 18
//     (capacities 580, 1044, 2088 bits); a modulus takes the smallest width with bits(N) <= 29 L - 2, so that R > 4N keeps
//     the lazy [0, 2N) invariant with no conditional subtraction inside a chain.  LPL = 27 (3132 bits) is the wide width:
//     a group of 384-byte elements and scalars (moduli of 2049 .. 3072 bits) always runs at it, and one of 512-byte
//     elements and scalars (3073 .. 4096 bits) at LPL = 36 (4176 bits).
//   * n0inv = -N^-1 mod 2^29 is an argument (bn::mont_mul<N0INV_RUNTIME>: a VGPR value, one more v_mul_lo_u32 per row).
//   * a 2048-bit input enters a narrower width by a product of OUTER = IN_ROWS / LPL > 4 groups of rows (rt_to_mont): one
//     long product with a host constant reduces it mod N and converts it to Montgomery form at once.
//
// Column bound: every column passes the lowest position of its lane every LPL rows and is carried there, so it collects
// at most 2 LPL products < 2^58.01 between two carries, however many rows there are -- 36 at LPL = 18 as in bn_quad.h, fewer below
// (tests/test_modp_rt_model.py checks this for each instantiated width with worst-case limbs and a run-time n0inv).  At
// LPL = 27 that is 54 products, 54 (2^29 - 1 + 2^9)^2 < 2^63.76, the last width that fits: 72 products at LPL = 36 (4096 bits)
// pass 2^64 (tests/test_modp_rt_wide_model.py), so at LPL = 36 bn::mont_mul carries a column a second time, half way down its
// lane (`if constexpr (K > 27)`): tests/test_modp_rt_4096_model.py has the bound with that carry, DESIGN section 13 the count.
#pragma once
#include "bn_quad.h"

namespace bnrt {

using bn::Lane;
using bn::load_lane_limbs;
using bn::make_lane;
using bn::MASK;
using bn::mont_mul;
using bn::N0INV_RUNTIME;
using bn::slot_fill_from_global;
using bn::slot_load;
using bn::slot_store;
using bn::store_lane_limbs;
using bn::u32;
using bn::u64;
using bn::W;

// the width's constants; EB: bytes of an element or scalar on the ABI of a group of this width; IN_ROWS: rows of the long
// product that takes a whole EB-byte input (its limbs, padded to a multiple of LPL so that the accumulators end where they
// started: 75, 72, 72 and, at 27 and 36 limbs per lane, 108 and 144 = L, a plain product with R^2 mod N); COMB_ROWS: 4-bit windows of an exponent;
// KS_ROWS: 256-bit rows of an exponent (the rows of a key set)
template <int LPL>
struct Width {
  static constexpr int L = 4 * LPL;
  static constexpr int EB = LPL == 36 ? 512 : LPL == 27 ? 384 : 256;
  static constexpr int IN_ROWS = LPL * (((8 * EB + 28) / 29 + LPL - 1) / LPL);
  static constexpr int COMB_ROWS = 2 * EB;
  static constexpr int KS_ROWS = EB / 32;
  static constexpr int SLOT = ((IN_ROWS > L ? IN_ROWS : L) + 3) & ~3;   // LDS words of one operand slot (16-byte multiple)
  static constexpr int CAP_BITS = 29 * L - 2;                            // largest modulus this width takes
};

}  // namespace bnrt
