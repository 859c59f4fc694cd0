// The limb form of the MODP layouts and its byte edge, written once for the quad (bn_quad.h), pair (bn_pair.h), row
// (bn_row.h) and run-time (bn_quad_rt.h) layouts: a number is L limbs of radix 2^29, least significant first, in HBM and
// in an LDS operand slot alike; on the ABI it is 256 big-endian bytes.
//
// Plain C++ (host + device): tests/limbs_host_shim.cpp runs the same code on the CPU against Python integers
// (tests/test_limbs_host.py).  What is per layout -- which lane runs the serial pass, which lane emits which word, the
// barriers around them -- stays with the layout's kernels.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LIMBS_HD __host__ __device__ __forceinline__
#else
#define LIMBS_HD inline
#endif

namespace limbs {

typedef uint32_t u32;
typedef uint64_t u64;

constexpr int W = 29;                // bits per limb
constexpr int L = 72;                // limbs of a 2048-bit number (capacity 2088 bits, R = 2^2088)
constexpr u32 MASK = (1u << W) - 1;

// device-resident constants of a fixed 2048-bit modulus: N, R^2 mod N, R mod N (Montgomery one), plain 1
struct ModpConsts {
  u32 n[L];
  u32 r2[L];
  u32 one_m[L];
  u32 one[L];
};

// limb j (W bits at bit offset W j) of an EB-byte big-endian integer; 0 above bit 8 EB - 1.  EB = 256 on every ABI but that
// of the wider run-time groups (bn_quad_rt.h, 384 and 512 bytes).
template <int EB>
LIMBS_HD u32 be_limb(const uint8_t* __restrict__ be, int j) {
  const int o = W * j;
  const int p = o >> 3, s = o & 7;
  u64 w = 0;
#pragma unroll
  for (int t = 0; t < 5; ++t) {                // W + 7 <= 40 bits
    const int idx = EB - 1 - (p + t);
    if (idx >= 0) w |= (u64)be[idx] << (8 * t);
  }
  return (u32)(w >> s) & MASK;
}
LIMBS_HD u32 be256_limb(const uint8_t* __restrict__ be, int j) { return be_limb<256>(be, j); }

// Geometry of a rows-by-windows table of one base y: table[j][d] = y^(d 2^(B j)), j < R rows of B bits, d < 2^W -- y^e for a
// 2048-bit e is then the product over the rows of R B-bit exponentiations that share one chain of TOP squarings.  The registered
// key tables are RowGeom<8, 256, 7>, the call tables RowGeom<8, 256, 5>; every kernel that builds or reads such a table takes
// its sizes and its digits from here.
template <int R_, int B_, int W_>
struct RowGeom {
  static_assert(R_ * B_ == 2048 && W_ >= 1 && W_ <= 8, "rows of a 2048-bit exponent, windows within two bytes");
  static constexpr int R = R_, B = B_, WIN = W_;
  static constexpr int ENT = 1 << WIN;                       // entries per row
  static constexpr int NWIN = (B + WIN - 1) / WIN;           // windows per row (the top one holds B - TOP bits)
  static constexpr int TOP = WIN * (NWIN - 1);               // weight of a row's top window
  static constexpr unsigned long long KEY_WORDS = (unsigned long long)R * ENT * L;
  // window w of row j of the 256-byte big-endian e: bits [B j + WIN w, B j + WIN w + WIN) of e, without the bits of row j + 1
  static LIMBS_HD u32 digit(const uint8_t* __restrict__ e, int j, int w) {
    const int g = B * j + WIN * w, b = g >> 3;
    const u32 lo = e[255 - b];
    const u32 hi = (b + 1 < 256) ? e[254 - b] : 0u;
    const int top = B - WIN * w;                             // bits of this window that belong to the row
    return ((lo | (hi << 8)) >> (g & 7)) & (u32)((1 << (top < WIN ? top : WIN)) - 1);
  }
};

// Almost-normalised value < 2N in a slot of LIMBS limbs (every limb <= 2^W - 1 + 2^9) -> its canonical residue in
// [0, N), exact limbs.  Serial: ONE lane of the number runs it, between two barriers.
// lift_parity 0 / 1 (scalar ring, n = the limbs of q'): the residue v in [0, q') is lifted to the number in
// [0, 2q') = [0, q-1) of that parity, v or v + q' (Chinese remainders; q' is odd).
template <int LIMBS>
LIMBS_HD void slot_canonicalize(u32* slot, const u32* __restrict__ n, int lift_parity = -1) {
  // exact carry propagation
  u32 c = 0;
#pragma nounroll
  for (int j = 0; j < LIMBS; ++j) {
    const u32 v = slot[j] + c;
    slot[j] = v & MASK;
    c = v >> W;
  }
  // value < 2N: subtract N once if value >= N
  int ge = 1;  // value >= N ?  (decided by the most significant differing limb)
#pragma nounroll
  for (int j = LIMBS - 1; j >= 0; --j) {
    const u32 x = slot[j], y = n[j];
    if (x != y) { ge = x > y; break; }
  }
  if (ge) {
    u32 borrow = 0;
#pragma nounroll
    for (int j = 0; j < LIMBS; ++j) {
      const u32 d = slot[j] - n[j] - borrow;
      borrow = (d >> 31) & 1;  // operands < 2^W, so a wrap sets the top bit
      slot[j] = d & MASK;
    }
  }
  if (lift_parity >= 0 && (int)(slot[0] & 1u) != lift_parity) {
    u32 carry = 0;
#pragma nounroll
    for (int j = 0; j < LIMBS; ++j) {
      const u32 v = slot[j] + n[j] + carry;
      slot[j] = v & MASK;
      carry = v >> W;
    }
  }
}

// little-endian 32-bit word wd (0 .. EB/4 - 1) of the EB-byte number in a slot of LIMBS exact limbs (limbs >= LIMBS are zero).
// The ABI's byte order puts it, byte-swapped, at the mirrored position: out32[EB/4 - 1 - wd] = bswap32(word).
template <int LIMBS, int EB = 256>
LIMBS_HD u32 slot_word32(const u32* slot, int wd) {
  const int bit = 32 * wd;
  const int j = bit / W, s = bit % W;
  u32 v = 0;
  if (LIMBS * W >= 8 * EB || j < LIMBS) {
    // 32 bits starting at bit s of limb j: up to three limbs (s + 32 can exceed 2 W)
    u64 two = (u64)slot[j] | ((u64)(j + 1 < LIMBS ? slot[j + 1] : 0u) << W);
    two >>= s;
    if (2 * W - s < 32) two |= (u64)(j + 2 < LIMBS ? slot[j + 2] : 0u) << (2 * W - s);
    v = (u32)two;
  }
  return v;
}

}  // namespace limbs
