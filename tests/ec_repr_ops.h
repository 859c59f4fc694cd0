// Test infrastructure, never shipped: the one-lane point operations of mpvss_rs_amd/csrc/ec_curves.h on operands given as
// RAW LIMB WORDS (30 / 40 per point, any representative), results as canonical encodings.  One body for the CPU
// (tests/ec_host_shim.cpp) and the GPU (tests/ec_repr_unit.hip); the cases and the expected bytes are those of
// tests/ec_repr_cases.py.
//
// repr_pair<C>(P, Q, out): REPR_SLOTS encodings of C::ENC_LEN bytes, P = a G, Q = b G
//    0  add(P, Q)                              (a + b) G
//    1  dbl(P)                                 2a G
//    2  neg(P)                                 -a G
//    3  add_affine(P, +A)   4  add_affine(P, -A)     A = to_affine(Q) packed and unpacked as the combs hold it; an
//                                              identity Q (ks_is_identity) has no affine form: A is the generator's then
//    5  add_cached(P, +to_cached(Q))   6  add_cached(P, -to_cached(Q))
//    7  cmov(r = P, Q, true)           8  cmov(r = P, Q, false)       b G, a G: encode of the operands themselves
//    9  acc = P; 64 steps of acc += Q (even steps) / acc = 2 acc (odd steps): results fed back in as operands
//   10  byte 0: ks_is_identity(P) | ks_is_identity(Q) << 1, the rest zero
#pragma once
#include "../mpvss_rs_amd/csrc/ec_keyset.h"

#if defined(__HIPCC__)
#define REPR_FN __host__ __device__ __noinline__
#else
#define REPR_FN __attribute__((noinline))
#endif

namespace ec {

constexpr int REPR_SLOTS = 11;
constexpr int REPR_CLOSURE_STEPS = 64;

template <class C>
REPR_FN void repr_encode(uint8_t* out, const typename C::Point& p) {
  C::encode(out, p);
}
template <class C>
REPR_FN void repr_add(typename C::Point& r, const typename C::Point& p, const typename C::Point& q) {
  C::add(r, p, q);
}
template <class C>
REPR_FN void repr_dbl(typename C::Point& r, const typename C::Point& p) {
  C::dbl(r, p);
}

template <class C>
REPR_FN void repr_pair(const u32* pw, const u32* qw, uint8_t* out) {
  constexpr int L = C::ENC_LEN;
  typename C::Point P, Q, r;
  ks_load_point<C>(P, pw);
  ks_load_point<C>(Q, qw);
  repr_add<C>(r, P, Q);
  repr_encode<C>(out + 0 * L, r);
  repr_dbl<C>(r, P);
  repr_encode<C>(out + 1 * L, r);
  C::neg(r, P);
  repr_encode<C>(out + 2 * L, r);
  const bool p_id = ks_is_identity(P), q_id = ks_is_identity(Q);
  {
    typename C::Point base = Q, g;
    C::generator(g);
    C::cmov(base, g, q_id);
    typename C::Affine A, B;
    u32 packed[C::AFFINE_PACKED_WORDS];
    C::to_affine(A, base);
    C::pack_affine(packed, A);
    C::unpack_affine(B, packed);
    C::add_affine(r, P, B, false);
    repr_encode<C>(out + 3 * L, r);
    C::add_affine(r, P, B, true);
    repr_encode<C>(out + 4 * L, r);
  }
  {
    typename C::Cached cq;
    C::to_cached(cq, Q);
    C::add_cached(r, P, cq, false);
    repr_encode<C>(out + 5 * L, r);
    C::add_cached(r, P, cq, true);
    repr_encode<C>(out + 6 * L, r);
  }
  r = P;
  C::cmov(r, Q, true);
  repr_encode<C>(out + 7 * L, r);
  r = P;
  C::cmov(r, Q, false);
  repr_encode<C>(out + 8 * L, r);
  r = P;
  for (int s = 0; s < REPR_CLOSURE_STEPS; ++s) {
    typename C::Point t;
    if (s % 2 == 0) repr_add<C>(t, r, Q); else repr_dbl<C>(t, r);
    r = t;
  }
  repr_encode<C>(out + 9 * L, r);
  for (int i = 0; i < L; ++i) out[10 * L + i] = 0;
  out[10 * L] = (uint8_t)((p_id ? 1 : 0) | (q_id ? 2 : 0));
}

// secp256k1's encode_batch<8>: eight points as raw limb words (8 x 30) -> 8 x 33 bytes
REPR_FN void repr_batch8(const u32* pts, uint8_t* out) {
  Secp::encode_batch<8>(
      out, 33, [&](int i, Secp::Point& q) { ks_load_point<Secp>(q, pts + 30 * i); }, [&](int) { return true; });
}

}  // namespace ec
