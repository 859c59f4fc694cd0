// Key sets of a curve group: the generator's fixed-base comb (ec_kernels.hip), built per public key and kept in HBM.
//   rows[key][w][i] = (i + 1) * 16^w * y_key,  w < 65, i < 8,  packed affine entries in the comb's own packing and order,
// so k * y costs one mixed addition per window and no doublings (dleq.rs:214-216 a2 = w y, participant.rs:1190 Y = P(i) y).
// The bodies are plain C++ (host + device): tests/ec_keyset_host_shim.cpp compiles them for the CPU.
//
// The identity is a valid key (33 / 32 zero bytes) and has no affine form on secp256k1, so a key carries a mark: a marked
// key's rows hold the GENERATOR's multiples (valid entries nobody uses) and the walk hands out the identity for it.
// ristretto255 could walk the identity's rows as they are ((1, 1, 0) is its affine Niels form); it follows the same rule
// so that both curves run one body.
#pragma once
#include "ec_curves.h"

namespace ec {

constexpr int KS_WINDOWS = 65;
constexpr int KS_ENTRIES = 8;

template <class C>
struct KeysetGeom {
  static constexpr int ENTRY_WORDS = C::AFFINE_PACKED_WORDS;                 // 16 / 24
  static constexpr int WINDOW_WORDS = KS_ENTRIES * ENTRY_WORDS;              // 128 / 192: a projective point (30 / 40 words) fits
  static constexpr int ROW_WORDS = KS_WINDOWS * WINDOW_WORDS;                // 8 320 / 12 480 words = 33 280 / 49 920 bytes
  static_assert(C::POINT_WORDS <= WINDOW_WORDS, "the build parks a window's base at the head of the window");
};

template <class C>
EC_HD void ks_load_point(typename C::Point& p, const u32* src) {
  u32* w = reinterpret_cast<u32*>(&p);
#pragma unroll
  for (int i = 0; i < C::POINT_WORDS; ++i) w[i] = src[i];
}
template <class C>
EC_HD void ks_store_point(u32* dst, const typename C::Point& p) {
  const u32* w = reinterpret_cast<const u32*>(&p);
#pragma unroll
  for (int i = 0; i < C::POINT_WORDS; ++i) dst[i] = w[i];
}

// is a decoded point the identity (of its encoding: ristretto255's decoder yields x = 0 for the zero encoding alone)
EC_HD bool ks_is_identity(const Secp::Point& p) { return Secp::Fp::is_zero(p.Z); }
EC_HD bool ks_is_identity(const Ristretto::Point& p) { return Ristretto::Fp::is_zero(p.X); }

// affine entry of m from 1 / Z (the values of C::to_affine, without its inversion)
EC_HD void ks_affine_from_zinv(Secp::Affine& r, const Secp::Point& m, const Fe& zi) {
  typedef Secp::Fp Fp;
  Fp::mul(r.x, m.X, zi);
  Fp::mul(r.y, m.Y, zi);
  Fp::canon(r.x);
  Fp::canon(r.y);
}
EC_HD void ks_affine_from_zinv(Ristretto::Affine& r, const Ristretto::Point& m, const Fe& zi) {
  typedef Ristretto::Fp Fp;
  const Fe d2 = {EC_ED_2D_INIT};
  Fe x, y, t;
  Fp::mul(x, m.X, zi);
  Fp::mul(y, m.Y, zi);
  Fp::addc(r.ypx, y, x);
  Fp::sub(r.ymx, y, x);
  Fp::mul(t, x, y);
  Fp::mul(r.xy2d, t, d2);
  Fp::canon(r.ypx);
  Fp::canon(r.ymx);
  Fp::canon(r.xy2d);
}

// ---- build, first pass: one key ------------------------------------------------------------------------------------
// Decodes the key ONCE (*ok = validity, *mark = it is the identity) and walks the windows upward, base <- 16 * base (four
// doublings per window, 256 in all -- not 4 w per window): the projective base 16^w * y is parked at the head of window w
// of the key's row for the second pass.  An invalid or marked key goes on with the generator: the arithmetic stays on
// affine-representable points whatever the caller sent.
template <class C>
EC_HD void keyset_bases_body(const uint8_t* enc, u32* row, uint8_t* ok, uint8_t* mark) {
  typename C::Point base, g;
  const bool good = C::decode(base, enc);        // (invalid: decode leaves the identity)
  const bool ident = ks_is_identity(base);
  C::generator(g);
  C::cmov(base, g, ident);
  *ok = good ? 1 : 0;
  *mark = (good && ident) ? 1 : 0;
#pragma unroll 1
  for (int w = 0; w < KS_WINDOWS; ++w) {
    ks_store_point<C>(row + (size_t)w * KeysetGeom<C>::WINDOW_WORDS, base);
#pragma unroll 1
    for (int i = 0; i < 4; ++i) C::dbl(base, base);
  }
}

// ---- build, second pass: one window of one key ----------------------------------------------------------------------
// base = 16^w y from the head of the window; B .. 8B by 4 doublings and 3 additions; ONE field inversion for the eight
// entries (Montgomery's trick over their Z: 3 * 7 products beside it); the packed entries overwrite the window.
// No Z is zero: the base is a multiple of a point of prime order (or of the generator), never the identity.
template <class C>
EC_HD void keyset_window_body(u32* window) {
  typedef typename C::Fp Fp;
  typename C::Point m[KS_ENTRIES];
  ks_load_point<C>(m[0], window);
  C::dbl(m[1], m[0]);
  C::add(m[2], m[1], m[0]);
  C::dbl(m[3], m[1]);
  C::add(m[4], m[3], m[0]);
  C::dbl(m[5], m[2]);
  C::add(m[6], m[5], m[0]);
  C::dbl(m[7], m[3]);
  Fe pre[KS_ENTRIES], acc, zi;
  pre[0] = m[0].Z;
#pragma unroll
  for (int i = 1; i < KS_ENTRIES; ++i) Fp::mul(pre[i], pre[i - 1], m[i].Z);      // pre[i] = Z_0 .. Z_i
  C::invert(acc, pre[KS_ENTRIES - 1]);                                            // 1 / (Z_0 .. Z_7)
  // (kept rolled: eight copies of canon + pack pass the unroller's budget.  m and pre are then indexed at run time and live in
  // scratch, 1.3 / 1.6 KB per lane -- the build runs once per key, the walk is the kernel that must not spill)
#pragma unroll 1
  for (int i = KS_ENTRIES - 1; i >= 0; --i) {
    if (i > 0) {
      Fp::mul(zi, acc, pre[i - 1]);       // 1 / Z_i
      Fp::mul(acc, acc, m[i].Z);          // 1 / (Z_0 .. Z_(i-1))
    } else {
      zi = acc;
    }
    typename C::Affine a;
    ks_affine_from_zinv(a, m[i], zi);
    C::pack_affine(window + i * KeysetGeom<C>::ENTRY_WORDS, a);
  }
}

// ---- walk: k * y from the key's row ------------------------------------------------------------------------------------
// 65 windows upward, one add_signed_digit_affine each.  The recoded scalar stays in nine registers: the current word is
// shifted a nibble per window and the words move down one place every eight windows (static indices only: nothing is
// indexed by a run-time value, so nothing goes to scratch).  The address of an entry depends on its digit alone, not on the
// accumulator: the packed entry of window w + 1 is loaded before the addition of window w.
template <class C>
EC_HD void ks_load_entry(u32 (&e)[C::AFFINE_PACKED_WORDS], const u32* row, int w, int d) {
  const int mag = d < 0 ? -d : d;
  // (rows start on an allocation's boundary and entries are 64 / 96 bytes: 16-byte loads)
  const u32* src = static_cast<const u32*>(
      __builtin_assume_aligned(row + (size_t)(w * KS_ENTRIES + (mag > 0 ? mag - 1 : 0)) * C::AFFINE_PACKED_WORDS, 16));
#pragma unroll
  for (int i = 0; i < C::AFFINE_PACKED_WORDS; ++i) e[i] = src[i];
}

template <class C>
EC_HD void keyset_walk_body(typename C::Point& acc, const u32* row, bool marked, const uint8_t* k) {
  u32 kp[9];
  recode_signed4<C>(kp, k);
  u32 cur = kp[0];
  // the digit of window w, taken in order w = 0, 1, ..: nibble minus 8 below the top window, the nibble itself there
  auto next_digit = [&](int w) {
    const int nib = (int)(cur & 15u);
    cur >>= 4;
    if ((w & 7) == 7) {
#pragma unroll
      for (int j = 0; j < 8; ++j) kp[j] = kp[j + 1];
      cur = kp[0];
    }
    return w == KS_WINDOWS - 1 ? nib : nib - 8;
  };
  C::identity(acc);
  u32 e_next[C::AFFINE_PACKED_WORDS];
  int d_next = next_digit(0);
  ks_load_entry<C>(e_next, row, 0, d_next);
#pragma unroll 1
  for (int w = 0; w < KS_WINDOWS; ++w) {
    const int d = d_next;
    u32 e[C::AFFINE_PACKED_WORDS];
#pragma unroll
    for (int i = 0; i < C::AFFINE_PACKED_WORDS; ++i) e[i] = e_next[i];
    if (w + 1 < KS_WINDOWS) {
      d_next = next_digit(w + 1);
      ks_load_entry<C>(e_next, row, w + 1, d_next);
    }
    add_signed_digit_affine<C>(acc, d, [&](typename C::Affine& a, int) { C::unpack_affine(a, e); });
  }
  typename C::Point id;
  C::identity(id);
  C::cmov(acc, id, marked);
}

}  // namespace ec
