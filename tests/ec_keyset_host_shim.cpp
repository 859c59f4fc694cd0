// Host build of the key-set bodies of the curve groups (mpvss_rs_amd/csrc/ec_keyset.h) for CPU unit tests.
// Test infrastructure: compiled by tests/ec_keyset_cases.py with g++, never shipped.
#include "../mpvss_rs_amd/csrc/ec_keyset.h"

using namespace ec;

// the two passes of the build for one key: row = ROW_WORDS words
template <class C>
static void t_build(const uint8_t* enc, u32* row, uint8_t* ok, uint8_t* mark) {
  keyset_bases_body<C>(enc, row, ok, mark);
  for (int w = 0; w < KS_WINDOWS; ++w) keyset_window_body<C>(row + (size_t)w * KeysetGeom<C>::WINDOW_WORDS);
}

template <class C>
static void t_walk(const u32* row, int marked, const uint8_t* k, uint8_t* out) {
  typename C::Point acc;
  keyset_walk_body<C>(acc, row, marked != 0, k);
  C::encode(out, acc);
}

// a packed entry back to the canonical encoding of its point; 0, or -1 when the entry is not a consistent affine form
static int t_entry(const Secp&, const u32* e, uint8_t* out) {
  Secp::Affine a;
  Secp::unpack_affine(a, e);
  Secp::Point p;
  p.X = a.x;
  p.Y = a.y;
  Secp::Fp::one(p.Z);
  Secp::encode(out, p);
  return 0;
}
static int t_entry(const Ristretto&, const u32* e, uint8_t* out) {
  typedef Ristretto::Fp Fp;
  const Fe d2 = {EC_ED_2D_INIT};
  Ristretto::Affine a;
  Ristretto::unpack_affine(a, e);
  Fe two, half, x, y, t;
  Fp::one(two);
  Fp::addc(two, two, two);
  Ristretto::invert(half, two);
  Fp::sub(x, a.ypx, a.ymx);
  Fp::mul(x, x, half);
  Fp::addc(y, a.ypx, a.ymx);
  Fp::mul(y, y, half);
  Ristretto::Point p;
  p.X = x;
  p.Y = y;
  Fp::one(p.Z);
  Fp::mul(p.T, x, y);
  Fp::mul(t, p.T, d2);
  Ristretto::encode(out, p);
  return Fp::equal(t, a.xy2d) ? 0 : -1;
}

extern "C" {
int ks_row_words(int group) { return group == 1 ? KeysetGeom<Secp>::ROW_WORDS : KeysetGeom<Ristretto>::ROW_WORDS; }
int ks_entry_words(int group) { return group == 1 ? KeysetGeom<Secp>::ENTRY_WORDS : KeysetGeom<Ristretto>::ENTRY_WORDS; }
void ks_build(int group, const uint8_t* enc, uint32_t* row, uint8_t* ok, uint8_t* mark) {
  if (group == 1) t_build<Secp>(enc, row, ok, mark); else t_build<Ristretto>(enc, row, ok, mark);
}
void ks_walk(int group, const uint32_t* row, int marked, const uint8_t* k, uint8_t* out) {
  if (group == 1) t_walk<Secp>(row, marked, k, out); else t_walk<Ristretto>(row, marked, k, out);
}
int ks_entry_encode(int group, const uint32_t* entry, uint8_t* out) {
  return group == 1 ? t_entry(Secp(), entry, out) : t_entry(Ristretto(), entry, out);
}
}
