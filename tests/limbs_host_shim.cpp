// The bytes <-> limbs edge of the MODP kernels (mpvss_rs_amd/csrc/modp_limbs.h) compiled for the CPU, for
// tests/test_limbs_host.py: the very functions every layout's kernels inline.  Test infrastructure, never shipped.
// Every buffer the functions index is surrounded by poison here, so that a read outside it changes a result.
#include <stdint.h>
#include <string.h>

#include "../mpvss_rs_amd/csrc/modp_limbs.h"

namespace {

// slot (LIMBS lazy limbs, value < 2N) -> canonical limbs back into `slot`, the number's 64 little-endian words into `words`
template <int LIMBS>
void canonical(uint32_t* slot, const uint32_t* n, int lift_parity, uint32_t* words) {
  uint32_t s[LIMBS + 2];
  memcpy(s, slot, 4 * LIMBS);
  s[LIMBS] = s[LIMBS + 1] = 0xffffffffu;
  limbs::slot_canonicalize<LIMBS>(s, n, lift_parity);
  for (int wd = 0; wd < 64; ++wd) words[wd] = limbs::slot_word32<LIMBS>(s, wd);
  memcpy(slot, s, 4 * LIMBS);
}

}  // namespace

extern "C" {

// the 72 limbs of a 256-byte big-endian number
void limbs_from_be256(const uint8_t* be, uint32_t* out72) {
  uint8_t buf[8 + 256 + 8];
  memset(buf, 0xff, sizeof(buf));
  memcpy(buf + 8, be, 256);
  for (int j = 0; j < limbs::L; ++j) out72[j] = limbs::be256_limb(buf + 8, j);
}

// widths of the library (20, 36, 72 limbs) and the small ones at which a 32-bit word needs a limb at or above the top one
int limbs_canonical(int width, uint32_t* slot, const uint32_t* n, int lift_parity, uint32_t* words64) {
  switch (width) {
    case 10: canonical<10>(slot, n, lift_parity, words64); return 0;
    case 11: canonical<11>(slot, n, lift_parity, words64); return 0;
    case 20: canonical<20>(slot, n, lift_parity, words64); return 0;
    case 21: canonical<21>(slot, n, lift_parity, words64); return 0;
    case 22: canonical<22>(slot, n, lift_parity, words64); return 0;
    case 36: canonical<36>(slot, n, lift_parity, words64); return 0;
    case 72: canonical<72>(slot, n, lift_parity, words64); return 0;
  }
  return -1;
}
}
