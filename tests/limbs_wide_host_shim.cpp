// The bytes <-> limbs edge of a wide run-time MODP group (384-byte elements, 108 limbs: mpvss_rs_amd/csrc/modp_limbs.h at
// EB = 384) compiled for the CPU, for tests/test_modp_rt_wide_host.py: the very functions the 27-limb kernels inline.
// Test infrastructure, never shipped.  Every buffer the functions index is surrounded by poison here, so that a read
// outside it changes a result.
#include <stdint.h>
#include <string.h>

#include "../mpvss_rs_amd/csrc/modp_limbs.h"

extern "C" {

// the 108 limbs of a 384-byte big-endian number
void limbs_from_be384(const uint8_t* be, uint32_t* out108) {
  uint8_t buf[8 + 384 + 8];
  memset(buf, 0xff, sizeof(buf));
  memcpy(buf + 8, be, 384);
  for (int j = 0; j < 108; ++j) out108[j] = limbs::be_limb<384>(buf + 8, j);
}

// slot (108 lazy limbs, value < 2N) -> canonical limbs back into `slot`, the number's 96 little-endian words into `words96`
void limbs_canonical108(uint32_t* slot, const uint32_t* n, uint32_t* words96) {
  uint32_t s[108 + 2];
  memcpy(s, slot, 4 * 108);
  s[108] = s[109] = 0xffffffffu;
  limbs::slot_canonicalize<108>(s, n);
  for (int wd = 0; wd < 96; ++wd) words96[wd] = limbs::slot_word32<108, 384>(s, wd);
  memcpy(slot, s, 4 * 108);
}
}
