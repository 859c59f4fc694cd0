// The PORTABLE compression function of mpvss_rs_amd/csrc/sha256.cpp for CPU unit tests: the library picks SHA-NI at load time on a CPU
// that has it and offers no way to take the other path, so tests/test_transcript_sweep.py compiles the same source here with the x86
// branch preprocessed away.  Test infrastructure, never shipped.
// Every system header that sha256.h / sha256.cpp include is included FIRST, with the macro still defined (glibc's headers need it); their
// include guards make the later #include lines no-ops, so the #undef reaches only the library's own code.  If sha256.cpp gains a header, add
// it to this list.  portable_uses_shani() == 0 is asserted by the test: a build that still took the SHA-NI branch is noticed.
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#undef __x86_64__
#include "../mpvss_rs_amd/csrc/sha256.cpp"

extern "C" {
int portable_uses_shani(void) { return mpvss::sha256_uses_shani() ? 1 : 0; }
// SHA-256 of data absorbed as [0, cut) then [cut, len)
void portable_sha256_split(const uint8_t* data, size_t len, size_t cut, uint8_t* out32) {
  mpvss::Sha256 s;
  s.update(data, cut);
  s.update(data + cut, len - cut);
  s.final(out32);
}
}
