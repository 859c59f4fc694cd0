// CPU run of the lane body of k_ec_lagrange (mpvss_rs_amd/csrc/ec_lagrange.h, ec_scalar.h): the same inline functions the kernel
// calls -- mont_step_u64, the two product loops over staged tiles with the lane's own index skipped, the Fermat inverse, the sign,
// the byte order -- compiled for the host.  stdin: any number of cases "m x_1 .. x_m"; stdout: per case m lines
// "<secp256k1 scalar, 64 hex digits> <ristretto255 scalar, 64 hex digits>", the 32 bytes in each group's scalar byte order.
// tests/test_ec_lagrange_host_unit.py compares them with Python integers.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../mpvss_rs_amd/csrc/ec_consts.h"
#include "../mpvss_rs_amd/csrc/ec_lagrange.h"

template <class O, bool BE>
static void coefficient(const std::vector<int64_t>& pos, size_t i, uint8_t* out32) {
  const size_t m = pos.size();
  ec::LagrangeLane s;
  ec::lagrange_begin(s);
  for (size_t base = 0; base < m; base += ec::LAGRANGE_STAGE) {     // the kernel's staging loop, tile by tile
    const size_t cnt = m - base < (size_t)ec::LAGRANGE_STAGE ? m - base : (size_t)ec::LAGRANGE_STAGE;
    ec::lagrange_accumulate<O>(s, pos[i], pos.data() + base, (int)cnt, (i >= base && i - base < cnt) ? (int)(i - base) : -1);
  }
  ec::Sc lambda;
  ec::lagrange_finish<O>(lambda, s);
  ec::lagrange_store<BE>(out32, lambda);
}

static void hex(const uint8_t* b) {
  for (int k = 0; k < 32; ++k) printf("%02x", b[k]);
}

int main() {
  long long m;
  while (scanf("%lld", &m) == 1) {
    if (m < 0 || m > (1 << 20)) return 2;
    std::vector<int64_t> pos((size_t)m);
    for (auto& x : pos) {
      long long v;
      if (scanf("%lld", &v) != 1) return 2;
      x = (int64_t)v;
    }
    for (size_t i = 0; i < pos.size(); ++i) {
      uint8_t a[32], b[32];
      coefficient<ec::OrderSecp, true>(pos, i, a);
      coefficient<ec::OrderEd, false>(pos, i, b);
      hex(a);
      printf(" ");
      hex(b);
      printf("\n");
    }
  }
  return 0;
}
