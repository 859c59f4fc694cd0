// Row-layout kernels of a run-time MODP group (bn_row_rt.h: 16 lanes per number, four numbers per one-wave workgroup) for the
// SMALL calls of the mpvss_modp_group_* entry points: a call of a handful to a few thousand numbers is the latency of one
// number's chain of 2 000 to 5 000 Montgomery operations, and about a third of the quad layout's instructions lie on that chain
// (by the count of a row's instructions in DESIGN section 13, not by a measurement).  The counterpart of k_modp_dual_exp_row
// (modp_row_kernels.hip) at the handles of 18 / 27 / 36 quad limbs per lane.
//
//   k_rt_dual_exp_row<LPL>  the program of rt_dual_exp_body (modp_rt_kernels.inc): out = B1^e1 B2^e2, 4-bit windows from the
//                           wave's highest one over e1 and e2, squarings shared; tab2 optional; strides of 0 mean shared;
//                           blockIdx.y = 1: a second exponent set over the same table (k_rt_exp_sets' shape)
//   k_rt_comb_exp_row<LPL>  the program of k_rt_comb_exp: e1 over the comb of the shared base without squarings (rows whose digit
//                           is 0 in all four numbers of the wave are skipped by ballot), e2 left to right over tab2
//
// They read the 16-entry tables (k_rt_table) and combs (k_rt_comb_*) of the quad kernels as they lie in HBM, take the
// modp_rt_consts image handed in (q, or q' for the Lagrange inverses) and write Montgomery limbs below 2N, which
// modp_rt_launch_from_mont turns into canonical bytes (one more product by plain 1, the exit step of the quad programs).
// A translation unit of its own: no existing instance is compiled differently.
//
// Out of scope: row variants of k_rt_keyset_exp(_idx), k_rt_commit_eval*, k_rt_twin_exp and k_rt_fd_chain.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bn_row_rt.h"
#include "modp_rt_kernels.h"

using namespace bnrowrt;

namespace {

// the row layout of a quad width: QL quad limbs per lane -> L, EB, row LPL
template <int QL>
struct RowWidth {
  static constexpr int L = 4 * QL;
  static constexpr int EB = QL == 36 ? 512 : QL == 27 ? 384 : 256;
  static constexpr int LPL = row_lpl(QL);
  static constexpr int SLOT = Slot<LPL>::WORDS;
  static constexpr int LDS_WORDS = NUMS_PER_WAVE * SLOT + LDS_PAD;
};

// bit length of an EB-byte big-endian number, the maximum over the whole wave (every row: lane l scans bytes EB/16 l ..
// EB/16 l + EB/16 - 1, lane 0 the most significant ones)
template <int EB>
__device__ __forceinline__ int wave_max_bits(const uint8_t* __restrict__ be, const Lane& ln) {
  constexpr int WORDS = EB / 64;                            // 32-bit words of a lane's sixteenth
  const u32* p = reinterpret_cast<const u32*>(be) + WORDS * ln.l;
  int bl = 0;
#pragma unroll
  for (int i = WORDS - 1; i >= 0; --i) {
    const u32 word = __builtin_bswap32(p[i]);               // big-endian word i of this lane's part
    if (word != 0) bl = (WORDS - i) * 32 - __builtin_clz(word);
  }
  if (bl > 0) bl += (15 - (int)ln.l) * (EB / 2);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int other = __shfl_xor(bl, off);
    bl = other > bl ? other : bl;
  }
  return __builtin_amdgcn_readfirstlane(bl);
}

template <int EB>
__device__ __forceinline__ u32 nibble(const uint8_t* __restrict__ e, int w) {
  const u32 byte = e[EB - 1 - (w >> 1)];
  return (w & 1) ? (byte >> 4) : (byte & 15u);
}

}  // namespace

// one wave per workgroup; the product holds about 4 LPL + 20 registers, so the allocation never bounds the residency
#define RT_ROW_KERNEL __launch_bounds__(64)

template <int QL>
__global__ void RT_ROW_KERNEL k_rt_dual_exp_row(const u32* __restrict__ tab1, size_t tab1_stride, const u32* __restrict__ tab2,
                                                size_t tab2_stride, const uint8_t* __restrict__ e1_be, size_t e1_stride,
                                                const uint8_t* __restrict__ e2_be, size_t e2_stride,
                                                const uint8_t* __restrict__ e1b_be, int count, u32* __restrict__ out_m,
                                                const modp_rt_consts* __restrict__ cs) {
  using RW = RowWidth<QL>;
  constexpr int L = RW::L, LPL = RW::LPL, EB = RW::EB;
  __shared__ __attribute__((aligned(16))) u32 lds[RW::LDS_WORDS];
  const Lane ln = make_lane();
  const int num = threadIdx.x >> 4;
  const int xi = blockIdx.x * NUMS_PER_WAVE + num;
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + num * RW::SLOT;
  const u32 n0inv = cs->n0inv;
  const bool has2 = tab2 != nullptr;
  const u32* t1 = tab1 + (size_t)x * tab1_stride;
  const u32* t2 = has2 ? tab2 + (size_t)x * tab2_stride : t1;
  const uint8_t* e1 = (blockIdx.y ? e1b_be : e1_be) + (size_t)x * e1_stride;
  const uint8_t* e2 = has2 ? e2_be + (size_t)x * e2_stride : e1;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL, L>(n, cs->n, ln);
  int nb = wave_max_bits<EB>(e1, ln);
  if (has2) {
    const int nb2 = wave_max_bits<EB>(e2, ln);
    nb = nb2 > nb ? nb2 : nb;
  }
  const int nw = (nb + 3) >> 2;
  // steps: 0..3 square, 4 times tab1[d1], 5 times tab2[d2], 6 next window (the last window ends the chain)
  int w = nw - 1, s = has2 ? 5 : 6;
  if (nw == 0) load_lane_limbs<LPL, L>(acc, cs->one_m, ln);
  else load_lane_limbs<LPL, L>(acc, t1 + (size_t)nibble<EB>(e1, w) * L, ln);
  while (nw != 0) {
    if (s == 6) {
      if (w == 0) break;
      --w;
      s = 0;
    }
    if (s < 4) {
      slot_store<LPL>(slot, acc, ln);
    } else {
      const u32 d = nibble<EB>(s == 4 ? e1 : e2, w);
      slot_fill_from_global<LPL, L>(slot, (s == 4 ? t1 : t2) + (size_t)d * L, ln);
    }
    __builtin_amdgcn_wave_barrier();
    if (s < 4) mont_mul<LPL, L, true>(acc, acc, slot, n, n0inv, ln);
    else mont_mul<LPL, L>(acc, acc, slot, n, n0inv, ln);
    __builtin_amdgcn_wave_barrier();
    ++s;
    if (s == 5 && !has2) s = 6;
  }
  if (live) store_lane_limbs<LPL, L>(out_m + ((size_t)blockIdx.y * count + x) * L, acc, ln);
}

template <int QL>
__global__ void RT_ROW_KERNEL k_rt_comb_exp_row(const u32* __restrict__ comb, const u32* __restrict__ tab2, size_t tab2_stride,
                                                const uint8_t* __restrict__ e1_be, const uint8_t* __restrict__ e2_be, size_t e2_stride,
                                                int count, u32* __restrict__ out_m, const modp_rt_consts* __restrict__ cs) {
  using RW = RowWidth<QL>;
  constexpr int L = RW::L, LPL = RW::LPL, EB = RW::EB;
  __shared__ __attribute__((aligned(16))) u32 lds[RW::LDS_WORDS];
  const Lane ln = make_lane();
  const int num = threadIdx.x >> 4;
  const int xi = blockIdx.x * NUMS_PER_WAVE + num;
  const bool live = xi < count;
  const int x = live ? xi : count - 1;
  u32* slot = lds + num * RW::SLOT;
  const u32 n0inv = cs->n0inv;
  const bool has2 = tab2 != nullptr;
  const uint8_t* e1 = e1_be + (size_t)x * EB;
  const uint8_t* e2 = has2 ? e2_be + (size_t)x * e2_stride : e1;
  const u32* t2 = has2 ? tab2 + (size_t)x * tab2_stride : comb;
  u32 n[LPL], acc[LPL];
  load_lane_limbs<LPL, L>(n, cs->n, ln);
  const int nw1 = (wave_max_bits<EB>(e1, ln) + 3) >> 2;                 // <= 2 EB, the comb's rows
  const int nw2 = has2 ? (wave_max_bits<EB>(e2, ln) + 3) >> 2 : 0;
  // steps: 0..3 square, 4 times tab2[d2], 5 next window of e2, 6 times comb[k][d1] (the comb's last live row ends the chain)
  int w = nw2 - 1, k = 0, s;
  if (nw2 == 0) {
    load_lane_limbs<LPL, L>(acc, cs->one_m, ln);
    s = 6;
  } else {
    load_lane_limbs<LPL, L>(acc, t2 + (size_t)nibble<EB>(e2, w) * L, ln);
    s = 5;
  }
  while (true) {
    if (s == 5) {
      if (w == 0) {
        s = 6;
      } else {
        --w;
        s = 0;
      }
    }
    if (s == 6) {
      while (k < nw1 && __builtin_amdgcn_ballot_w64(nibble<EB>(e1, k) != 0) == 0) ++k;
      if (k == nw1) break;
    }
    if (s < 4) {
      slot_store<LPL>(slot, acc, ln);
    } else if (s == 4) {
      slot_fill_from_global<LPL, L>(slot, t2 + (size_t)nibble<EB>(e2, w) * L, ln);
    } else {
      slot_fill_from_global<LPL, L>(slot, comb + ((size_t)k * 16 + nibble<EB>(e1, k)) * L, ln);
      ++k;
    }
    __builtin_amdgcn_wave_barrier();
    if (s < 4) mont_mul<LPL, L, true>(acc, acc, slot, n, n0inv, ln);
    else mont_mul<LPL, L>(acc, acc, slot, n, n0inv, ln);
    __builtin_amdgcn_wave_barrier();
    if (s < 5) ++s;
  }
  if (live) store_lane_limbs<LPL, L>(out_m + (size_t)x * L, acc, ln);
}

static inline int row_grid(int count) { return (count + NUMS_PER_WAVE - 1) / NUMS_PER_WAVE; }

#define RT_ROW_DISPATCH(lpl, KERNEL, ...)                                   \
  do {                                                                      \
    if ((lpl) == 18) hipLaunchKernelGGL(KERNEL<18>, __VA_ARGS__);           \
    else if ((lpl) == 27) hipLaunchKernelGGL(KERNEL<27>, __VA_ARGS__);      \
    else if ((lpl) == 36) hipLaunchKernelGGL(KERNEL<36>, __VA_ARGS__);      \
    else return (int)hipErrorInvalidValue;                                  \
  } while (0)

extern "C" int modp_rt_row_launch_dual_exp(int lpl, const uint32_t* tab1, size_t tab1_stride, const uint32_t* tab2, size_t tab2_stride,
                                           const uint8_t* e1, size_t e1_stride, const uint8_t* e2, size_t e2_stride, int count,
                                           uint32_t* out_m, const modp_rt_consts* cs, hipStream_t s) {
  if (lpl != 18 && lpl != 27 && lpl != 36) return (int)hipErrorInvalidValue;
  if (count <= 0) return 0;
  RT_ROW_DISPATCH(lpl, k_rt_dual_exp_row, dim3(row_grid(count)), dim3(64), 0, s, tab1, tab1_stride, tab2, tab2_stride, e1, e1_stride, e2,
                  e2_stride, (const uint8_t*)nullptr, count, out_m, cs);
  return (int)hipGetLastError();
}

extern "C" int modp_rt_row_launch_exp_sets(int lpl, const uint32_t* tab, size_t tab_stride, const uint8_t* e1, const uint8_t* e2, int count,
                                           uint32_t* out_m, const modp_rt_consts* cs, hipStream_t s) {
  if (lpl != 18 && lpl != 27 && lpl != 36) return (int)hipErrorInvalidValue;
  if (count <= 0) return 0;
  const size_t eb = lpl == 36 ? 512 : lpl == 27 ? 384 : 256;
  RT_ROW_DISPATCH(lpl, k_rt_dual_exp_row, dim3(row_grid(count), 2), dim3(64), 0, s, tab, tab_stride, (const uint32_t*)nullptr, (size_t)0, e1,
                  eb, (const uint8_t*)nullptr, (size_t)0, e2, count, out_m, cs);
  return (int)hipGetLastError();
}

extern "C" int modp_rt_row_launch_comb_exp(int lpl, const uint32_t* comb, const uint32_t* tab2, size_t tab2_stride, const uint8_t* e1,
                                           const uint8_t* e2, size_t e2_stride, int count, uint32_t* out_m, const modp_rt_consts* cs,
                                           hipStream_t s) {
  if (lpl != 18 && lpl != 27 && lpl != 36) return (int)hipErrorInvalidValue;
  if (count <= 0) return 0;
  RT_ROW_DISPATCH(lpl, k_rt_comb_exp_row, dim3(row_grid(count)), dim3(64), 0, s, comb, tab2, tab2_stride, e1, e2, e2_stride, count, out_m,
                  cs);
  return (int)hipGetLastError();
}
