// =====================================================================================================
// Scalar-field side of the protocol (host, behind the C ABI) and `reconstruct` for the three groups.
// Part of mpvss_capi.cpp (included after capi_ec.inc).
// =====================================================================================================
#include "host_scalar.h"

namespace {

// order of the scalar ring of a group: MODP q - 1 (32 limbs), secp256k1 n, ristretto255 l (4 limbs)
const hsc::Modulus<32>& modp_order() {        // q - 1   (src/groups/modp.rs:67,101-103)
  static const hsc::Modulus<32> M = [] {
    uint8_t qbe[EB];
    for (size_t byte = 0; byte < EB; ++byte) {
      unsigned v = 0;
      for (int bit = 0; bit < 8; ++bit) {
        const size_t b = byte * 8 + bit;
        v |= ((MODP_N_LIMBS[b / MODP_W] >> (b % MODP_W)) & 1u) << bit;
      }
      qbe[EB - 1 - byte] = (uint8_t)v;
    }
    uint64_t q[32];
    hsc::from_bytes<32>(q, qbe, true);
    q[0] -= 1;                                  // q is odd
    hsc::Modulus<32> m;
    m.set(q);
    return m;
  }();
  return M;
}
const hsc::Modulus<32>& modp_subgroup_order() {   // (q - 1) / 2   (src/groups/modp.rs:59,105-107), an odd prime
  static const hsc::Modulus<32> M = [] {
    uint64_t g[32];
    memcpy(g, modp_order().m, sizeof(g));
    for (int i = 0; i < 31; ++i) g[i] = (g[i] >> 1) | (g[i + 1] << 63);
    g[31] >>= 1;
    hsc::Modulus<32> m;
    m.set(g);
    return m;
  }();
  return M;
}
const hsc::Modulus<4>& ec_order(const EcInfo* gi) {
  static const hsc::Modulus<4> M[2] = {[] { uint64_t n[4]; hsc::from_bytes<4>(n, ec_info(1)->order_be, true); hsc::Modulus<4> m; m.set(n); return m; }(),
                                       [] { uint64_t n[4]; hsc::from_bytes<4>(n, ec_info(2)->order_be, true); hsc::Modulus<4> m; m.set(n); return m; }()};
  return M[gi->group - 1];
}
int host_threads(int requested) {
  if (requested > 0) return requested > 64 ? 64 : requested;
  const unsigned hc = std::thread::hardware_concurrency();
  return hc == 0 ? 1 : (hc > 16 ? 16 : (int)hc);
}

// generic bodies over (N limbs, byte width, endianness); Mod: hsc::Modulus<N>, or hsc::ModulusRt for N = 32
template <int N, class Mod>
void scalar_mul_bytes(const Mod& M, bool be, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  uint64_t x[N], y[N], r[N];
  hsc::from_bytes<N>(x, a, be);
  hsc::from_bytes<N>(y, b, be);
  M.mulmod(r, x, y);                                                   // (a * b) % order
  hsc::to_bytes<N>(out, r, be);
}
template <int N, class Mod>
void scalar_sub_bytes(const Mod& M, bool be, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  // modp.rs:184-192: diff = a - b; diff < 0 ? diff + order : diff % order   (the curve crates reduce as well)
  uint64_t x[N], y[N], r[N];
  hsc::from_bytes<N>(x, a, be);
  hsc::from_bytes<N>(y, b, be);
  if (hsc::sub_n<N>(r, x, y)) hsc::add_n<N>(r, r, M.m); else M.reduce1(r);
  hsc::to_bytes<N>(out, r, be);
}
// r_i = w_i - (alpha_i * c) % order, normalised as scalar_sub does   (dleq.rs:42-50, participant.rs:255-264)
template <int N, class Mod>
void responses_bytes(const Mod& M, bool be, const uint8_t* w, const uint8_t* alpha, const uint8_t* c, size_t c_stride,
                     size_t n, uint8_t* r_out, int threads) {
  constexpr size_t SB = (size_t)N * 8;
  hsc::parallel_for(n, threads, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      uint64_t ww[N], aa[N], cc[N], p[N], r[N];
      hsc::from_bytes<N>(ww, w + i * SB, be);
      hsc::from_bytes<N>(aa, alpha + i * SB, be);
      hsc::from_bytes<N>(cc, c + i * c_stride, be);
      M.mulmod(p, aa, cc);
      M.reduce1(ww);
      M.submod(r, ww, p);
      hsc::to_bytes<N>(r_out + i * SB, r, be);
    }
  });
}
// out_i = P(positions_i) mod order, P = sum_j coeffs_j x^j   (polynomial.rs:50-58 evaluates over the integers and the
// caller reduces, participant.rs:202 / 1155-1157 / 1619-1621: the same residue as Horner's rule in the ring)
template <int N, class Mod>
void poly_eval_bytes(const Mod& M, bool be, const uint8_t* coeffs, size_t t, const int64_t* positions, size_t n,
                     uint8_t* out, int threads) {
  constexpr size_t SB = (size_t)N * 8;
  std::vector<hsc::Num<N>> cf(t);
  for (size_t j = 0; j < t; ++j) {
    hsc::from_bytes<N>(cf[j].v, coeffs + j * SB, be);
    M.reduce1(cf[j].v);
  }
  auto horner = [&](uint64_t x, uint64_t* acc) {
    // the position as a ring element: MODP positions are >= 0 (the reference's BigInt::from(i64) with a negative
    // value makes `% order` negative -- not a value any caller produces); the curves use `position as u64`
    memcpy(acc, cf[t - 1].v, sizeof(uint64_t) * N);
    for (size_t j = t - 1; j-- > 0;) M.muladd_small(acc, acc, x, cf[j].v);
  };
  hsc::parallel_for(n, threads, [&](size_t lo, size_t hi) {
    // Consecutive positions (the dealer's 1..n, participant.rs:186,198): P has degree t-1, so its t-th forward difference
    // vanishes and P(i+1) follows from P(i) by t-1 modular ADDITIONS along the bottom diagonal of the difference table
    // (b_k <- b_k + b_(k+1), b_(t-1) constant) instead of a Horner pass of t-1 multiply-adds -- 4-5x less work per share at
    // t = 256.  A run needs t values by Horner's rule and t^2/2 subtractions to start, so it pays from about 4 t positions.
    std::vector<hsc::Num<N>> diag;
    size_t i = lo;
    while (i < hi) {
      size_t run = 1;
      while (i + run < hi && positions[i + run] == positions[i + run - 1] + 1 && positions[i + run] > 0) ++run;
      if (t >= 2 && run >= 4 * t) {
        diag.resize(t);
        for (size_t j = 0; j < t; ++j) {
          horner((uint64_t)positions[i + j], diag[j].v);
          hsc::to_bytes<N>(out + (i + j) * SB, diag[j].v, be);
        }
        // in place: after level k, diag[j] = Delta^k P(x_j) for j <= t-1-k; what stays behind is the bottom diagonal,
        // diag[t-1-k] = Delta^k P(x_(t-1-k))
        for (size_t k = 1; k < t; ++k)
          for (size_t j = 0; j + k < t; ++j) M.submod(diag[j].v, diag[j + 1].v, diag[j].v);
        for (size_t s = t; s < run; ++s) {
          for (size_t k = t - 1; k-- > 0;) M.addmod(diag[t - 1 - k].v, diag[t - 1 - k].v, diag[t - 2 - k].v);
          hsc::to_bytes<N>(out + (i + s) * SB, diag[t - 1].v, be);
        }
      } else {
        for (size_t j = 0; j < run; ++j) {
          uint64_t acc[N];
          horner((uint64_t)positions[i + j], acc);
          hsc::to_bytes<N>(out + (i + j) * SB, acc, be);
        }
      }
      i += run;
    }
    for (auto& v : diag) {                              // the difference table is a function of the (secret) coefficients
      volatile uint64_t* wp = v.v;
      for (int k = 0; k < N; ++k) wp[k] = 0;
    }
  });
  for (auto& v : cf) {
    volatile uint64_t* wp = v.v;
    for (int k = 0; k < N; ++k) wp[k] = 0;
  }
}

// |lambda_i| mod M with the fraction in lowest terms first, as the reference forms it for MODP (participant.rs:546-553: numerator
// and denominator divided by their gcd, then the denominator inverted mod M).  lagrange_at_zero comes here only when the raw
// denominator has no inverse mod M: a modulus so small that a position or a difference of two positions shares a factor with it
// (q = 23: positions {1, 11, 12} give 132/110 = 6/5 mod 11).  The 64-bit factors x_j and |x_j - x_i| are cancelled pairwise; each
// pair is visited once and later steps only divide, so afterwards every pair is coprime and so are the two products.  A
// quadratic number of gcds per coefficient, paid by no call whose raw denominators are units.  False: the reduced denominator
// has no inverse either (the reference returns None).
template <int N, class Mod>
bool lagrange_reduced_magnitude(const Mod& M, const int64_t* pos, size_t m, size_t i, uint64_t* mag) {
  std::vector<uint64_t> top, bot;
  for (size_t j = 0; j < m; ++j) {
    if (j == i) continue;
    const int64_t diff = pos[j] - pos[i];
    top.push_back((uint64_t)pos[j]);
    bot.push_back((uint64_t)(diff < 0 ? -diff : diff));
  }
  for (uint64_t& x : top)
    for (uint64_t& y : bot) {
      if (x == 1) break;
      uint64_t a = x, b = y;
      while (b) { const uint64_t r = a % b; a = b; b = r; }
      x /= a;
      y /= a;
    }
  uint64_t num[N], den[N], inv[N];
  const uint64_t zero[N] = {0};
  memset(num, 0, sizeof(num));
  num[0] = 1;
  memcpy(den, num, sizeof(num));
  for (uint64_t x : top) M.muladd_small(num, num, x, zero);
  for (uint64_t y : bot) M.muladd_small(den, den, y, zero);
  if (!M.invert(inv, den)) return false;
  M.mulmod(mag, num, inv);
  return true;
}

// Lagrange coefficients at 0 over the ring of an ODD modulus:
//   lambda_i = prod_{j != i} x_j / (x_j - x_i)      magnitude mod M, sign separately (participant.rs:1525-1544)
// positions must be pairwise different.  mag[i] = |num| * |den|^-1 mod M; neg[i] = sign of the integer coefficient.  A unit
// denominator gives the value of the reduced fraction as it stands (the gcd divides it, so the gcd is a unit too); only a
// denominator without inverse goes through lagrange_reduced_magnitude.  Over the prime moduli of the fixed groups (all above 2^63)
// every denominator is a unit.
// One coefficient, lambda_i: the coefficients of a position list are independent of each other, so a caller with many of them may
// spread them over host threads (mpvss_modp_group_reconstruct_many).
template <int N, class Mod>
bool lagrange_coefficient_at_zero(const Mod& M, const int64_t* pos, size_t m, size_t i, uint64_t* mag, char* neg) {
  uint64_t num[N], den[N], one[N];
  memset(one, 0, sizeof(one));
  one[0] = 1;
  memcpy(num, one, sizeof(one));
  memcpy(den, one, sizeof(one));
  const uint64_t zero[N] = {0};
  bool negative = false;
  for (size_t j = 0; j < m; ++j) {
    if (j == i) continue;
    if (pos[j] == pos[i]) return false;
    const uint64_t xj = (uint64_t)pos[j];           // Scalar::from(j as u64) / BigInt j >= 1
    M.muladd_small(num, num, xj, zero);
    const int64_t diff = pos[j] - pos[i];
    if (diff < 0) negative = !negative;
    M.muladd_small(den, den, (uint64_t)(diff < 0 ? -diff : diff), zero);
  }
  uint64_t inv[N];
  if (M.invert(inv, den)) M.mulmod(mag, num, inv);
  else if (!lagrange_reduced_magnitude<N>(M, pos, m, i, mag)) return false;
  *neg = negative ? 1 : 0;
  return true;
}

template <int N, class Mod>
bool lagrange_at_zero(const Mod& M, const int64_t* pos, size_t m, std::vector<hsc::Num<N>>& mag, std::vector<char>& neg,
                      bool positions_as_u64) {
  (void)positions_as_u64;
  mag.resize(m);
  neg.assign(m, 0);
  for (size_t i = 0; i < m; ++i)
    if (!lagrange_coefficient_at_zero<N>(M, pos, m, i, mag[i].v, &neg[i])) return false;
  return true;
}

}  // namespace

// ---- Group::scalar_mul / scalar_sub (src/group.rs:108-113) ------------------------------------------------------
extern "C" int mpvss_modp_scalar_mul(const uint8_t* a256, const uint8_t* b256, uint8_t* out256) {
  if (!a256 || !b256 || !out256) return MPVSS_E_INVALID;
  scalar_mul_bytes<32>(modp_order(), true, a256, b256, out256);          // modp.rs:180-182
  return MPVSS_OK;
}
extern "C" int mpvss_modp_scalar_sub(const uint8_t* a256, const uint8_t* b256, uint8_t* out256) {
  if (!a256 || !b256 || !out256) return MPVSS_E_INVALID;
  scalar_sub_bytes<32>(modp_order(), true, a256, b256, out256);          // modp.rs:184-192
  return MPVSS_OK;
}
extern "C" int mpvss_ec_scalar_mul(int group, const uint8_t* a32, const uint8_t* b32, uint8_t* out32) {
  const EcInfo* gi = ec_info(group);
  if (!gi || !a32 || !b32 || !out32) return MPVSS_E_INVALID;
  scalar_mul_bytes<4>(ec_order(gi), gi->scalar_be, a32, b32, out32);     // secp256k1.rs:173-176, ristretto255.rs:244-247
  return MPVSS_OK;
}
extern "C" int mpvss_ec_scalar_sub(int group, const uint8_t* a32, const uint8_t* b32, uint8_t* out32) {
  const EcInfo* gi = ec_info(group);
  if (!gi || !a32 || !b32 || !out32) return MPVSS_E_INVALID;
  scalar_sub_bytes<4>(ec_order(gi), gi->scalar_be, a32, b32, out32);     // secp256k1.rs:178-181, ristretto255.rs:249-252
  return MPVSS_OK;
}

// ---- batched DLEQ responses r_i = w_i - alpha_i * c (dleq.rs:42-50) -------------------------------------------------
extern "C" int mpvss_modp_dleq_responses(const uint8_t* w, const uint8_t* alpha, const uint8_t* c, int c_per_share, size_t n,
                                         uint8_t* r_out, int threads) {
  if (n == 0) return MPVSS_OK;
  if (!w || !alpha || !c || !r_out) return MPVSS_E_INVALID;
  responses_bytes<32>(modp_order(), true, w, alpha, c, c_per_share ? EB : 0, n, r_out, host_threads(threads));
  return MPVSS_OK;
}
extern "C" int mpvss_ec_dleq_responses(int group, const uint8_t* w, const uint8_t* alpha, const uint8_t* c, int c_per_share,
                                       size_t n, uint8_t* r_out, int threads) {
  const EcInfo* gi = ec_info(group);
  if (!gi) return MPVSS_E_UNSUPPORTED;
  if (n == 0) return MPVSS_OK;
  if (!w || !alpha || !c || !r_out) return MPVSS_E_INVALID;
  responses_bytes<4>(ec_order(gi), gi->scalar_be, w, alpha, c, c_per_share ? 32 : 0, n, r_out, host_threads(threads));
  return MPVSS_OK;
}

// ---- polynomial values P(i) mod order (polynomial.rs:50-58 + the caller's `% order`) ---------------------------------
extern "C" int mpvss_modp_poly_eval(const uint8_t* coeffs, size_t t, const int64_t* positions, size_t n, uint8_t* out, int threads) {
  if (n == 0) return MPVSS_OK;
  if (!coeffs || !positions || !out || t == 0) return MPVSS_E_INVALID;
  for (size_t i = 0; i < n; ++i)
    if (positions[i] < 0) return MPVSS_E_INVALID;
  poly_eval_bytes<32>(modp_order(), true, coeffs, t, positions, n, out, host_threads(threads));
  return MPVSS_OK;
}
// ---- the same two on the device (MODP: the scalars are 2048 bits wide and the host loops cost more than the group work of
// a box: 86 ms against 74 ms per 65536-share box on 16 host threads; the kernels below take a millisecond or two) -----------
// Z/(q-1) = Z/2 x Z/q' (q' = (q-1)/2 odd): residues mod q' by the Montgomery product of the group kernels with the constants
// of q', parities on the side (k_modq_* in modp_kernels.hip).
namespace {
// a'_j = (a_j mod (q-1)) 2^(522 j) mod q' as 72 limbs of 29 bits each; parities of P at even and odd positions
void modq_poly_limbs(const uint8_t* coeffs_host, size_t t, uint32_t* limbs, int* par_even, int* par_odd) {
  const hsc::Modulus<32>& M = modp_order();
  const hsc::Modulus<32>& Q = modp_subgroup_order();
  uint64_t f[32], step[32], a[32], r[32];
  memset(f, 0, sizeof(f));
  f[0] = 1;
  memset(step, 0, sizeof(step));
  step[522 / 64] = (uint64_t)1 << (522 % 64);
  Q.reduce1(step);
  *par_even = 0;
  *par_odd = 0;
  for (size_t j = 0; j < t; ++j) {
    hsc::from_bytes<32>(a, coeffs_host + j * EB, true);
    M.reduce1(a);
    if (j == 0) *par_even = (int)(a[0] & 1);
    *par_odd ^= (int)(a[0] & 1);
    Q.reduce1(a);
    Q.mulmod(r, a, f);
    for (int k = 0; k < MODP_L; ++k) {
      const int bit = MODP_W * k, w = bit / 64, sft = bit % 64;
      uint64_t v = w < 32 ? r[w] >> sft : 0;          // limb 71 starts at bit 2059
      if (sft + MODP_W > 64 && w + 1 < 32) v |= r[w + 1] << (64 - sft);
      limbs[j * MODP_L + k] = (uint32_t)v & ((1u << MODP_W) - 1);
    }
    Q.mulmod(r, f, step);
    memcpy(f, r, sizeof(f));
  }
  for (uint64_t* buf : {a, r, f}) {                   // the coefficients are the dealer's secret
    volatile uint64_t* wipe = buf;
    for (int i = 0; i < 32; ++i) wipe[i] = 0;
  }
}
int modq_consts(mpvss_ctx* ctx) {
  if (ctx->consts_q) return 0;
  const int rc = modq_consts_upload(&ctx->consts_q);
  if (rc != 0) return fail(ctx, MPVSS_E_DEVICE, "constants of (q-1)/2", (hipError_t)rc);
  return 0;
}
// The stand-alone calls run on their own high-priority stream and give the context lock back while they wait, so that they
// neither queue behind the boxes in flight nor hold up the threads that enqueue and absorb those.  A small ring of staging
// entries (pinned host + device, one event each) carries their few hundred bytes of parameters.
int scalar_entry(mpvss_ctx* ctx, size_t bytes, mpvss_ctx::ScalarEntry** out) {
  if (!ctx->scalar_stream) HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->scalar_stream, hipStreamNonBlocking, ctx->prio_high));
  // an entry belongs to its call until that call has re-taken the context lock and is done with the pinned memory
  // (in_use): a caller that finds all of them taken is the seventeenth concurrent scalar call on one context
  mpvss_ctx::ScalarEntry* e = nullptr;
  for (unsigned k = 0; k < mpvss_ctx::SCALAR_RING && !e; ++k) {
    mpvss_ctx::ScalarEntry& c = ctx->scalar_ring[(ctx->scalar_seq + k) % mpvss_ctx::SCALAR_RING];
    if (!c.in_use) { e = &c; ctx->scalar_seq += k + 1; }
  }
  if (!e) return fail(ctx, MPVSS_E_INVALID, "scalar side: too many concurrent calls on one context (16)");
  if (!e->done) HIPCHK(ctx, hipEventCreateWithFlags(&e->done, hipEventDisableTiming | hipEventBlockingSync));
  if (bytes > e->cap) {
    if (e->pin) HIPCHK(ctx, hipHostFree(e->pin));
    e->pin = nullptr;
    e->cap = 0;
    hipError_t rc = hipHostMalloc(&e->pin, bytes, hipHostMallocDefault);
    if (rc != hipSuccess) return fail(ctx, MPVSS_E_NOMEM, "hipHostMalloc(scalar staging)", rc);
    e->cap = bytes;
  }
  RET_IF(ensure(ctx, e->dev, bytes));
  e->in_use = true;
  *out = e;
  return 0;
}
// gives the entry back when the call leaves (the context lock is held whenever this runs), wiping `wipe_words` words of secrets
struct ScalarEntryGuard {
  mpvss_ctx::ScalarEntry* e;
  size_t wipe_words;
  mpvss_ctx* ctx = nullptr;
  ~ScalarEntryGuard() {
    // nothing may still read the staging when it is wiped and handed out again: on an error return between the upload and
    // this call's hipEventRecord(e->done) the event still belongs to an EARLIER call, so the stream itself is drained first
    // (a no-op after a call that waited for its event)
    if (ctx && ctx->scalar_stream) (void)hipStreamSynchronize(ctx->scalar_stream);
    if (e->done) (void)hipEventSynchronize(e->done);
    volatile uint32_t* wp = (volatile uint32_t*)e->pin;
    for (size_t i = 0; wp && i < wipe_words; ++i) wp[i] = 0;
    e->in_use = false;
  }
};
}  // namespace

/* Synchronous: the results are in HBM when the call returns. */
extern "C" int mpvss_modp_poly_eval_device(mpvss_ctx* ctx, const uint8_t* coeffs_host, size_t t, const int64_t* positions_dev,
                                           size_t n, uint8_t* out_dev) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  if (n == 0) return MPVSS_OK;
  if (!coeffs_host || !positions_dev || !out_dev || t == 0 || t > 0x7fffffff || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "poly_eval_device: bad argument (t must be >= 1)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  RET_IF(modq_consts(ctx));
  mpvss_ctx::ScalarEntry* e;
  RET_IF(scalar_entry(ctx, t * MODP_L * 4 + n * 8, &e));
  ScalarEntryGuard guard{e, t * MODP_L, ctx};                  // the coefficient limbs are wiped on every way out
  int par_even, par_odd;
  modq_poly_limbs(coeffs_host, t, (uint32_t*)e->pin, &par_even, &par_odd);
  int64_t* hp = (int64_t*)((uint8_t*)e->pin + t * MODP_L * 4);
  hipStream_t s = ctx->scalar_stream;
  HIPCHK(ctx, hipMemcpyAsync(e->dev.p, e->pin, t * MODP_L * 4, hipMemcpyHostToDevice, s));
  LAUNCHCHK(ctx, modq_launch_poly_eval((const uint32_t*)e->dev.p, (int)t, positions_dev, (int)n, par_even, par_odd, out_dev,
                                       ctx->consts_q, s));
  // positions are validated after the fact (a negative one is the caller's bug; the reference would panic)
  HIPCHK(ctx, hipMemcpyAsync(hp, positions_dev, n * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipEventRecord(e->done, s));
  lk.unlock();
  const hipError_t rc = hipEventSynchronize(e->done);
  lk.lock();
  if (rc != hipSuccess) return fail(ctx, MPVSS_E_DEVICE, "poly_eval_device: hipEventSynchronize", rc);
  for (size_t i = 0; i < n; ++i)
    if (hp[i] < 0) return fail(ctx, MPVSS_E_INVALID, "negative position (the reference panics: negative exponent)");
  return MPVSS_OK;
}

extern "C" int mpvss_modp_dleq_responses_device(mpvss_ctx* ctx, const uint8_t* w_dev, const uint8_t* alpha_dev, const uint8_t* c_host,
                                                size_t n, uint8_t* r_dev_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  if (n == 0) return MPVSS_OK;
  if (!w_dev || !alpha_dev || !c_host || !r_dev_out || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "dleq_responses_device: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  RET_IF(modq_consts(ctx));
  const hsc::Modulus<32>& M = modp_order();
  const hsc::Modulus<32>& Q = modp_subgroup_order();
  uint64_t c[32], neg[32];
  hsc::from_bytes<32>(c, c_host, true);
  M.reduce1(c);
  const int c_parity = (int)(c[0] & 1);
  Q.reduce1(c);
  bool zero = true;
  for (int i = 0; i < 32; ++i) zero = zero && c[i] == 0;
  if (zero) memset(neg, 0, sizeof(neg)); else hsc::sub_n<32>(neg, Q.m, c);       // -c mod q'
  mpvss_ctx::ScalarEntry* e;
  RET_IF(scalar_entry(ctx, EB, &e));
  ScalarEntryGuard guard{e, 0, ctx};
  hsc::to_bytes<32>((uint8_t*)e->pin, neg, true);
  hipStream_t s = ctx->scalar_stream;
  HIPCHK(ctx, hipMemcpyAsync(e->dev.p, e->pin, EB, hipMemcpyHostToDevice, s));
  LAUNCHCHK(ctx, modq_launch_responses(w_dev, alpha_dev, (const uint8_t*)e->dev.p, c_parity, (int)n, r_dev_out, ctx->consts_q, s));
  HIPCHK(ctx, hipEventRecord(e->done, s));
  lk.unlock();
  const hipError_t rc = hipEventSynchronize(e->done);
  lk.lock();
  if (rc != hipSuccess) return fail(ctx, MPVSS_E_DEVICE, "dleq_responses_device: hipEventSynchronize", rc);
  return MPVSS_OK;
}

// ---- the curve groups' pair on the device (kernels: verdict_kernels.hip k_ec_poly_eval / k_ec_responses) ---------------------
// Like the MODP calls above they run on the context's high-priority scalar stream and give the context lock back while they
// wait, so that a dealer's responses neither queue behind the boxes in flight nor hold up the threads that enqueue them.
extern "C" int mpvss_ec_poly_eval_device(mpvss_ctx* ctx, int group, const uint8_t* coeffs_host, size_t t, const int64_t* positions_dev,
                                         size_t n, uint8_t* out_dev) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  const EcInfo* gi = ec_info(group);
  if (!gi) return fail(ctx, MPVSS_E_UNSUPPORTED, "ec_poly_eval_device: unknown group");
  if (n == 0) return MPVSS_OK;
  if (!coeffs_host || !positions_dev || !out_dev || t == 0 || t > 0x7fffffff || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "ec_poly_eval_device: bad argument (t must be >= 1)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t cb = t * 32;
  mpvss_ctx::ScalarEntry* e;
  RET_IF(scalar_entry(ctx, 2 * cb, &e));                   // coefficient bytes | their Montgomery forms (device side)
  ScalarEntryGuard guard{e, (cb + 3) / 4, ctx};
  memcpy(e->pin, coeffs_host, cb);
  hipStream_t s = ctx->scalar_stream;
  HIPCHK(ctx, hipMemcpyAsync(e->dev.p, e->pin, cb, hipMemcpyHostToDevice, s));
  LAUNCHCHK(ctx, ec_scalar_launch_poly_eval(group, (const uint8_t*)e->dev.p, (int)t, positions_dev, (int)n,
                                            (uint32_t*)((uint8_t*)e->dev.p + cb), out_dev, s));
  HIPCHK(ctx, hipMemsetAsync(e->dev.p, 0, 2 * cb, s));      // the coefficients are the dealer's secret
  HIPCHK(ctx, hipEventRecord(e->done, s));
  lk.unlock();
  const hipError_t rc = hipEventSynchronize(e->done);
  lk.lock();
  if (rc != hipSuccess) return fail(ctx, MPVSS_E_DEVICE, "ec_poly_eval_device: hipEventSynchronize", rc);
  return MPVSS_OK;
}

extern "C" int mpvss_ec_dleq_responses_device(mpvss_ctx* ctx, int group, const uint8_t* w_dev, const uint8_t* alpha_dev,
                                              const uint8_t* c_host32, size_t n, uint8_t* r_dev_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  const EcInfo* gi = ec_info(group);
  if (!gi) return fail(ctx, MPVSS_E_UNSUPPORTED, "ec_dleq_responses_device: unknown group");
  if (n == 0) return MPVSS_OK;
  if (!w_dev || !alpha_dev || !c_host32 || !r_dev_out || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "ec_dleq_responses_device: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  mpvss_ctx::ScalarEntry* e;
  RET_IF(scalar_entry(ctx, 32, &e));
  ScalarEntryGuard guard{e, 0, ctx};
  memcpy(e->pin, c_host32, 32);
  hipStream_t s = ctx->scalar_stream;
  HIPCHK(ctx, hipMemcpyAsync(e->dev.p, e->pin, 32, hipMemcpyHostToDevice, s));
  LAUNCHCHK(ctx, ec_scalar_launch_responses(group, w_dev, alpha_dev, (const uint8_t*)e->dev.p, 0, (int)n, r_dev_out, s));
  HIPCHK(ctx, hipEventRecord(e->done, s));
  lk.unlock();
  const hipError_t rc = hipEventSynchronize(e->done);
  lk.lock();
  if (rc != hipSuccess) return fail(ctx, MPVSS_E_DEVICE, "ec_dleq_responses_device: hipEventSynchronize", rc);
  return MPVSS_OK;
}

// The dealer of participant.rs:160-286 in ONE call for a host application whose data lives in host memory: P(i), the group
// work, the transcript, the challenge and the responses -- everything after "draw the polynomial and the witnesses" and
// before "put the maps together" -- with the 2048-bit scalar arithmetic on the device as well.
// Any n (the reference has no size limit): the box is cut into blocks of at most MAX_CHUNK shares that run through the block
// pipeline two at a time (the GPU works on block k+1 while the host hashes block k) into ONE transcript; P(i) and the
// witnesses of every block stay in HBM until the challenge is known, then one kernel forms all responses.
// The call's inputs and intermediate secrets live in buffers of their own (mpvss_ctx::DealBufs, one set per deal in flight, from
// the context's pool) -- NOT in the shared workspace of the synchronous entry points, which other threads may use while this
// call has released the context lock to wait for and hash a block -- and P(i), the witnesses and the staged coefficient limbs
// are zeroed before the call returns.  Several host threads may deal on one context at once: every call owns its blocks by
// their numbers and absorbs exactly those.
namespace {
struct DealWipe {        // zero the secrets and give the buffers back whichever way the call ends (context lock held)
  mpvss_ctx* ctx;
  mpvss_ctx::DealBufs* dp;
  size_t n, t;
  ~DealWipe() {
    mpvss_ctx::DealBufs& d = *dp;
    if (d.pin) {
      volatile uint32_t* wp = (volatile uint32_t*)d.pin;
      for (size_t i = 0; i < d.pin_cap / 4; ++i) wp[i] = 0;
    }
    if (hipSetDevice(ctx->device) == hipSuccess) {
      if (d.p.p) (void)hipMemsetAsync(d.p.p, 0, d.p.cap < n * EB ? d.p.cap : n * EB, ctx->stream);
      if (d.w.p) (void)hipMemsetAsync(d.w.p, 0, d.w.cap < n * EB ? d.w.cap : n * EB, ctx->stream);
      if (d.coef.p) (void)hipMemsetAsync(d.coef.p, 0, d.coef.cap < t * MODP_L * 4 ? d.coef.cap : t * MODP_L * 4, ctx->stream);
      (void)hipStreamSynchronize(ctx->stream);
    }
    d.in_use = false;
  }
};
}  // namespace

extern "C" int mpvss_modp_deal(mpvss_ctx* ctx, const uint8_t* coeffs_host, size_t t, const int64_t* positions_host,
                               const uint8_t* pubkeys_host, const uint8_t* witnesses_host, size_t n, uint8_t* x_out, uint8_t* y_out,
                               uint8_t* a1_out, uint8_t* a2_out, uint8_t* digest32_out, uint8_t* challenge_out256, uint8_t* r_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  if (n == 0 || !coeffs_host || !positions_host || !pubkeys_host || !witnesses_host || !y_out || !r_out || t == 0 || t > 0x7fffffff ||
      n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "deal: bad argument (t >= 1, 1 <= n < 2^31)");
  if (t > n) return fail(ctx, MPVSS_E_INVALID, "deal: threshold > number of public keys (participant.rs:166)");
  RET_IF(check_positions_host(ctx, positions_host, n));
  HIPCHK(ctx, hipSetDevice(ctx->device));
  RET_IF(modq_consts(ctx));
  // cross-call key cache (mpvss_ctx_set_key_cache_lru): dealers to the same long-lived participants find the keys' tables built --
  // Y_i = y_i^P(i) and a2_i = y_i^w_i in 2 x 548 instead of 2 865 Montgomery operations per share
  const mpvss_keyset* cached = dealer_key_cache(ctx, lk, pubkeys_host, n);
  CacheUse cache_use{ctx, cached};
  mpvss_ctx::DealBufs* dbufs = ctx->deal_acquire();
  if (!dbufs) return fail(ctx, MPVSS_E_NOMEM, "deal: no buffers");
  mpvss_ctx::DealBufs& d = *dbufs;
  DealWipe wipe{ctx, dbufs, n, t};
  // MPVSS_TRACE_DEAL=1: where one call's time goes (stderr): staging | enqueue | wait + hash + copies | responses
  static const int trace_deal = fd_env("MPVSS_TRACE_DEAL", 0);
  const auto t_d0 = std::chrono::steady_clock::now();
  double t_marks[4] = {0, 0, 0, 0};
  auto dmark = [&](int k) { t_marks[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_d0).count(); };
  for (DevBuf* b : {&d.p, &d.w, &d.r}) RET_IF(ensure(ctx, *b, n * EB));
  if (!cached) RET_IF(ensure(ctx, d.keys, n * EB));
  RET_IF(ensure(ctx, d.pos, n * 8));
  RET_IF(ensure(ctx, d.coef, t * MODP_L * 4));
  RET_IF(ensure(ctx, d.c, EB));
  if (t * MODP_L * 4 > d.pin_cap) {
    if (d.pin) HIPCHK(ctx, hipHostFree(d.pin));
    d.pin = nullptr;
    d.pin_cap = 0;
    hipError_t rc = hipHostMalloc(&d.pin, t * MODP_L * 4, hipHostMallocDefault);
    if (rc != hipSuccess) return fail(ctx, MPVSS_E_NOMEM, "hipHostMalloc(deal staging)", rc);
    d.pin_cap = t * MODP_L * 4;
  }
  // the polynomial once per box: a'_j = a_j 2^(522 j) mod q' as limbs, the parities of P at even / odd positions
  int par_even, par_odd;
  modq_poly_limbs(coeffs_host, t, (uint32_t*)d.pin, &par_even, &par_odd);
  HIPCHK(ctx, hipMemcpyAsync(d.coef.p, d.pin, t * MODP_L * 4, hipMemcpyHostToDevice, ctx->stream));
  if (!cached) HIPCHK(ctx, hipMemcpyAsync(d.keys.p, pubkeys_host, n * EB, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d.w.p, witnesses_host, n * EB, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d.pos.p, positions_host, n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // the blocks' own streams read them next
  dmark(0);
  uint8_t state[MPVSS_TRANSCRIPT_STATE_BYTES];
  mpvss_transcript_init(state);
  // A dealer that has the chip to itself: the box in blocks, block k + 1 starting on the GPU when block k is done -- the dealer's kernels
  // are plain data-parallel launches (no latency chain like the verifier's X path), so blocks that fill every wave slot of the chip run
  // back to back at the whole box's rate and the transcript of block k is hashed while block k + 1 computes: only the last block's hash
  // stays behind the GPU work.  With key tables 32768 shares fill the chip (two exponent sets = 1024 workgroups): one call at
  // (65536, 256) 70 -> 56 ms.  The bucket kernels need 65536 shares for two waves per SIMD (a half box takes 44 of the whole box's 52 ms:
  // measured, no gain), so without key tables only boxes of 131072 shares and more are cut, into blocks of 65536 (262144 shares: 414 ms in
  // blocks of 32768, 317-338 ms in blocks of 65536; profiles/r06_lone_dealer_blocks.txt).  Dealers that share the chip keep whole blocks: their hashes hide behind each other's work.
  const size_t LONE_BLOCK = cached ? 32768 : 65536;
  const bool chained = !ctx->busy_with_others() && n >= 2 * LONE_BLOCK && MAX_CHUNK >= LONE_BLOCK;
  const size_t BLK = chained ? LONE_BLOCK : MAX_CHUNK;
  const size_t nblk = (n + BLK - 1) / BLK;
  std::vector<unsigned long long> blk_pos;                   // this call's blocks by their numbers in the ring
  blk_pos.reserve(nblk);
  auto absorb = [&](size_t b) -> int {
    const size_t off = b * BLK;
    return verify_block_absorb_locked(ctx, lk, state, x_out ? x_out + off * EB : nullptr, a1_out ? a1_out + off * EB : nullptr,
                                      a2_out ? a2_out + off * EB : nullptr, y_out + off * EB, &blk_pos[b], true);
  };
  int rc = MPVSS_OK;
  size_t enq = 0, done = 0;
  for (; enq < nblk && rc == MPVSS_OK; ++enq) {
    const size_t off = enq * BLK, cnt = (n - off < BLK) ? n - off : BLK;
    // (the block before this one is still in its slot: it is absorbed below, after this one is enqueued)
    hipEvent_t after = (chained && enq >= 1) ? ctx->ring_slot((unsigned)blk_pos[enq - 1]).done : nullptr;
    const DealPoly poly{nullptr, t, (const int64_t*)d.pos.p + off, (uint8_t*)d.p.p + off * EB, (const uint32_t*)d.coef.p, par_even, par_odd};
    rc = wait_for_room(ctx, lk);
    if (rc == MPVSS_OK)
      rc = distribute_block_compute_locked(ctx, MPVSS_DEVICE, nullptr, 0, nullptr, cached ? nullptr : (const uint8_t*)d.keys.p + off * EB,
                                           (const uint8_t*)d.p.p + off * EB, (const uint8_t*)d.w.p + off * EB, cnt, nullptr, nullptr,
                                           nullptr, nullptr, &poly, cached, off, after);
    if (rc == MPVSS_OK) blk_pos.push_back(ctx->own_last(1));
    if (rc == MPVSS_OK && enq >= 1) rc = absorb(done++);     // block enq runs on the GPU while block enq - 1 is hashed
  }
  if (rc != MPVSS_OK) {                                      // drain what was enqueued: nothing of this call stays in the ring
    const std::string why = ctx->err;
    uint8_t scrap[MPVSS_TRANSCRIPT_STATE_BYTES];
    mpvss_transcript_init(scrap);
    for (size_t b = 0; b < blk_pos.size(); ++b)
      if (ctx->ring_slot((unsigned)blk_pos[b]).busy && !ctx->ring_slot((unsigned)blk_pos[b]).absorbing)
        (void)verify_block_absorb_locked(ctx, lk, scrap, nullptr, nullptr, nullptr, nullptr, &blk_pos[b], true);
    { std::lock_guard<std::mutex> g(ctx->err_mu); ctx->err = why; }
    return rc;
  }
  dmark(1);
  while (done < nblk) RET_IF(absorb(done++));
  dmark(2);
  uint8_t digest[32], challenge[EB];
  {
    mpvss::Sha256 tr;
    memcpy(&tr, state, sizeof(tr));
    tr.final(digest);                                        // participant.rs:251: the dealer's transcript digest
  }
  mpvss_modp_hash_to_scalar(digest, 32, challenge);          // :251-252
  if (digest32_out) memcpy(digest32_out, digest, 32);
  if (challenge_out256) memcpy(challenge_out256, challenge, EB);
  // r_i = w_i - P(i) c                                       participant.rs:255-264, dleq.rs:42-50
  {
    const hsc::Modulus<32>& Q = modp_subgroup_order();
    uint64_t c[32], neg[32];
    hsc::from_bytes<32>(c, challenge, true);                 // below 2^256 < (q-1)/2: already reduced
    bool zero = true;
    for (int i = 0; i < 32; ++i) zero = zero && c[i] == 0;
    if (zero) memset(neg, 0, sizeof(neg)); else hsc::sub_n<32>(neg, Q.m, c);
    uint8_t cneg[EB];
    hsc::to_bytes<32>(cneg, neg, true);
    HIPCHK(ctx, hipMemcpy(d.c.p, cneg, EB, hipMemcpyHostToDevice));
    LAUNCHCHK(ctx, modq_launch_responses((const uint8_t*)d.w.p, (const uint8_t*)d.p.p, (const uint8_t*)d.c.p,
                                         (int)(challenge[EB - 1] & 1), (int)n, (uint8_t*)d.r.p, ctx->consts_q, ctx->stream));
  }
  HIPCHK(ctx, hipMemcpyAsync(r_out, d.r.p, n * EB, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  dmark(3);
  if (trace_deal)
    fprintf(stderr, "[mpvss] deal n=%zu t=%zu: staging %.1f | enqueue (last block, incl. absorbing the blocks before) %.1f | wait + hash + copies %.1f | "
            "challenge + responses + copy %.1f ms (pipeline: wait %.1f, hash %.1f)\n", n, t, t_marks[0], t_marks[1] - t_marks[0],
            t_marks[2] - t_marks[1], t_marks[3] - t_marks[2], ctx->pstats.wait_ms, ctx->pstats.hash_ms);
  return MPVSS_OK;
}

extern "C" int mpvss_ec_poly_eval(int group, const uint8_t* coeffs, size_t t, const int64_t* positions, size_t n, uint8_t* out,
                                  int threads) {
  const EcInfo* gi = ec_info(group);
  if (!gi) return MPVSS_E_UNSUPPORTED;
  if (n == 0) return MPVSS_OK;
  if (!coeffs || !positions || !out || t == 0) return MPVSS_E_INVALID;
  poly_eval_bytes<4>(ec_order(gi), gi->scalar_be, coeffs, t, positions, n, out, host_threads(threads));
  return MPVSS_OK;
}

// ---- reconstruct (src/participant.rs:462-561 MODP, 1452-1557 secp256k1, 1895-2002 ristretto255) -----------------------
// G^s = prod_i S_i^lambda_i from m decrypted shares at pairwise different positions: the Lagrange coefficients in
// the scalar field on the host (the reference's integer num/den of util.rs:47-64 reduce to the same residues), the
// m exponentiations and their product on the GPU.  Outputs G^s (encoded) and the mask the reference XORs onto U:
// int_BE(SHA256(bytes(G^s))) reduced as the group's code does (mod q: identity on 256 bits; secp256k1: mod n;
// ristretto255: mod l), 32 bytes big-endian.
namespace {

// product of m elements (device bytes) by pairwise rounds; result in buf[0..256)
int modp_product_tree(mpvss_ctx* ctx, uint8_t* buf, size_t m) {
  while (m > 1) {
    const size_t half = m / 2;
    LAUNCHCHK(ctx, modp_launch_mul(buf, buf + half * EB, buf, (int)half, ctx->consts, ctx->stream));
    if (m & 1) {
      HIPCHK(ctx, hipMemcpyAsync(buf + half * EB, buf + (m - 1) * EB, EB, hipMemcpyDeviceToDevice, ctx->stream));
      m = half + 1;
    } else {
      m = half;
    }
  }
  return 0;
}

}  // namespace

extern "C" int mpvss_modp_reconstruct(mpvss_ctx* ctx, int space, const int64_t* positions_host, const uint8_t* shares, size_t m,
                                      uint8_t* gs_out256, uint8_t* mask_out32) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!positions_host || !shares || m == 0 || !gs_out256 || m > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "reconstruct: bad argument");
  // util.rs:47-64 only multiplies positions j >= 1 into the coefficient: other positions are outside its domain
  for (size_t i = 0; i < m; ++i)
    if (positions_host[i] < 1) return fail(ctx, MPVSS_E_INVALID, "reconstruct: positions must be >= 1 (util.rs:47-64)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  spans_reset(ctx);
  std::vector<hsc::Num<32>> mag;
  std::vector<char> neg;
  if (!lagrange_at_zero<32>(modp_subgroup_order(), positions_host, m, mag, neg, false))
    return fail(ctx, MPVSS_E_INVALID, "reconstruct: duplicate positions");
  // exponent: e = num/den mod (q-1)/2 for a positive coefficient (participant.rs:540-548); a negative coefficient
  // inverts the factor (:551-553), and S^-e = S^((q-1) - e) for every unit S -- the same element, no inversion
  std::vector<uint8_t> exps(m * EB);
  for (size_t i = 0; i < m; ++i) {
    uint64_t e[32];
    memcpy(e, mag[i].v, sizeof(e));
    if (neg[i]) {
      bool zero = true;
      for (int k = 0; k < 32; ++k) zero = zero && e[k] == 0;
      if (!zero) hsc::sub_n<32>(e, modp_order().m, e);
    }
    hsc::to_bytes<32>(exps.data() + i * EB, e, true);
  }
  const void* dS;
  RET_IF(stage_in(ctx, space, shares, m * EB, ctx->w->in_a, &dS));
  RET_IF(ensure(ctx, ctx->w->in_b, m * EB));
  HIPCHK(ctx, hipMemcpyAsync(ctx->w->in_b.p, exps.data(), m * EB, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // exps is pageable host memory of this call
  RET_IF(ensure(ctx, ctx->w->out1, m * EB));
  uint8_t* dF = (uint8_t*)ctx->w->out1.p;
  RET_IF(exp_dev(ctx, (const uint8_t*)dS, (const uint8_t*)ctx->w->in_b.p, m, dF));      // S_i^lambda_i
  RET_IF(modp_product_tree(ctx, dF, m));                                               // fold with mul, :503-505
  uint8_t gs[EB];
  HIPCHK(ctx, hipMemcpyAsync(gs, dF, EB, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  // a share that is 0 mod q has no inverse: the reference returns None when its coefficient is negative (:551-553)
  {
    std::vector<uint8_t> hs;
    RET_IF(small_vec_to_host(ctx, space, shares, m * EB, hs));
    uint8_t qbe[EB];
    hsc::to_bytes<32>(qbe, modp_order().m, true);
    qbe[EB - 1] |= 1;                                        // q = (q - 1) + 1, q - 1 is even
    for (size_t i = 0; i < m; ++i) {
      bool zero = true, is_q = true;
      for (size_t k = 0; k < EB; ++k) { zero = zero && hs[i * EB + k] == 0; is_q = is_q && hs[i * EB + k] == qbe[k]; }
      if ((zero || is_q) && neg[i]) return fail(ctx, MPVSS_E_INVALID, "reconstruct: a share is 0 mod q and has no inverse");
    }
  }
  memcpy(gs_out256, gs, EB);
  if (mask_out32) {
    mpvss::Sha256 h;
    frame_min_bytes_update(h, gs);                           // SHA256(element_to_bytes(G^s)): minimal-length bytes, no length prefix
    h.final(mask_out32);                                     // < 2^256 < q: `mod q` is the identity (:512-515)
  }
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}

namespace {

// lambda_i of a position list as the 32-byte scalar the kernels multiply a share by: |lambda_i| mod the order, the order's
// complement for a negative non-zero coefficient (-(lambda S) = (order - lambda) S, participant.rs:1546-1555), in the group's scalar
// byte order.  False: duplicate positions.  One place for the one-secret call and for mpvss_ec_reconstruct_many.
bool ec_lagrange_scalar(const EcInfo* gi, const int64_t* pos, size_t m, size_t i, uint8_t* out32) {
  uint64_t e[4];
  char neg = 0;
  if (!lagrange_coefficient_at_zero<4>(ec_order(gi), pos, m, i, e, &neg)) return false;
  if (neg && (e[0] | e[1] | e[2] | e[3])) hsc::sub_n<4>(e, ec_order(gi).m, e);
  hsc::to_bytes<4>(out32, e, gi->scalar_be);
  return true;
}
// SHA256(bytes(G^s)) as a big-endian integer, reduced mod the group order (participant.rs:1495-1508, 1939-1946);
// secp256k1's Scalar::from_repr(...).unwrap() panics for a digest >= n (p ~ 2^-128): reduced here instead
void ec_secret_mask(const EcInfo* gi, const uint8_t* gs, uint8_t* mask_out32) {
  uint8_t h[32];
  mpvss::sha256(gs, gi->enc, h);
  uint64_t x[4];
  hsc::from_bytes<4>(x, h, true);
  ec_order(gi).reduce1(x);
  hsc::to_bytes<4>(mask_out32, x, true);
}

// ---- the same scalars on the device (DESIGN section 13, "Lagrange coefficients on the device, curve groups") --------------------
// One list longer than this keeps the host path: its one launch would run for seconds on a shared machine.  Nobody has measured
// that size; the value is a guess at "seconds", not a crossover.
constexpr size_t EC_LAGRANGE_DEVICE_MAX_M = (size_t)1 << 20;
// Mode 1 of mpvss_ctx_set_ec_lagrange takes the device for a call whose work -- the sum of m^2 over its distinct position lists, m^2
// of a lone secret -- is at least this.  Set from tools/ec_reconstruct_many.py --lagrange against a build of the parent commit
// (profiles/ec_lagrange_device.txt): the smallest measured work from which the device is not slower than the parent beyond the
// spread of the parent's three runs, on both curves and in both spaces.  That is 200 secrets of 34 shares with a list each,
// 200 x 34^2 (2.0 against 2.9 ms); every measured shape above it is faster on the device (60 x 1024 over one list 3.3 against
// 5.1 ms, with a list each 3.5 against 170 ms), the three below it -- 9, 1 156 and 3 600 -- are 0.5 to 0.7 ms slower: the
// launch costs the latency of one Fermat inversion whatever its size.  Nothing between 3 600 and 231 200 is measured: automatic
// stays on the host there.
constexpr double EC_LAGRANGE_DEVICE_MIN_WORK = 200.0 * 34 * 34;

bool ec_lagrange_on_device(const mpvss_ctx* ctx, double work, size_t longest, size_t coefs) {
  // (tile rows hold positions' and coefficients' indices in 32 bits)
  if (ctx->ec_lagrange_mode == 0 || longest > EC_LAGRANGE_DEVICE_MAX_M || coefs > 0x7fffffffu) return false;
  return ctx->ec_lagrange_mode == 2 || work >= EC_LAGRANGE_DEVICE_MIN_WORK;
}
// duplicates by sorting a copy, O(m log m): what the quadratic host loop finds on its way
bool ec_positions_distinct(const int64_t* pos, size_t m) {
  std::vector<int64_t> s(pos, pos + m);
  std::sort(s.begin(), s.end());
  return std::adjacent_find(s.begin(), s.end()) == s.end();
}
// `total` positions (the launch's lists back to back) and the tile rows up, then ONE k_ec_lagrange launch into out_dev (32 bytes
// per position).  The copies are asynchronous: positions and tiles stay alive until the caller has drained the stream.
int ec_lagrange_dev(mpvss_ctx* ctx, const EcInfo* gi, DevBuf& pos_buf, DevBuf& tile_buf, const int64_t* positions, size_t total,
                    const std::vector<uint32_t>& tiles, uint8_t* out_dev) {
  RET_IF(ensure(ctx, pos_buf, total * 8));
  RET_IF(ensure(ctx, tile_buf, tiles.size() * 4));
  HIPCHK(ctx, hipMemcpyAsync(pos_buf.p, positions, total * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(tile_buf.p, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  TIMED_LAUNCH(ctx, 4, ec_lagrange_launch(gi->group, (const int64_t*)pos_buf.p, (const uint32_t*)tile_buf.p, (int)(tiles.size() / 4),
                                          out_dev, ctx->stream));
  return MPVSS_OK;
}
struct StreamDrainIf {          // StreamDrain for a path that is only sometimes asynchronous
  mpvss_ctx* c;
  bool on = false;
  ~StreamDrainIf() { if (on) (void)hipStreamSynchronize(c->stream); }
};

// one secret under the context lock (mpvss_ec_reconstruct, and the one-secret path of mpvss_ec_reconstruct_many).  The m scalars of
// ec_lagrange_scalar when the caller has them already (computed with the call's other position lists): scalars_pre in host memory
// or scalars_dev in device memory; else both null, and they are computed here, on the host or on the device.
int ec_reconstruct_locked(mpvss_ctx* ctx, const EcInfo* gi, EcWork& w, int space, const int64_t* positions_host, const uint8_t* shares,
                          size_t m, uint8_t* gs_out, uint8_t* mask_out32, const uint8_t* scalars_pre, const uint8_t* scalars_dev = nullptr) {
  const int group = gi->group;
  if (!positions_host || !shares || m == 0 || !gs_out || m > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "ec_reconstruct: bad argument");
  // a box's positions are 1..n (participant.rs:1127, 1600); the coefficient of a position <= 0 would multiply `j as u64` into
  // the numerator and the signed difference into the denominator, which is no Lagrange coefficient: refused as for MODP
  for (size_t i = 0; i < m; ++i)
    if (positions_host[i] < 1) return fail(ctx, MPVSS_E_INVALID, "ec_reconstruct: positions must be >= 1");
  // lambda * S, negated for a negative coefficient (participant.rs:1546-1555)
  std::vector<uint8_t> ks;
  std::vector<uint32_t> tiles;
  StreamDrainIf drain{ctx, scalars_dev != nullptr};          // (after the host sources of the device path's copies)
  const uint8_t* dK = scalars_dev;
  if (!scalars_pre && !scalars_dev) {
    if (ec_lagrange_on_device(ctx, (double)m * (double)m, m, m)) {
      if (!ec_positions_distinct(positions_host, m)) return fail(ctx, MPVSS_E_INVALID, "ec_reconstruct: duplicate positions");
      ec::lagrange_tiles(0, m, tiles);
      RET_IF(ensure(ctx, w.d, m * 32));
      drain.on = true;
      RET_IF(ec_lagrange_dev(ctx, gi, w.lag_pos, w.lag_tiles, positions_host, m, tiles, (uint8_t*)w.d.p));   // straight into ec_dual's scalars
      dK = (const uint8_t*)w.d.p;
      ++ctx->ec_lagrange_dev_lists;
    } else {
      ks.resize(m * 32);
      for (size_t i = 0; i < m; ++i)
        if (!ec_lagrange_scalar(gi, positions_host, m, i, ks.data() + i * 32)) return fail(ctx, MPVSS_E_INVALID, "ec_reconstruct: duplicate positions");
      scalars_pre = ks.data();
      ++ctx->ec_lagrange_host_lists;
    }
  }
  const void* dS;
  RET_IF(stage_in(ctx, space, shares, m * gi->enc, w.a, &dS));
  if (!dK) {
    RET_IF(ensure(ctx, w.d, m * 32));
    HIPCHK(ctx, hipMemcpyAsync(w.d.p, scalars_pre, m * 32, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    dK = (const uint8_t*)w.d.p;
  }
  RET_IF(ensure(ctx, w.ok, m > 4096 ? m : 4096));
  RET_IF(ensure(ctx, w.o1, (m + 1) * gi->enc));
  EcBase b1;
  b1.enc = (const uint8_t*)dS;
  b1.enc_stride = gi->enc;
  uint8_t* dF = (uint8_t*)w.o1.p;
  RET_IF(ec_dual(ctx, gi, b1, dK, 32, nullptr, nullptr, 0, m, w.tab1, w.tab2, w.p1, dF, (uint8_t*)w.ok.p, nullptr));
  // sum of the m factors (fold with Group::mul, participant.rs:1489-1492): one workgroup over the internal points
  LAUNCHCHK(ctx, ec_launch_sum(group, (const uint32_t*)w.p1.p, (int)m, (uint32_t*)w.p1.p, ctx->stream));
  LAUNCHCHK(ctx, ec_launch_encode(group, (const uint32_t*)w.p1.p, 1, dF, ctx->stream));
  uint8_t gs[33];
  HIPCHK(ctx, hipMemcpyAsync(gs, dF, gi->enc, hipMemcpyDeviceToHost, ctx->stream));
  RET_IF(ec_check_ok(ctx, (const uint8_t*)w.ok.p, m, "ec_reconstruct shares"));
  memcpy(gs_out, gs, gi->enc);
  if (mask_out32) ec_secret_mask(gi, gs, mask_out32);
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}

}  // namespace

extern "C" int mpvss_ec_reconstruct(mpvss_ctx* ctx, int group, int space, const int64_t* positions_host, const uint8_t* shares,
                                    size_t m, uint8_t* gs_out, uint8_t* mask_out32) {
  EC_PROLOGUE("ec_reconstruct");
  return ec_reconstruct_locked(ctx, gi, w, space, positions_host, shares, m, gs_out, mask_out32, nullptr);
}

// =====================================================================================================================
// Many secrets of a curve group in one call (DESIGN section 13, "Many secrets in one call, curve groups"):
// mpvss_ec_reconstruct_many, the curve counterpart of mpvss_modp_group_reconstruct_many (capi_modp_rt.inc).  One secret per call is
// a quadratic Lagrange loop on one host thread, two synchronisations and three launches of one partial workgroup each; here the
// coefficients are computed once per distinct position list on the call's host threads, and runs of secrets travel as ONE dense
// concatenation of shares through the launches of one secret, the fold replaced by one k_*_sum_segments launch (one wave per
// secret).  The plan of the position lists and the walk that forms the passes: many::plan_secrets, many::walk_secrets (host_many.h).
// =====================================================================================================================
namespace {

// shares of one secret that may travel in a pass (the project's RT_GROUP_BOX_MAX; DESIGN section 13 has the measurement it rests on)
constexpr size_t EC_GROUP_SECRET_MAX = 16384;

// a grouped pass: the secrets run[0 .. B) (indices into `secrets`, all many::SECRET_GROUPED), S <= MAX_CHUNK shares in all.  The
// launches of one secret over the concatenation -- the S factors are never encoded -- then one sum per secret into B dense points,
// one encode of those and one synchronisation.  A secret with a share that is no valid encoding is refused here: its sum ran with
// the others and is dropped.
int ec_reconstruct_pass(mpvss_ctx* ctx, const EcInfo* gi, EcWork& w, int space, const mpvss_ec_secret* secrets,
                        const std::vector<size_t>& run, const std::vector<many::SecretPlan>& plan, const uint8_t* scalars,
                        const uint8_t* scalars_dev, int host_threads, int* status, uint8_t* gs_out, uint8_t* masks_out32) {
  const int group = gi->group;
  const size_t B = run.size(), L = gi->enc;
  std::vector<uint32_t> segs(2 * B);                                // {first factor, m} of every secret
  size_t S = 0;
  for (size_t k = 0; k < B; ++k) {
    segs[2 * k] = (uint32_t)S;
    segs[2 * k + 1] = (uint32_t)secrets[run[k]].m;
    S += secrets[run[k]].m;
  }
  // host sources of asynchronous copies and the results read back: declared before the guard, whose way out drains the stream
  std::vector<uint8_t> g_sh, g_k(scalars_dev ? 0 : S * 32), h_enc(B * L), h_ok(S);
  std::vector<const uint8_t*> srcs, ksrcs;
  StreamDrain drain{ctx};
  spans_reset(ctx);
  if (!scalars_dev)
    for (size_t k = 0; k < B; ++k) memcpy(g_k.data() + (size_t)segs[2 * k] * 32, scalars + plan[run[k]].coef * 32, secrets[run[k]].m * 32);
  RET_IF(ensure(ctx, w.a, S * L));
  RET_IF(ensure(ctx, w.b, segs.size() * 4));
  RET_IF(ensure(ctx, w.d, S * 32));
  RET_IF(ensure(ctx, w.ok, S > 4096 ? S : 4096));
  RET_IF(ensure(ctx, w.p2, B * (size_t)ec_point_words(group) * 4));
  RET_IF(ensure(ctx, w.o1, (B + 1) * L));
  HIPCHK(ctx, hipMemcpyAsync(w.b.p, segs.data(), segs.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (space == MPVSS_HOST) {
    g_sh.resize(S * L);
    for (size_t k = 0; k < B; ++k) memcpy(g_sh.data() + (size_t)segs[2 * k] * L, secrets[run[k]].shares, secrets[run[k]].m * L);
    HIPCHK(ctx, hipMemcpyAsync(w.a.p, g_sh.data(), S * L, hipMemcpyHostToDevice, ctx->stream));
  } else {                  // every secret's shares lie in a device buffer of their own: one gather launch, not B copies
    srcs.resize(B);
    for (size_t k = 0; k < B; ++k) srcs[k] = secrets[run[k]].shares;
    RET_IF(ensure(ctx, w.c, B * sizeof(const uint8_t*)));
    HIPCHK(ctx, hipMemcpyAsync(w.c.p, srcs.data(), B * sizeof(const uint8_t*), hipMemcpyHostToDevice, ctx->stream));
    LAUNCHCHK(ctx, ec_launch_gather_segments((const uint8_t* const*)w.c.p, (const uint32_t*)w.b.p, (int)B, (uint32_t)L, (uint8_t*)w.a.p,
                                             ctx->stream));
  }
  if (scalars_dev) {        // the coefficients never left the device: the same gather, from the call's coefficient buffer
    ksrcs.resize(B);
    for (size_t k = 0; k < B; ++k) ksrcs[k] = scalars_dev + plan[run[k]].coef * 32;
    RET_IF(ensure(ctx, w.lag_src, B * sizeof(const uint8_t*)));
    HIPCHK(ctx, hipMemcpyAsync(w.lag_src.p, ksrcs.data(), B * sizeof(const uint8_t*), hipMemcpyHostToDevice, ctx->stream));
    LAUNCHCHK(ctx, ec_launch_gather_segments((const uint8_t* const*)w.lag_src.p, (const uint32_t*)w.b.p, (int)B, 32, (uint8_t*)w.d.p, ctx->stream));
  } else {
    HIPCHK(ctx, hipMemcpyAsync(w.d.p, g_k.data(), S * 32, hipMemcpyHostToDevice, ctx->stream));
  }
  EcBase b1;
  b1.enc = (const uint8_t*)w.a.p;
  b1.enc_stride = L;
  RET_IF(ec_dual(ctx, gi, b1, (const uint8_t*)w.d.p, 32, nullptr, nullptr, 0, S, w.tab1, w.tab2, w.p1, nullptr, (uint8_t*)w.ok.p, nullptr));
  LAUNCHCHK(ctx, ec_launch_sum_segments(group, (const uint32_t*)w.p1.p, (const uint32_t*)w.b.p, (int)B, (uint32_t*)w.p2.p, ctx->stream));
  LAUNCHCHK(ctx, ec_launch_encode(group, (const uint32_t*)w.p2.p, (int)B, (uint8_t*)w.o1.p, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(h_enc.data(), w.o1.p, B * L, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(h_ok.data(), w.ok.p, S, hipMemcpyDeviceToHost, ctx->stream));
  RET_IF(spans_collect(ctx));                                       // the pass's one synchronisation
  std::vector<char> refused(B, 0);
  size_t good = 0;
  for (size_t k = 0; k < B; ++k) {
    const uint8_t* ok = h_ok.data() + segs[2 * k];
    refused[k] = std::find(ok, ok + segs[2 * k + 1], 0) != ok + segs[2 * k + 1];
    if (!refused[k]) ++good;
  }
  hsc::parallel_for(B, many::many_threads(host_threads, B, 256), [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      if (refused[k]) continue;
      const size_t i = run[k];
      memcpy(gs_out + i * L, h_enc.data() + k * L, L);
      if (masks_out32) ec_secret_mask(gi, h_enc.data() + k * L, masks_out32 + 32 * i);
      status[i] = MPVSS_OK;
    }
  });
  if (good) {
    ++ctx->ec_rec_passes;
    ctx->ec_rec_grouped_secrets += good;
  }
  return MPVSS_OK;
}

}  // namespace

extern "C" int mpvss_ec_reconstruct_many(mpvss_ctx* ctx, int group, int space, const mpvss_ec_secret* secrets, size_t count,
                                         int host_threads, int* status, uint8_t* gs_out, uint8_t* masks_out32) {
  EC_PROLOGUE("ec_reconstruct_many");
  if (count == 0) return MPVSS_OK;
  if (!secrets || !status || !gs_out) return fail(ctx, MPVSS_E_INVALID, "ec_reconstruct_many: bad argument");
  const size_t L = gi->enc;
  // a refused secret has no result: its status, zeros in gs and in its mask.  Every secret is refused until it has its result.
  for (size_t i = 0; i < count; ++i) status[i] = MPVSS_E_INVALID;
  memset(gs_out, 0, count * L);
  if (masks_out32) memset(masks_out32, 0, 32 * count);

  // the Lagrange scalars ONCE per distinct position list (a list without them has duplicate positions: its secrets are refused):
  // on the host threads of the call, or by ONE k_ec_lagrange launch over all lists into a buffer the passes gather from
  many::SecretPlans lists = many::plan_lists(secrets, count, EC_GROUP_SECRET_MAX, MAX_CHUNK);
  double work = 0;
  for (const size_t lm : lists.list_m) work += (double)lm * (double)lm;
  const bool on_device = !lists.list_m.empty() &&
                         ec_lagrange_on_device(ctx, work, *std::max_element(lists.list_m.begin(), lists.list_m.end()), lists.coefs);
  std::vector<uint8_t> scalars;
  std::vector<int64_t> all_pos;                               // host sources of the launch's copies: before the guard
  std::vector<uint32_t> tiles;
  StreamDrainIf drain{ctx, on_device};
  const uint8_t* scalars_dev = nullptr;
  ctx->call_spans.spans.clear();
  ctx->call_spans.ev_used = 0;
  if (on_device) {
    std::vector<char> list_ok(lists.list_m.size(), 0);
    hsc::parallel_for(list_ok.size(), many::many_threads(host_threads, lists.coefs, 4096), [&](size_t lo, size_t hi) {
      for (size_t l = lo; l < hi; ++l) list_ok[l] = ec_positions_distinct(lists.list_pos[l], lists.list_m[l]) ? 1 : 0;
    });
    many::plan_settle(lists, list_ok);
    all_pos.resize(lists.coefs);
    size_t good = 0;
    for (size_t l = 0; l < list_ok.size(); ++l) {             // coefficient c belongs to position c; a refused list has no tile
      memcpy(all_pos.data() + lists.list_first[l], lists.list_pos[l], lists.list_m[l] * 8);
      if (!list_ok[l]) continue;
      ec::lagrange_tiles(lists.list_first[l], lists.list_m[l], tiles);
      ++good;
    }
    if (good) {
      RET_IF(ensure(ctx, w.lag_coef, lists.coefs * 32));
      ctx->sp = &ctx->call_spans;
      const int rc = ec_lagrange_dev(ctx, gi, w.lag_call_pos, w.lag_call_tiles, all_pos.data(), lists.coefs, tiles, (uint8_t*)w.lag_coef.p);
      ctx->sp = &ctx->main_spans;
      RET_IF(rc);
      ctx->ec_lagrange_dev_lists += good;
    }
    scalars_dev = (const uint8_t*)w.lag_coef.p;
  } else {
    many::plan_host_coefficients(lists, host_threads, [&](size_t coefs) { scalars.resize(coefs * 32); },
                                 [&](const int64_t* pos, size_t m, size_t j, size_t c) { return ec_lagrange_scalar(gi, pos, m, j, scalars.data() + c * 32); });
    std::vector<char> counted(lists.list_m.size(), 0);
    for (size_t i = 0; i < count; ++i)
      if (lists.secret[i].kind == many::SECRET_GROUPED && !counted[lists.list_of[i]]) {
        counted[lists.list_of[i]] = 1;
        ++ctx->ec_lagrange_host_lists;
      }
  }
  const std::vector<many::SecretPlan>& plan = lists.secret;
  // A code of the one-secret path other than MPVSS_E_INVALID (which refuses that secret alone) ends the call.
  auto single = [&](size_t i) -> int {
    const mpvss_ec_secret& s = secrets[i];
    spans_reset(ctx);
    const bool pre = plan[i].coef != (size_t)-1;             // a run of one: its list's scalars are there already
    const int rc = ec_reconstruct_locked(ctx, gi, w, space, s.positions_host, s.shares, s.m, gs_out + i * L,
                                         masks_out32 ? masks_out32 + 32 * i : nullptr,
                                         pre && !scalars_dev ? scalars.data() + plan[i].coef * 32 : nullptr,
                                         pre && scalars_dev ? scalars_dev + plan[i].coef * 32 : nullptr);
    if (rc == MPVSS_E_INVALID) {                            // (nothing of a refused secret stays in its outputs)
      memset(gs_out + i * L, 0, L);
      if (masks_out32) memset(masks_out32 + 32 * i, 0, 32);
      return MPVSS_OK;
    }
    RET_IF(rc);
    status[i] = MPVSS_OK;
    ++ctx->ec_rec_single_secrets;
    return MPVSS_OK;
  };
  RET_IF(many::walk_secrets(secrets, plan, MAX_CHUNK, single, [&](const std::vector<size_t>& run) {
    return ec_reconstruct_pass(ctx, gi, w, space, secrets, run, plan, scalars.data(), scalars_dev, host_threads, status, gs_out, masks_out32);
  }));
  if (!ctx->call_spans.spans.empty()) {                       // the coefficient launch among the kernel times of the call's last pass
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->call_spans.spans[0].a, ctx->call_spans.spans[0].b));
    ctx->kernel_ms[4] = ms;
    ctx->kernel_launches[4] = 1;
  }
  return MPVSS_OK;
}

extern "C" int mpvss_ec_reconstruct_many_stats(mpvss_ctx* ctx, unsigned long long* passes, unsigned long long* grouped_secrets,
                                               unsigned long long* single_secrets) {
  return many_stats(ctx, &mpvss_ctx::ec_rec_passes, &mpvss_ctx::ec_rec_grouped_secrets, &mpvss_ctx::ec_rec_single_secrets, passes,
                    grouped_secrets, single_secrets);
}

// ---- where the Lagrange coefficients of the curve groups are computed, and the kernel on its own ---------------------------------
extern "C" int mpvss_ctx_set_ec_lagrange(mpvss_ctx* ctx, int mode) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (mode < 0 || mode > 2) return fail(ctx, MPVSS_E_INVALID, "set_ec_lagrange: mode is 0, 1 or 2");
  const int before = ctx->ec_lagrange_mode;
  ctx->ec_lagrange_mode = mode;
  return before;
}

extern "C" int mpvss_ec_lagrange_stats(mpvss_ctx* ctx, unsigned long long* device_lists, unsigned long long* host_lists) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (device_lists) *device_lists = ctx->ec_lagrange_dev_lists;
  if (host_lists) *host_lists = ctx->ec_lagrange_host_lists;
  return MPVSS_OK;
}

extern "C" int mpvss_ec_lagrange_scalars(mpvss_ctx* ctx, int group, const int64_t* positions_host, size_t m, uint8_t* scalars_out_host) {
  EC_PROLOGUE("ec_lagrange_scalars");
  if (!positions_host || !scalars_out_host || m == 0 || m > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "ec_lagrange_scalars: bad argument");
  for (size_t i = 0; i < m; ++i)
    if (positions_host[i] < 1) return fail(ctx, MPVSS_E_INVALID, "ec_lagrange_scalars: positions must be >= 1");
  std::vector<uint8_t> ks(m * 32);                           // the output stays untouched by a refused call
  std::vector<uint32_t> tiles;
  StreamDrainIf drain{ctx};
  if (ec_lagrange_on_device(ctx, (double)m * (double)m, m, m)) {
    if (!ec_positions_distinct(positions_host, m)) return fail(ctx, MPVSS_E_INVALID, "ec_lagrange_scalars: duplicate positions");
    ec::lagrange_tiles(0, m, tiles);
    RET_IF(ensure(ctx, w.d, m * 32));
    drain.on = true;
    RET_IF(ec_lagrange_dev(ctx, gi, w.lag_pos, w.lag_tiles, positions_host, m, tiles, (uint8_t*)w.d.p));
    HIPCHK(ctx, hipMemcpyAsync(ks.data(), w.d.p, m * 32, hipMemcpyDeviceToHost, ctx->stream));
    RET_IF(spans_collect(ctx));
    ++ctx->ec_lagrange_dev_lists;
  } else {
    for (size_t i = 0; i < m; ++i)
      if (!ec_lagrange_scalar(gi, positions_host, m, i, ks.data() + i * 32)) return fail(ctx, MPVSS_E_INVALID, "ec_lagrange_scalars: duplicate positions");
    ++ctx->ec_lagrange_host_lists;
  }
  memcpy(scalars_out_host, ks.data(), m * 32);
  return MPVSS_OK;
}
