// C ABI of a run-time MODP group (include/mpvss_hip.h, "MODP groups of a run-time modulus"): the group handle, its
// host-side constants and hash_to_scalar, and the batched entry points over modp_rt_kernels.hip.  Included at the end
// of mpvss_capi.cpp (it uses the context, staging and transcript helpers defined there).

struct mpvss_modp_group {
  modp_rt_consts c;          // device image of the constants (copied to the device by every call)
  int bits = 0;
  int lpl = 0;
  uint8_t sub_be[256];       // (q-1)/2 big-endian: hash_to_scalar's modulus (modp.rs:142-148)
  uint8_t g_be[256];         // subgroup generator 4 (modp.rs:65-66 for any q >= 5)
  uint8_t G_be[256];         // main generator 2
};

namespace {

// ---- host big integers: little-endian 32-bit words, fixed capacity (2 q < 2^2050) ------------------------------
constexpr int RTW = 66;
typedef uint32_t RtNum[RTW];

void rt_from_be(RtNum x, const uint8_t* be, size_t len) {
  memset(x, 0, sizeof(RtNum));
  for (size_t i = 0; i < len; ++i) {
    const size_t bitpos = 8 * (len - 1 - i);
    x[bitpos / 32] |= (uint32_t)be[i] << (bitpos % 32);
  }
}
void rt_to_be256(const RtNum x, uint8_t* be) {
  for (int i = 0; i < 256; ++i) be[255 - i] = (uint8_t)(x[i / 4] >> (8 * (i % 4)));
}
int rt_cmp(const RtNum a, const RtNum b) {
  for (int i = RTW - 1; i >= 0; --i)
    if (a[i] != b[i]) return a[i] > b[i] ? 1 : -1;
  return 0;
}
void rt_sub(RtNum a, const RtNum b) {   // a -= b, a >= b
  uint64_t borrow = 0;
  for (int i = 0; i < RTW; ++i) {
    const uint64_t d = (uint64_t)a[i] - b[i] - borrow;
    a[i] = (uint32_t)d;
    borrow = (d >> 63) & 1;
  }
}
// a = (2 a + bit) mod n, a < n
void rt_dbl_mod(RtNum a, uint32_t bit, const RtNum n) {
  uint32_t c = bit;
  for (int i = 0; i < RTW; ++i) {
    const uint32_t v = (a[i] << 1) | c;
    c = a[i] >> 31;
    a[i] = v;
  }
  if (rt_cmp(a, n) >= 0) rt_sub(a, n);
}
int rt_bits(const RtNum a) {
  for (int i = RTW - 1; i >= 0; --i)
    if (a[i]) return 32 * i + 32 - __builtin_clz(a[i]);
  return 0;
}
// 2^e mod n
void rt_pow2_mod(RtNum out, int e, const RtNum n) {
  memset(out, 0, sizeof(RtNum));
  out[0] = 1;
  if (rt_cmp(out, n) >= 0) rt_sub(out, n);
  for (int i = 0; i < e; ++i) rt_dbl_mod(out, 0, n);
}
// 29-bit limbs (zero above L)
void rt_limbs(const RtNum x, uint32_t* limbs, int L) {
  memset(limbs, 0, MODP_RT_MAX_LIMBS * 4);
  for (int j = 0; j < L; ++j) {
    const int bit = 29 * j;
    const int w = bit / 32, s = bit % 32;
    uint64_t v = x[w] >> s;
    if (w + 1 < RTW) v |= (uint64_t)x[w + 1] << (32 - s);
    limbs[j] = (uint32_t)v & ((1u << 29) - 1);
  }
}

// width of a modulus: the smallest of 5, 9, 18 limbs per lane with bits <= 29 L - 2 (R > 4 N)
int rt_lpl_for_bits(int bits) {
  for (int lpl : {5, 9, 18})
    if (bits <= 29 * 4 * lpl - 2) return lpl;
  return 0;
}

// the call's device copy of the group constants (context workspace, stream order)
int rt_upload(mpvss_ctx* ctx, const mpvss_modp_group* grp, const modp_rt_consts** dev) {
  RET_IF(ensure(ctx, ctx->rt_consts, sizeof(modp_rt_consts)));
  HIPCHK(ctx, hipMemcpyAsync(ctx->rt_consts.p, &grp->c, sizeof(modp_rt_consts), hipMemcpyHostToDevice, ctx->stream));
  *dev = (const modp_rt_consts*)ctx->rt_consts.p;
  return 0;
}

size_t rt_L(const mpvss_modp_group* grp) { return (size_t)4 * grp->lpl; }

// 16-entry tables of `count` bases (base_stride 0: one shared base) into buf
int rt_tables(mpvss_ctx* ctx, const mpvss_modp_group* grp, const modp_rt_consts* dc, const uint8_t* bases_dev, size_t base_stride,
              size_t count, DevBuf& buf, const uint32_t** tab) {
  RET_IF(ensure(ctx, buf, count * 16 * rt_L(grp) * 4));
  TIMED_LAUNCH(ctx, 2, modp_rt_launch_table(grp->lpl, bases_dev, base_stride, (int)count, (uint32_t*)buf.p, dc, ctx->stream));
  *tab = (const uint32_t*)buf.p;
  return 0;
}

// a host 256-byte value on the device (small staging buffer of the context)
int rt_stage_small(mpvss_ctx* ctx, const uint8_t* host256, DevBuf& buf, const uint8_t** dev) {
  RET_IF(ensure(ctx, buf, EB));
  HIPCHK(ctx, hipMemcpyAsync(buf.p, host256, EB, hipMemcpyHostToDevice, ctx->stream));
  *dev = (const uint8_t*)buf.p;
  return 0;
}

// a1 = g1^r h1^c and a2 = g2^r h2^c for cnt shares (device pointers; g1 one shared base, c stride 0 = shared)
int rt_dleq_dev(mpvss_ctx* ctx, const mpvss_modp_group* grp, const modp_rt_consts* dc, const uint8_t* g1_dev, const uint8_t* h1,
                const uint8_t* g2, const uint8_t* h2, const uint8_t* r, const uint8_t* c, size_t c_stride, size_t cnt, uint8_t* a1,
                uint8_t* a2) {
  const size_t TW = 16 * rt_L(grp);
  const uint32_t *tg, *t1, *t2;
  if (a1) {
    RET_IF(rt_tables(ctx, grp, dc, g1_dev, 0, 1, ctx->rt_tabg, &tg));
    RET_IF(rt_tables(ctx, grp, dc, h1, EB, cnt, ctx->rt_tab1, &t1));
    TIMED_LAUNCH(ctx, 1, modp_rt_launch_dual_exp(grp->lpl, tg, 0, t1, TW, r, EB, c, c_stride, (int)cnt, a1, dc, ctx->stream));
  }
  if (a2) {
    RET_IF(rt_tables(ctx, grp, dc, g2, EB, cnt, ctx->rt_tab1, &t1));
    RET_IF(rt_tables(ctx, grp, dc, h2, EB, cnt, ctx->rt_tab2, &t2));
    TIMED_LAUNCH(ctx, 3, modp_rt_launch_dual_exp(grp->lpl, t1, TW, t2, TW, r, EB, c, c_stride, (int)cnt, a2, dc, ctx->stream));
  }
  return 0;
}

// X_i of cnt shares (commitments already in ctx->rt_cm, Montgomery form)
int rt_commit_eval_dev(mpvss_ctx* ctx, const mpvss_modp_group* grp, const modp_rt_consts* dc, size_t t, const int64_t* pos_dev,
                       size_t cnt, uint8_t* x_dev) {
  TIMED_LAUNCH(ctx, 0, modp_rt_launch_commit_eval(grp->lpl, (const uint32_t*)ctx->rt_cm.p, (int)t, pos_dev, (int)cnt, x_dev, dc,
                                                  ctx->stream));
  return 0;
}

int rt_stage_commitments(mpvss_ctx* ctx, const mpvss_modp_group* grp, const modp_rt_consts* dc, int space, const uint8_t* commitments,
                         size_t t) {
  const void* dcm;
  RET_IF(stage_in(ctx, space, commitments, t * EB, ctx->rt_in[4], &dcm));
  RET_IF(ensure(ctx, ctx->rt_cm, t * rt_L(grp) * 4));
  LAUNCHCHK(ctx, modp_rt_launch_to_mont(grp->lpl, (const uint8_t*)dcm, (int)t, (uint32_t*)ctx->rt_cm.p, dc, ctx->stream));
  return 0;
}

// hash_to_scalar of the group: int(SHA-256(data)) mod (q-1)/2, 256 bytes big-endian
void rt_hash_to_scalar(const mpvss_modp_group* grp, const uint8_t* data, size_t len, uint8_t out256[256]) {
  uint8_t h[32];
  mpvss::sha256(data, len, h);
  RtNum m, r;
  rt_from_be(m, grp->sub_be, EB);
  memset(r, 0, sizeof(RtNum));
  for (int i = 0; i < 256; ++i) rt_dbl_mod(r, (h[i / 8] >> (7 - i % 8)) & 1, m);
  rt_to_be256(r, out256);
}

bool rt_bad_group(const mpvss_modp_group* grp) { return grp == nullptr || grp->lpl == 0; }

}  // namespace

extern "C" int mpvss_modp_group_create(const uint8_t* q_be, size_t q_len, mpvss_modp_group** out) {
  if (!out) return MPVSS_E_INVALID;
  *out = nullptr;
  if (!q_be) return MPVSS_E_INVALID;
  size_t skip = 0;
  while (skip < q_len && q_be[skip] == 0) ++skip;          // leading zero bytes are allowed
  if (q_len - skip > EB) return MPVSS_E_INVALID;           // more than 2048 bits
  RtNum q;
  rt_from_be(q, q_be + skip, q_len - skip);
  const int bits = rt_bits(q);
  if (bits == 0 || (q[0] & 1) == 0 || (bits <= 3 && q[0] < 5)) return MPVSS_E_INVALID;   // even, or below 5
  mpvss_modp_group* g = new (std::nothrow) mpvss_modp_group();
  if (!g) return MPVSS_E_NOMEM;
  memset(&g->c, 0, sizeof(g->c));
  g->bits = bits;
  g->lpl = rt_lpl_for_bits(bits);
  const int L = 4 * g->lpl;
  const int in_rows = modp_rt_in_rows(g->lpl);
  rt_limbs(q, g->c.n, L);
  RtNum k;
  rt_pow2_mod(k, 29 * (in_rows + L), q);
  rt_limbs(k, g->c.kin, L);
  rt_pow2_mod(k, 29 * L, q);
  rt_limbs(k, g->c.one_m, L);
  g->c.one[0] = 1;
  // n0inv = -q^-1 mod 2^29 (Newton: every step doubles the correct low bits)
  uint32_t inv = q[0];
  for (int i = 0; i < 5; ++i) inv *= 2u - q[0] * inv;
  g->c.n0inv = (0u - inv) & ((1u << 29) - 1);
  g->c.lpl = (uint32_t)g->lpl;
  if (bits <= 64) {
    const uint64_t qm1 = (((uint64_t)q[1] << 32) | q[0]) - 1;
    g->c.qm1_lo = (uint32_t)qm1;
    g->c.qm1_hi = (uint32_t)(qm1 >> 32);
  }
  RtNum sub;
  memcpy(sub, q, sizeof(RtNum));
  for (int i = 0; i < RTW; ++i) sub[i] = (q[i] >> 1) | (i + 1 < RTW ? q[i + 1] << 31 : 0);   // (q-1)/2 = q >> 1 (q odd)
  rt_to_be256(sub, g->sub_be);
  memset(g->g_be, 0, EB);
  g->g_be[EB - 1] = 4;
  memset(g->G_be, 0, EB);
  g->G_be[EB - 1] = 2;
  *out = g;
  return MPVSS_OK;
}

extern "C" void mpvss_modp_group_destroy(mpvss_modp_group* grp) { delete grp; }

extern "C" int mpvss_modp_group_bits(const mpvss_modp_group* grp) { return grp ? grp->bits : MPVSS_E_INVALID; }

extern "C" int mpvss_modp_group_limbs_per_lane(const mpvss_modp_group* grp) { return grp ? grp->lpl : MPVSS_E_INVALID; }

extern "C" int mpvss_modp_group_hash_to_scalar(const mpvss_modp_group* grp, const uint8_t* data, size_t len, uint8_t out256[256]) {
  if (!grp || !out256 || (!data && len)) return MPVSS_E_INVALID;
  rt_hash_to_scalar(grp, data, len, out256);
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_batch_exp(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* bases,
                                          const uint8_t* exps, size_t n, uint8_t* out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_batch_exp: no group");
  if (n == 0) return MPVSS_OK;
  if (!bases || !exps || !out) return fail(ctx, MPVSS_E_INVALID, "group_batch_exp: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  spans_reset(ctx);
  const modp_rt_consts* dc;
  RET_IF(rt_upload(ctx, grp, &dc));
  for (size_t off = 0; off < n; off += MAX_CHUNK) {
    const size_t cnt = (n - off < MAX_CHUNK) ? n - off : MAX_CHUNK;
    const void *db, *de;
    RET_IF(stage_in(ctx, space, bases + off * EB, cnt * EB, ctx->rt_in[0], &db));
    RET_IF(stage_in(ctx, space, exps + off * EB, cnt * EB, ctx->rt_in[1], &de));
    uint8_t* dout = out + off * EB;
    if (space == MPVSS_HOST) {
      RET_IF(ensure(ctx, ctx->rt_out[0], cnt * EB));
      dout = (uint8_t*)ctx->rt_out[0].p;
    }
    const uint32_t* t1;
    RET_IF(rt_tables(ctx, grp, dc, (const uint8_t*)db, EB, cnt, ctx->rt_tab1, &t1));
    TIMED_LAUNCH(ctx, 3, modp_rt_launch_dual_exp(grp->lpl, t1, 16 * rt_L(grp), nullptr, 0, (const uint8_t*)de, EB, nullptr, 0, (int)cnt,
                                                 dout, dc, ctx->stream));
    if (space == MPVSS_HOST) RET_IF(copy_out(ctx, space, out + off * EB, dout, cnt * EB));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_batch_mul(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* a, const uint8_t* b,
                                          size_t n, uint8_t* out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_batch_mul: no group");
  if (n == 0) return MPVSS_OK;
  if (!a || !b || !out || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "group_batch_mul: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  spans_reset(ctx);
  const modp_rt_consts* dc;
  RET_IF(rt_upload(ctx, grp, &dc));
  const void *da, *db;
  RET_IF(stage_in(ctx, space, a, n * EB, ctx->rt_in[0], &da));
  RET_IF(stage_in(ctx, space, b, n * EB, ctx->rt_in[1], &db));
  uint8_t* dout = out;
  if (space == MPVSS_HOST) {
    RET_IF(ensure(ctx, ctx->rt_out[0], n * EB));
    dout = (uint8_t*)ctx->rt_out[0].p;
  }
  const size_t LW = rt_L(grp);
  RET_IF(ensure(ctx, ctx->rt_tab1, n * LW * 4));
  RET_IF(ensure(ctx, ctx->rt_tab2, n * LW * 4));
  LAUNCHCHK(ctx, modp_rt_launch_to_mont(grp->lpl, (const uint8_t*)da, (int)n, (uint32_t*)ctx->rt_tab1.p, dc, ctx->stream));
  LAUNCHCHK(ctx, modp_rt_launch_to_mont(grp->lpl, (const uint8_t*)db, (int)n, (uint32_t*)ctx->rt_tab2.p, dc, ctx->stream));
  LAUNCHCHK(ctx, modp_rt_launch_mul(grp->lpl, (const uint32_t*)ctx->rt_tab1.p, (const uint32_t*)ctx->rt_tab2.p, (int)n, dout, dc,
                                    ctx->stream));
  if (space == MPVSS_HOST) RET_IF(copy_out(ctx, space, out, dout, n * EB));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_commit_eval(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* commitments,
                                            size_t t, const int64_t* positions, size_t n, uint8_t* x_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_commit_eval: no group");
  if (n == 0) return MPVSS_OK;
  if (!commitments || !positions || !x_out || t == 0 || t > 0x7fffffff || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "group_commit_eval: bad argument (t must be >= 1)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  spans_reset(ctx);
  const modp_rt_consts* dc;
  RET_IF(rt_upload(ctx, grp, &dc));
  RET_IF(rt_stage_commitments(ctx, grp, dc, space, commitments, t));
  const int64_t* dpos;
  RET_IF(stage_positions(ctx, space, positions, n, &dpos));
  uint8_t* dout = x_out;
  if (space == MPVSS_HOST) {
    RET_IF(ensure(ctx, ctx->rt_out[0], n * EB));
    dout = (uint8_t*)ctx->rt_out[0].p;
  }
  RET_IF(rt_commit_eval_dev(ctx, grp, dc, t, dpos, n, dout));
  if (space == MPVSS_HOST) RET_IF(copy_out(ctx, space, x_out, dout, n * EB));
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_dleq_commitments(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* g1_host,
                                                 const uint8_t* h1, const uint8_t* g2, const uint8_t* h2, const uint8_t* r,
                                                 const uint8_t* c, int c_per_share, size_t n, uint8_t* a1_out, uint8_t* a2_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_dleq_commitments: no group");
  if (n == 0) return MPVSS_OK;
  if (!g1_host || !h1 || !g2 || !h2 || !r || !c || !a1_out || !a2_out || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "group_dleq_commitments: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  spans_reset(ctx);
  const modp_rt_consts* dc;
  RET_IF(rt_upload(ctx, grp, &dc));
  const uint8_t *dg1 = nullptr, *dcc = nullptr;
  RET_IF(rt_stage_small(ctx, g1_host, ctx->rt_small[0], &dg1));
  if (!c_per_share) RET_IF(rt_stage_small(ctx, c, ctx->rt_small[1], &dcc));
  for (size_t off = 0; off < n; off += MAX_CHUNK) {
    const size_t cnt = (n - off < MAX_CHUNK) ? n - off : MAX_CHUNK;
    const void *dh1, *dg2, *dh2, *dr, *dcs = dcc;
    RET_IF(stage_in(ctx, space, h1 + off * EB, cnt * EB, ctx->rt_in[0], &dh1));
    RET_IF(stage_in(ctx, space, g2 + off * EB, cnt * EB, ctx->rt_in[1], &dg2));
    RET_IF(stage_in(ctx, space, h2 + off * EB, cnt * EB, ctx->rt_in[2], &dh2));
    RET_IF(stage_in(ctx, space, r + off * EB, cnt * EB, ctx->rt_in[3], &dr));
    if (c_per_share) RET_IF(stage_in(ctx, space, c + off * EB, cnt * EB, ctx->rt_in[5], &dcs));
    uint8_t* d1 = a1_out + off * EB;
    uint8_t* d2 = a2_out + off * EB;
    if (space == MPVSS_HOST) {
      RET_IF(ensure(ctx, ctx->rt_out[0], cnt * EB));
      RET_IF(ensure(ctx, ctx->rt_out[1], cnt * EB));
      d1 = (uint8_t*)ctx->rt_out[0].p;
      d2 = (uint8_t*)ctx->rt_out[1].p;
    }
    RET_IF(rt_dleq_dev(ctx, grp, dc, dg1, (const uint8_t*)dh1, (const uint8_t*)dg2, (const uint8_t*)dh2, (const uint8_t*)dr,
                       (const uint8_t*)dcs, c_per_share ? EB : 0, cnt, d1, d2));
    if (space == MPVSS_HOST) {
      RET_IF(copy_out(ctx, space, a1_out + off * EB, d1, cnt * EB));
      RET_IF(copy_out(ctx, space, a2_out + off * EB, d2, cnt * EB));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_verify_distribution(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* commitments,
                                                    size_t t, const int64_t* positions, const uint8_t* pubkeys, const uint8_t* shares,
                                                    const uint8_t* responses, size_t n, const uint8_t* challenge_host, int* verdict,
                                                    uint8_t* digest32_out, uint8_t* x_out_host, uint8_t* a1_out_host,
                                                    uint8_t* a2_out_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_verify_distribution: no group");
  if (!verdict || !challenge_host || n > 0x7fffffff || t > 0x7fffffff ||
      (n > 0 && (!commitments || !positions || !pubkeys || !shares || !responses || t == 0)))
    return fail(ctx, MPVSS_E_INVALID, "group_verify_distribution: bad argument");
  *verdict = 0;
  mpvss::Sha256 h;
  if (n > 0) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    spans_reset(ctx);
    const modp_rt_consts* dc;
    RET_IF(rt_upload(ctx, grp, &dc));
    RET_IF(rt_stage_commitments(ctx, grp, dc, space, commitments, t));
    const uint8_t *dg, *dch;
    RET_IF(rt_stage_small(ctx, grp->g_be, ctx->rt_small[0], &dg));
    RET_IF(rt_stage_small(ctx, challenge_host, ctx->rt_small[1], &dch));
    const size_t chunk = std::min(n, MAX_CHUNK);
    std::vector<uint8_t> hX(chunk * EB), hY(chunk * EB), h1(chunk * EB), h2(chunk * EB);
    for (size_t off = 0; off < n; off += MAX_CHUNK) {
      const size_t cnt = (n - off < MAX_CHUNK) ? n - off : MAX_CHUNK;
      const int64_t* dpos;
      RET_IF(stage_positions(ctx, space, positions + off, cnt, &dpos));
      const void *dy, *dY, *dr;
      RET_IF(stage_in(ctx, space, pubkeys + off * EB, cnt * EB, ctx->rt_in[1], &dy));
      RET_IF(stage_in(ctx, space, shares + off * EB, cnt * EB, ctx->rt_in[2], &dY));
      RET_IF(stage_in(ctx, space, responses + off * EB, cnt * EB, ctx->rt_in[3], &dr));
      for (DevBuf* b : {&ctx->rt_out[0], &ctx->rt_out[1], &ctx->rt_out[2]}) RET_IF(ensure(ctx, *b, cnt * EB));
      uint8_t* dX = (uint8_t*)ctx->rt_out[0].p;
      uint8_t* d1 = (uint8_t*)ctx->rt_out[1].p;
      uint8_t* d2 = (uint8_t*)ctx->rt_out[2].p;
      RET_IF(rt_commit_eval_dev(ctx, grp, dc, t, dpos, cnt, dX));
      // a1 = g^r X^c, a2 = y^r Y^c (src/participant.rs:436-447 -> src/dleq.rs:66-84)
      RET_IF(rt_dleq_dev(ctx, grp, dc, dg, dX, (const uint8_t*)dy, (const uint8_t*)dY, (const uint8_t*)dr, dch, 0, cnt, d1, d2));
      HIPCHK(ctx, hipMemcpyAsync(hX.data(), dX, cnt * EB, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipMemcpyAsync(h1.data(), d1, cnt * EB, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipMemcpyAsync(h2.data(), d2, cnt * EB, hipMemcpyDeviceToHost, ctx->stream));
      if (space == MPVSS_DEVICE) HIPCHK(ctx, hipMemcpyAsync(hY.data(), dY, cnt * EB, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      const uint8_t* Y = (space == MPVSS_DEVICE) ? hY.data() : shares + off * EB;
      // the transcript hashes Y_i as the box carries it (src/participant.rs:448), X_i, a1_i, a2_i canonical
      for (size_t i = 0; i < cnt; ++i) {
        frame_update(h, hX.data() + i * EB);
        frame_update(h, Y + i * EB);
        frame_update(h, h1.data() + i * EB);
        frame_update(h, h2.data() + i * EB);
      }
      if (x_out_host) memcpy(x_out_host + off * EB, hX.data(), cnt * EB);
      if (a1_out_host) memcpy(a1_out_host + off * EB, h1.data(), cnt * EB);
      if (a2_out_host) memcpy(a2_out_host + off * EB, h2.data(), cnt * EB);
    }
    RET_IF(spans_collect(ctx));
  }
  uint8_t digest[32], c[256];
  h.final(digest);
  if (digest32_out) memcpy(digest32_out, digest, 32);
  rt_hash_to_scalar(grp, digest, 32, c);          // src/participant.rs:451-455
  *verdict = memcmp(c, challenge_host, EB) == 0 ? 1 : 0;
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_verify_shares(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* pk,
                                              const uint8_t* s, const uint8_t* y, const uint8_t* c, const uint8_t* r, size_t n,
                                              uint8_t* verdicts_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_verify_shares: no group");
  if (n == 0) return MPVSS_OK;
  if (!pk || !s || !y || !c || !r || !verdicts_host || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "group_verify_shares: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  spans_reset(ctx);
  const modp_rt_consts* dc;
  RET_IF(rt_upload(ctx, grp, &dc));
  const uint8_t* dG;
  RET_IF(rt_stage_small(ctx, grp->G_be, ctx->rt_small[0], &dG));
  const size_t chunk = std::min(n, MAX_CHUNK);
  std::vector<uint8_t> hpk, hY, hc, h1(chunk * EB), h2(chunk * EB);
  if (space == MPVSS_DEVICE) { hpk.resize(chunk * EB); hY.resize(chunk * EB); hc.resize(chunk * EB); }
  for (size_t off = 0; off < n; off += MAX_CHUNK) {
    const size_t cnt = (n - off < MAX_CHUNK) ? n - off : MAX_CHUNK;
    const void *dpk, *ds, *dy, *dcc, *dr;
    RET_IF(stage_in(ctx, space, pk + off * EB, cnt * EB, ctx->rt_in[0], &dpk));
    RET_IF(stage_in(ctx, space, s + off * EB, cnt * EB, ctx->rt_in[1], &ds));
    RET_IF(stage_in(ctx, space, y + off * EB, cnt * EB, ctx->rt_in[2], &dy));
    RET_IF(stage_in(ctx, space, c + off * EB, cnt * EB, ctx->rt_in[5], &dcc));
    RET_IF(stage_in(ctx, space, r + off * EB, cnt * EB, ctx->rt_in[3], &dr));
    RET_IF(ensure(ctx, ctx->rt_out[1], cnt * EB));
    RET_IF(ensure(ctx, ctx->rt_out[2], cnt * EB));
    uint8_t* d1 = (uint8_t*)ctx->rt_out[1].p;
    uint8_t* d2 = (uint8_t*)ctx->rt_out[2].p;
    // a1 = G^r pk^c, a2 = S^r Y^c (src/participant.rs:361-386 -> src/dleq.rs:275-302)
    RET_IF(rt_dleq_dev(ctx, grp, dc, dG, (const uint8_t*)dpk, (const uint8_t*)ds, (const uint8_t*)dy, (const uint8_t*)dr,
                       (const uint8_t*)dcc, EB, cnt, d1, d2));
    HIPCHK(ctx, hipMemcpyAsync(h1.data(), d1, cnt * EB, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h2.data(), d2, cnt * EB, hipMemcpyDeviceToHost, ctx->stream));
    if (space == MPVSS_DEVICE) {
      HIPCHK(ctx, hipMemcpyAsync(hpk.data(), pk + off * EB, cnt * EB, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipMemcpyAsync(hY.data(), y + off * EB, cnt * EB, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipMemcpyAsync(hc.data(), c + off * EB, cnt * EB, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const uint8_t* P = space == MPVSS_DEVICE ? hpk.data() : pk + off * EB;
    const uint8_t* Y = space == MPVSS_DEVICE ? hY.data() : y + off * EB;
    const uint8_t* C = space == MPVSS_DEVICE ? hc.data() : c + off * EB;
    for (size_t i = 0; i < cnt; ++i) {
      mpvss::Sha256 hs;
      frame_update(hs, P + i * EB);
      frame_update(hs, Y + i * EB);
      frame_update(hs, h1.data() + i * EB);
      frame_update(hs, h2.data() + i * EB);
      uint8_t digest[32], cc[256];
      hs.final(digest);
      rt_hash_to_scalar(grp, digest, 32, cc);     // src/dleq.rs:119-126
      verdicts_host[off + i] = memcmp(cc, C + i * EB, EB) == 0 ? 1 : 0;
    }
  }
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}
